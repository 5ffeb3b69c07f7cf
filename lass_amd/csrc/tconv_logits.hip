// tconv_logits.hip - decoder_block6's transposed conv with the folded head's shortcut logits of its output formed in the same
// launch (conv_route.h: head_sc_fold; head_fold.h: Wt').  The kernel is conv.hip's single-buffered 1-tap kernel with 12 more
// columns, and a kernel of its own because the planes need a second argument block (the kernels that take ConvArgs alone keep theirs); it lives in a translation unit of its own because hipcc allocates conv.hip's existing kernels differently as soon as a
// further kernel in that file instantiates the same Phase.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "conv_common.h"
#include "conv_phase.h"
#include "wino_common.h"  // block_coords: the XCD-aware workgroup order

namespace {

// conv_kernel_sb<1, 2, NPX, PW, F_PRO | F_TCONV> whose workgroups also form the 12 live columns (3 logits x 2 x 2 sub-pixels) of the
// slab hs.w = Wt' [Cin][64] (head_fold.h) over the activated input tile they have staged anyway, and store them as three planes at
// the up-sampled resolution.  The NPX cout blocks of a tile share the work: block by takes pixel row by of each wave's NPX rows.
// Per chunk a workgroup stages 16 rows x 16 columns of the slab behind the chunk's own weights (columns 12 .. 15 are zeros of the
// slab) and contracts them on ONE 16-row tile of v_mfma_f32_16x16x4_f32 per 16 pixels: 12 of 16 rows live, 8 MFMAs of 8 passes per
// wave and chunk beside the 32 of 16 passes of the transposed conv itself.  Each accumulator sums its input channels in ascending
// order, as the 32x32x2 tile of the extra cout block did that this replaces (which staged and activated the whole tile a third
// time for these 12 columns).
template <int NPX, int PW>
struct TconvLogits {
    using PA = Phase<1, 16, 2, NPX, PW, true>;
    static constexpr int NT = PA::NT, CH_ELEMS = PA::CH_ELEMS, IN_ELEMS = PA::IN_ELEMS, IP = PA::IP, PH = PA::PH, WROWS = PA::WROWS;
    static constexpr int LROWS = 16;                    // rows of the logit tile: slab columns 0 .. 15
    static constexpr int LW_FLOATS = 16 * LROWS;        // one chunk of them: [channel 16][column 16], one float per thread
    static_assert(PW == 32 && PH == 1 && LW_FLOATS == NTHREADS, "two 16-pixel tiles per pixel row; one slab element per thread");

    // lane (kq, l15): A = Wt'[channel 4 s + kq][column l15], B = act[channel 4 s + kq][pixel row prow, x = 16 h + l15]
    __device__ __forceinline__ static void compute(const float* lds, const float* lwl, f32x4 (&lacc)[2], int lane, int wave, int prow) {
        const int kq = lane >> 4, l15 = lane & 15;
        const float* bbase = lds + kq * CH_ELEMS + (wave * WROWS + prow) * IP + l15;
        const float* abase = lwl + kq * LROWS + l15;
        constexpr int S = 16 / 4;  // k-steps: four channels
        float a[2], b[2][2];
        auto rd = [&](int s, float& aa, float (&bb)[2]) {
            aa = abase[s * 4 * LROWS];
            bb[0] = bbase[s * 4 * CH_ELEMS];
            bb[1] = bbase[s * 4 * CH_ELEMS + 16];
        };
        rd(0, a[0], b[0]);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s + 1 < S) rd(s + 1, a[(s + 1) & 1], b[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            lacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1], b[s & 1][0], lacc[0], 0, 0, 0);
            lacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s & 1], b[s & 1][1], lacc[1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // D row 4 kq + r = column (q, a, bb) of the slab: lane (kq = q < 3, l15) holds the 2 x 2 sub-pixels r = 2 a + bb of logit q at
    // its pixel - 8 contiguous bytes per output row, as tconv_store
    __device__ __forceinline__ static void store_planes(const ConvArgs& p, float* up, f32x4 (&lacc)[2], int b, int y0, int x0, int lane, int wave,
                                                        int prow) {
        const int q = lane >> 4, l15 = lane & 15;
        const int y = y0 + wave * WROWS + prow;
        if (y >= p.H || q >= 3) return;
        const int oW = p.W * 2;
        const size_t oHW = (size_t)p.H * p.W * 4;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int x = x0 + 16 * h + l15;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                float* dst = up + ((size_t)b * 3 + q) * oHW + (size_t)(y * 2 + a) * oW + x * 2;
                *reinterpret_cast<float2*>(dst) = make_float2(lacc[h][2 * a], lacc[h][2 * a + 1]);
            }
        }
    }
};

template <int NPX, int PW>
__global__ __launch_bounds__(NTHREADS, 4) void tconv_logits_kernel(ConvArgs p, HeadScPlanes hs) {
    using TL = TconvLogits<NPX, PW>;
    using PA = typename TL::PA;
    constexpr int PHT = PA::PHT, NT = PA::NT;
    __shared__ __attribute__((aligned(16))) float lds[PA::LDS_FLOATS + TL::LW_FLOATS];
    float* lwl = lds + PA::LDS_FLOATS;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);  // (gy = NPX: host-checked)
    const int n0 = by_ * NT;
    const int tiles_x = p.W / PW;
    const int y0 = (bx_ / tiles_x) * PHT, x0 = (bx_ % tiles_x) * PW;
    const int HW = p.H * p.W;
    const int nA = p.Cin / 16;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = p.pro_scale;
    const float* sh = p.pro_shift + (size_t)b * p.pro_shift_bs;

    PA pa;
    const auto rs = [](const float* ptr, long bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ptr), 0, (int)bytes, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t in_rs = rs(in_b, (long)p.Cin * HW * 4);
    const __amdgpu_buffer_rsrc_t wa_rs = rs(p.w + n0, ((long)p.Cin * p.Nw - n0) * 4);
    const __amdgpu_buffer_rsrc_t wl_rs = rs(hs.w, (long)p.Cin * NT * 4);  // the slab's pitch is NT = 64 columns (kHeadScCols)
    const unsigned wl_off = 4u * (unsigned)((tid >> 4) * NT + (tid & 15));
    float wl;  // this thread's slab element of the prefetched chunk
    auto loadA = [&](int c) {
        pa.load(in_rs, (unsigned)(c * 16 * HW) * 4u, HW, wa_rs, (unsigned)(c * 16 * p.Nw) * 4u, sc + c * 16, sh + c * 16);
        wl = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(wl_rs, (int)wl_off, (int)((unsigned)(c * 16 * NT) * 4u), 0));
    };
    auto storeA = [&]() {
        pa.store(lds, tid);
        lwl[tid] = wl;
    };
    pa.init(tid, y0, x0, p.H, p.W);
    pa.init_w(tid, p.Nw);
    loadA(0);
    storeA();
    __syncthreads();

    f32x16 acc[2][NPX];
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int px = 0; px < NPX; ++px)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[co][px][r] = 0.f;
    f32x4 lacc[2];  // [16-pixel half of pixel row by][sub-pixel], logit lane >> 4
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) lacc[h][r] = 0.f;

    for (int ch = 0; ch + 1 < nA; ++ch) {
        loadA(ch + 1);
        PA::compute(lds, acc, lane, wave);
        TL::compute(lds, lwl, lacc, lane, wave, by_);
        __syncthreads();
        storeA();
        __syncthreads();
    }
    PA::compute(lds, acc, lane, wave);
    TL::compute(lds, lwl, lacc, lane, wave, by_);
    TL::store_planes(p, hs.up, lacc, b, y0, x0, lane, wave, by_);
    tconv_store<2, NPX, PW>(p, acc, b, n0, y0, x0, lane, wave);
}

}  // namespace

// lass_tconv_logits_shape (conv_route.h) && the pointers are there; f32 output only; one cout block per pixel row of a wave (the
// blocks share the planes row by row: decoder_block6's 32 x 2 x 2 = 128 columns are two blocks)
bool lass_tconv_logits_supported(const ConvArgs& p, const HeadScPlanes& hs) {
    return p.B > 0 && p.in && p.w && p.out && p.pro_scale && p.pro_shift && !p.out_bf16 && p.N == p.Nw && p.N % 4 == 0 && p.N / 64 == 2 &&
           lass_tconv_logits_shape(p.Cin, p.N / 4, p.up_h, 2, p.H, p.W) && hs.up && hs.w;
}

hipError_t lass_launch_tconv_logits(const ConvArgs& p0, const HeadScPlanes& hs, hipStream_t stream) {
    if (!lass_tconv_logits_supported(p0, hs)) return hipErrorInvalidValue;
    constexpr int NPX = 2, PW = 32, PHT = 4 * NPX * (32 / PW);  // launch_geom's tile of a 1-tap conv at W >= 32
    ConvArgs p = p0;
    p.gx = (p.W / PW) * ((p.H + PHT - 1) / PHT);
    p.gy = p.N / 64;
    static_assert(NPX == 2, "lass_tconv_logits_supported: as many cout blocks as pixel rows of a wave");
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((tconv_logits_kernel<NPX, PW>), dim3((unsigned)((long)p.gx * p.gy * p.B)), dim3(NTHREADS), 0, stream, p, hs);
    return hipGetLastError();
}
