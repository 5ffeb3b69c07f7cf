// tconv_logits.hip - decoder_block6's transposed conv with the folded head's shortcut logits of its output formed in the same
// launch (conv_route.h: head_sc_fold; head_fold.h: Wt').  The kernel is conv.hip's single-buffered 1-tap kernel with one more cout
// block, and a kernel of its own because the planes need a second argument block (the kernels that take ConvArgs alone keep theirs); it lives in a translation unit of its own because hipcc allocates conv.hip's existing kernels differently as soon as a
// further kernel in that file instantiates the same Phase.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "conv_common.h"
#include "conv_phase.h"
#include "wino_common.h"  // block_coords: the XCD-aware workgroup order

namespace {

// conv_kernel_sb<1, 2, NPX, PW, F_PRO | F_TCONV> with one more cout block in the same launch.  Blocks 0 .. gy - 2 are the transposed
// conv as it is (64 columns of Wt each).  Block gy - 1 stages the same activated input tile - block_coords puts it on the XCD of
// the blocks that fetched the tile - and the 64-column slab hs.w = Wt' [Cin][64] (head_fold.h), contracts the FIRST 32-column tile
// only (compute_tile0: half the MFMAs of a block) and stores its 12 live columns (3 logits x 2 x 2 sub-pixels) as three planes at
// the up-sampled resolution.  One body for both kinds of block - staging, registers and the chunk loop are those of the
// transposed conv; what differs is workgroup-uniform: the weight base, the contraction called per chunk, the store.
template <int NPX, int PW>
struct TconvLogits {
    using PA = Phase<1, 16, 2, NPX, PW, true>;
    static constexpr int NT = PA::NT, CH_ELEMS = PA::CH_ELEMS, IN_ELEMS = PA::IN_ELEMS, IP = PA::IP, PH = PA::PH, WROWS = PA::WROWS;

    // PA::compute for cout tile 0 alone (the slab in LDS keeps its 64-column pitch)
    __device__ __forceinline__ static void compute_tile0(const float* lds, f32x16 (&acc)[2][NPX], int lane, int wave) {
        const int khalf = lane >> 5, j = lane & 31;
        const int ty = j / PW, tx = j % PW;
        const float* bbase = lds + khalf * CH_ELEMS + (wave * WROWS + ty) * IP + tx;
        const float* abase = lds + IN_ELEMS + khalf * NT + j;
        constexpr int S = 16 / 2;  // k-steps: channel pairs
        float a[2], b[2][NPX];
        auto rd = [&](int s, float& aa, float (&bb)[NPX]) {
            aa = abase[s * 2 * NT];
#pragma unroll
            for (int px = 0; px < NPX; ++px) bb[px] = bbase[s * 2 * CH_ELEMS + px * PH * IP];
        };
        rd(0, a[0], b[0]);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s + 1 < S) rd(s + 1, a[(s + 1) & 1], b[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int px = 0; px < NPX; ++px)
                acc[0][px] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1], b[s & 1][px], acc[0][px], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // column n = (r & 3) + 8 (r >> 2) + 4 khalf = (q, a, bb) of logit q = n >> 2, live below 12: registers (r, r + 1), r even, are
    // bb = 0 / 1 of one (q, a) - 8 contiguous bytes per lane, as tconv_store
    __device__ __forceinline__ static void store_planes(const ConvArgs& p, float* up, f32x16 (&acc)[2][NPX], int b, int y0, int x0, int lane,
                                                        int wave) {
        const int khalf = lane >> 5, j = lane & 31;
        const int ty = j / PW, tx = j % PW;
        const int x = x0 + tx;
        const int oW = p.W * 2;
        const size_t oHW = (size_t)p.H * p.W * 4;
#pragma unroll
        for (int px = 0; px < NPX; ++px) {
            const int y = y0 + wave * WROWS + px * PH + ty;
            if (y >= p.H) continue;
#pragma unroll
            for (int r = 0; r < 8; r += 2) {
                const int n = (r & 3) + 8 * (r >> 2) + 4 * khalf;
                if (n >= 12) continue;
                const int q = n >> 2, a = (n & 3) >> 1;
                float* dst = up + ((size_t)b * 3 + q) * oHW + (size_t)(y * 2 + a) * oW + x * 2;
                *reinterpret_cast<float2*>(dst) = make_float2(acc[0][px][r], acc[0][px][r + 1]);
            }
        }
    }
};

template <int NPX, int PW>
__global__ __launch_bounds__(NTHREADS, 4) void tconv_logits_kernel(ConvArgs p, HeadScPlanes hs) {
    using TL = TconvLogits<NPX, PW>;
    using PA = typename TL::PA;
    constexpr int PHT = PA::PHT, NT = PA::NT;
    __shared__ __attribute__((aligned(16))) float lds[PA::LDS_FLOATS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);
    const bool logits = by_ + 1 == p.gy;  // (workgroup-uniform)
    const int n0 = logits ? 0 : by_ * NT;
    const float* w = logits ? hs.w : p.w;
    const int Nw = logits ? NT : p.Nw;
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
    const __amdgpu_buffer_rsrc_t wa_rs = rs(w + n0, ((long)p.Cin * Nw - n0) * 4);
    auto loadA = [&](int c) {
        pa.load(in_rs, (unsigned)(c * 16 * HW) * 4u, HW, wa_rs, (unsigned)(c * 16 * Nw) * 4u, sc + c * 16, sh + c * 16);
    };
    pa.init(tid, y0, x0, p.H, p.W);
    pa.init_w(tid, Nw);
    loadA(0);
    pa.store(lds, tid);
    __syncthreads();

    f32x16 acc[2][NPX];
#pragma unroll
    for (int co = 0; co < 2; ++co)
#pragma unroll
        for (int px = 0; px < NPX; ++px)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[co][px][r] = 0.f;

    // the chunk loop once per kind of block, under one workgroup-uniform branch: hipcc keeps ONE set of accumulators that way
    if (logits) {
        for (int ch = 0; ch + 1 < nA; ++ch) {
            loadA(ch + 1);
            TL::compute_tile0(lds, acc, lane, wave);
            __syncthreads();
            pa.store(lds, tid);
            __syncthreads();
        }
        TL::compute_tile0(lds, acc, lane, wave);
        TL::store_planes(p, hs.up, acc, b, y0, x0, lane, wave);
    } else {
        for (int ch = 0; ch + 1 < nA; ++ch) {
            loadA(ch + 1);
            PA::compute(lds, acc, lane, wave);
            __syncthreads();
            pa.store(lds, tid);
            __syncthreads();
        }
        PA::compute(lds, acc, lane, wave);
        tconv_store<2, NPX, PW>(p, acc, b, n0, y0, x0, lane, wave);
    }
}

}  // namespace

// lass_tconv_logits_shape (conv_route.h) && the pointers are there; f32 output only
bool lass_tconv_logits_supported(const ConvArgs& p, const HeadScPlanes& hs) {
    return p.B > 0 && p.in && p.w && p.out && p.pro_scale && p.pro_shift && !p.out_bf16 && p.N == p.Nw && p.N % 4 == 0 &&
           lass_tconv_logits_shape(p.Cin, p.N / 4, p.up_h, 2, p.H, p.W) && hs.up && hs.w;
}

hipError_t lass_launch_tconv_logits(const ConvArgs& p0, const HeadScPlanes& hs, hipStream_t stream) {
    if (!lass_tconv_logits_supported(p0, hs)) return hipErrorInvalidValue;
    constexpr int NPX = 2, PW = 32, PHT = 4 * NPX * (32 / PW);  // launch_geom's tile of a 1-tap conv at W >= 32
    ConvArgs p = p0;
    p.gx = (p.W / PW) * ((p.H + PHT - 1) / PHT);
    p.gy = p.N / 64 + 1;
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((tconv_logits_kernel<NPX, PW>), dim3((unsigned)((long)p.gx * p.gy * p.B)), dim3(NTHREADS), 0, stream, p, hs);
    return hipGetLastError();
}
