// conv.hip - implicit-GEMM 3x3 / 1x1 / transposed convolutions of the ResUNet30 on gfx950 f32 MFMA.
//
// Replaces (reference: /root/reference/models/resunet.py):
//   ConvBlockRes.forward   :147-165   x1 = conv1(leaky(bn1(x)+b1)); x2 = conv2(leaky(bn2(x1)+b2)); out = sc(x) + x2
//   DecoderBlockRes1B.forward :254-255 x = conv1_T(leaky(bn1(x)+b1))   (kernel == stride, no overlap)
//
// GEMM view (per clip b):  D[n][p] = sum_k A[n][k] * B[k][p]
//   n = output channel (rows of D  -> the 16 accumulator registers of v_mfma_f32_32x32x2_f32)
//   p = output pixel   (cols of D  -> the lane, so NCHW stores are 128-B contiguous per half-wave)
//   k = (input channel, tap)
// A comes from the re-laid-out weights Wt[cin][tap][cout] (cout contiguous), B from a planar LDS halo tile
// [cin][row][col]; both fragments are single conflict-free ds_read_b32 per MFMA operand, register-prefetched one
// k-step ahead.  The f32 MFMA is a bit-exact f32 FMA chain, so results differ from the reference only by summation
// order.
//
// Fusions: BN(eval)+FiLM+leaky-ReLU as a prologue while staging the halo tile (zero padding is applied AFTER the
// activation, as conv padding does; the per-channel scale/shift are wave-uniform scalars because a staging pass
// covers exactly one channel pair), the block's second activation as conv1's epilogue (tables in LDS), the identity
// residual / shortcut bias as the INITIAL accumulator, the 1x1 shortcut conv as a second K-phase into the same
// accumulators, transposed-conv scatter, channel-slice ("virtual concat") output via batch strides.
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "conv_common.h"
#include "conv_phase.h"   // Phase: staging and contraction of one K-phase
#include "wino_common.h"  // block_coords: the XCD-aware workgroup order

namespace {

template <int A, int B>
struct MaxI {
    static constexpr int v = A > B ? A : B;
};


// ---- single-tile kernel, double-buffered LDS (one barrier per chunk) --------------------------------------------------
template <int TAPS, int NCO, int NPX, int PW, int FLAGS>
__global__ __launch_bounds__(NTHREADS) void conv_kernel_db(ConvArgs p) {
    constexpr bool PRO = (FLAGS & F_PRO) != 0;
    constexpr int KCA = (TAPS == 9) ? 8 : 16;
    using PA = Phase<TAPS, KCA, NCO, NPX, PW, PRO>;
    using PB = Phase<1, 16, NCO, NPX, PW, false>;
    constexpr int LDS_ONE = (FLAGS & F_PHASEB) ? MaxI<PA::LDS_FLOATS, PB::LDS_FLOATS>::v : PA::LDS_FLOATS;
    constexpr int LDS_MAIN = 2 * LDS_ONE;
    constexpr int PH = PA::PH, WROWS = PA::WROWS, PHT = PA::PHT, NT = PA::NT;
    constexpr bool EPI = (FLAGS & F_EPIACT) != 0;

    static_assert(LDS_MAIN % 4 == 0, "epilogue tables are read as float4");
    __shared__ __attribute__((aligned(16))) float lds[LDS_MAIN + (EPI ? 2 * NT : 0)];
    float* lds_es = lds + LDS_MAIN;  // epilogue scale / shift for this block's NT output channels
    float* lds_eh = lds_es + NT;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);  // 1-D grid: the cout blocks of one input tile on one XCD (wino_common.h)
    const int n0 = by_ * NT;
    const int tiles_x = p.W / PW;
    const int y0 = (bx_ / tiles_x) * PHT;
    const int x0 = (bx_ % tiles_x) * PW;
    const int HW = p.H * p.W;
    const int khalf = lane >> 5, j = lane & 31;
    const int ty = j / PW, tx = j % PW;
    const int x = x0 + tx;

    if (EPI) {
        if (tid < NT) {
            lds_es[tid] = p.epi_scale[n0 + tid];
            lds_eh[tid] = p.epi_shift[(size_t)b * p.epi_shift_bs + n0 + tid];
        }
    }

    // ---- accumulator initialisation: 0, the shortcut bias, or the identity residual ---------------------------
    f32x16 acc[NCO][NPX];
#pragma unroll
    for (int co = 0; co < NCO; ++co)
#pragma unroll
        for (int px = 0; px < NPX; ++px) {
            const int y = y0 + wave * WROWS + px * PH + ty;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + co * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf;
                float v = 0.f;
                if (FLAGS & F_BIAS) v = p.bias[n];
                if (FLAGS & F_RES)  // unconditional (row clamped; rows >= H are never stored)
                    v = p.res[(size_t)b * p.res_bs + (size_t)n * HW + (size_t)min(y, p.H - 1) * p.W + x];
                acc[co][px][r] = v;
            }
        }

    const float* sc = PRO ? p.pro_scale : nullptr;
    const float* sh = PRO ? p.pro_shift + (size_t)b * p.pro_shift_bs : nullptr;
    {
        PA ph;
        ph.run_db(lds, LDS_ONE, p.in + (size_t)b * p.in_bs, p.Cin, HW, p.w, p.Nw, n0, sc, sh, acc, tid, y0, x0, p.H,
                  p.W);
    }
    if (FLAGS & F_PHASEB) {
        PB ph;
        ph.run_db(lds, LDS_ONE, p.in2 + (size_t)b * p.in2_bs, p.Cin2, HW, p.w2, p.Nw, n0, nullptr, nullptr, acc, tid,
                  y0, x0, p.H, p.W);
    }

    // ---- epilogue ---------------------------------------------------------------------------------------------
    if (FLAGS & F_TCONV) {
        tconv_store<NCO, NPX, PW>(p, acc, b, n0, y0, x0, lane, wave);
    } else {
        store_tile<NCO, NPX, PW, (FLAGS & ~F_RES), false>(p, acc, nullptr, lds_es, lds_eh, b, n0, y0, x0, lane, wave);
    }
}

// ---- single-tile kernel, single-buffered LDS (two barriers per chunk, highest occupancy) ------------------------------
// Used for the 32-wide output tiles, the few-chunk layers and the 1-tap kernels.  Everything that has to come from HBM
// before the next contraction can start is requested one contraction earlier: chunk c+1 during chunk c, the shortcut
// phase's first chunk and the identity residual during the main phase's last chunk.
// (A multi-tile variant with cross-tile prefetch was measured and brought nothing: on these layers the matrix pipe is
// already ~90 % busy and the chip holds only ~1.9 GHz under their HBM + LDS load - see DESIGN.md.)
template <int TAPS, int NCO, int NPX, int PW, int FLAGS>
__global__ __launch_bounds__(NTHREADS) void conv_kernel_sb(ConvArgs p) {
    constexpr bool PRO = (FLAGS & F_PRO) != 0;
    constexpr bool HASB = (FLAGS & F_PHASEB) != 0;
    constexpr bool EPI = (FLAGS & F_EPIACT) != 0;
    constexpr bool BIAS = (FLAGS & F_BIAS) != 0;
    constexpr bool RES = (FLAGS & F_RES) != 0;
    constexpr bool RES_PF = RES && NCO == 1;  // residual prefetched into registers during the last chunk
    constexpr int KCA = (TAPS == 9) ? 8 : 16;
    using PA = Phase<TAPS, KCA, NCO, NPX, PW, PRO>;
    using PB = Phase<1, 16, NCO, NPX, PW, false>;
    constexpr int LDS_ONE = HASB ? MaxI<PA::LDS_FLOATS, PB::LDS_FLOATS>::v : PA::LDS_FLOATS;
    constexpr int PH = PA::PH, WROWS = PA::WROWS, PHT = PA::PHT, NT = PA::NT;
    constexpr int NTAB = (EPI ? 2 * NT : 0) + (BIAS ? NT : 0);

    static_assert(LDS_ONE % 4 == 0, "epilogue tables are read as float4");
    __shared__ __attribute__((aligned(16))) float lds[LDS_ONE + NTAB];
    float* lds_es = lds + LDS_ONE;  // epilogue scale / shift for this block's NT output channels
    float* lds_eh = lds_es + NT;
    float* lds_bias = lds + LDS_ONE + (EPI ? 2 * NT : 0);

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);  // 1-D grid: the cout blocks of one input tile on one XCD (wino_common.h)
    const int n0 = by_ * NT;
    const int tiles_x = p.W / PW;
    const int y0 = (bx_ / tiles_x) * PHT, x0 = (bx_ % tiles_x) * PW;
    const int HW = p.H * p.W;
    const int khalf = lane >> 5, j = lane & 31;
    const int ty = j / PW, tx = j % PW;
    const int x = x0 + tx;
    const int nA = p.Cin / KCA;
    const int nB = HASB ? p.Cin2 / 16 : 0;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* in2_b = HASB ? p.in2 + (size_t)b * p.in2_bs : nullptr;
    const float* sc = PRO ? p.pro_scale : nullptr;
    const float* sh = PRO ? p.pro_shift + (size_t)b * p.pro_shift_bs : nullptr;

    if (EPI && tid < NT) {
        lds_es[tid] = p.epi_scale[n0 + tid];
        lds_eh[tid] = p.epi_shift[(size_t)b * p.epi_shift_bs + n0 + tid];
    }
    if (BIAS && tid < NT) lds_bias[tid] = p.bias[n0 + tid];

    PA pa;
    PB pb;
    const auto rs = [](const float* ptr, long bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(ptr), 0, (int)bytes, 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t in_rs = rs(in_b, (long)p.Cin * HW * 4);
    const __amdgpu_buffer_rsrc_t wa_rs = rs(p.w + n0, ((long)p.Cin * TAPS * p.Nw - n0) * 4);
    const __amdgpu_buffer_rsrc_t in2_rs = HASB ? rs(in2_b, (long)p.Cin2 * HW * 4) : in_rs;
    const __amdgpu_buffer_rsrc_t wb_rs = HASB ? rs(p.w2 + n0, ((long)p.Cin2 * p.Nw - n0) * 4) : wa_rs;
    auto loadA = [&](int c) {
        pa.load(in_rs, (unsigned)(c * KCA * HW) * 4u, HW, wa_rs, (unsigned)(c * KCA * TAPS * p.Nw) * 4u, sc + c * KCA,
                sh + c * KCA);
    };
    auto loadB = [&](int c) {
        pb.load(in2_rs, (unsigned)(c * 16 * HW) * 4u, HW, wb_rs, (unsigned)(c * 16 * p.Nw) * 4u, nullptr, nullptr);
    };

    pa.init(tid, y0, x0, p.H, p.W);
    pa.init_w(tid, p.Nw);
    loadA(0);
    __syncthreads();  // tables visible
    pa.store(lds, tid);
    __syncthreads();

    f32x16 acc[NCO][NPX];
#pragma unroll
    for (int co = 0; co < NCO; ++co)
#pragma unroll
        for (int px = 0; px < NPX; ++px)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                acc[co][px][r] = BIAS ? lds_bias[co * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf] : 0.f;

    // ---- main phase, all chunks but the last
    for (int ch = 0; ch + 1 < nA; ++ch) {
        loadA(ch + 1);
        PA::compute(lds, acc, lane, wave);
        __syncthreads();
        pa.store(lds, tid);
        __syncthreads();
    }
    // ---- last chunk of the main phase: prefetch what the shortcut phase / the epilogue need
    float rtmp[RES_PF ? NPX : 1][16];
    if (HASB) {
        pb.init(tid, y0, x0, p.H, p.W);
        pb.init_w(tid, p.Nw);
        loadB(0);
    }
    if (RES_PF) {
#pragma unroll
        for (int px = 0; px < NPX; ++px) {
            const int y = min(y0 + wave * WROWS + px * PH + ty, p.H - 1);
            const float* src = p.res + (size_t)b * p.res_bs + (size_t)(n0 + 4 * khalf) * HW + (size_t)y * p.W + x;
#pragma unroll
            for (int r = 0; r < 16; ++r) rtmp[px][r] = src[(size_t)((r & 3) + 8 * (r >> 2)) * HW];
        }
    }
    PA::compute(lds, acc, lane, wave);
    // ---- shortcut phase (1x1 over the raw block input)
    if (HASB) {
        __syncthreads();
        pb.store(lds, tid);
        __syncthreads();
        for (int ch = 0; ch + 1 < nB; ++ch) {
            loadB(ch + 1);
            PB::compute(lds, acc, lane, wave);
            __syncthreads();
            pb.store(lds, tid);
            __syncthreads();
        }
        PB::compute(lds, acc, lane, wave);
    }
    // ---- epilogue
    if (FLAGS & F_TCONV)
        tconv_store<NCO, NPX, PW>(p, acc, b, n0, y0, x0, lane, wave);
    else
        store_tile<NCO, NPX, PW, FLAGS, RES_PF>(p, acc, rtmp, lds_es, lds_eh, b, n0, y0, x0, lane, wave);
}

template <int TAPS, int NCO, int NPX, int PW, int FLAGS>
hipError_t launch_one(const ConvArgs& p0, hipStream_t stream) {
    constexpr int PHT = 4 * NPX * (32 / PW);
    ConvArgs p = p0;
    // 1-D grid decoded by block_coords(): the gy cout blocks of a (tile, clip) pair run on ONE XCD - a transposed conv is a
    // 1-tap conv with 4 x Cout output channels, i.e. 2-12 cout blocks that all read the same input tile (in the natural
    // 3-D order they ran a whole grid row apart and the tile came from HBM once per block: 2x the input at decoder_block6)
    p.gx = (p.W / PW) * ((p.H + PHT - 1) / PHT);
    p.gy = p.N / (32 * NCO);
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    dim3 grid((unsigned)((long)p.gx * p.gy * p.B));
    // double-buffered kernel (one barrier per chunk) for the 64-wide 3x3 tiles with many chunks (16 and more of 8
    // channels), where it measured 1-9 % faster; the single-buffered kernel (higher occupancy) everywhere else
    constexpr bool HAS_DB = TAPS == 9 && NCO == 2 && PW == 32 && !(FLAGS & F_RES);  // geometries the db kernel exists for
    if constexpr (HAS_DB) {
        if (p.Cin / 8 >= 16) {
            hipLaunchKernelGGL((conv_kernel_db<TAPS, NCO, NPX, PW, FLAGS>), grid, dim3(NTHREADS), 0, stream, p);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((conv_kernel_sb<TAPS, NCO, NPX, PW, FLAGS>), grid, dim3(NTHREADS), 0, stream, p);
    return hipGetLastError();
}

// Tile geometry per layer shape.  Wave tile = NCO x NPX MFMA tiles of 32 couts x 32 pixels; block = 4 waves stacked
// over rows.  The bottom of the U-Net (W <= 16, 384 channels, a few thousand pixels per batch) needs small tiles to
// produce enough workgroups for 256 CUs.
template <int TAPS, int FLAGS>
hipError_t launch_geom(const ConvArgs& p, hipStream_t stream) {
    // measured (B=16): 3x3 at W=16 -> 32-cout x 32-px wave tiles in 8-row blocks; 3x3 at W=8 -> 32-cout tiles;
    // the 1-tap transposed convs keep the 64-cout tiles
    const int pw = p.W >= 32 ? 32 : p.W;
    if (pw == 32) {
        if (p.N % 64 == 0) return launch_one<TAPS, 2, 2, 32, FLAGS>(p, stream);
        return launch_one<TAPS, 1, 2, 32, FLAGS>(p, stream);
    }
    if (p.N % 64 != 0) return hipErrorInvalidValue;
    if constexpr (TAPS == 9) {
        if (pw == 16) return launch_one<TAPS, 1, 1, 16, FLAGS>(p, stream);
        if (pw == 8) return launch_one<TAPS, 1, 2, 8, FLAGS>(p, stream);
    } else {
        if (pw == 16) return launch_one<TAPS, 2, 2, 16, FLAGS>(p, stream);
        if (pw == 8) return launch_one<TAPS, 2, 2, 8, FLAGS>(p, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// Host-side shape validation shared by all conv launches: every assumption the kernel and its grid make.
static bool conv_args_ok(const ConvArgs& p, int taps, bool phaseb) {
    if (p.B <= 0 || p.H <= 0 || p.W <= 0) return false;
    if (p.W != 8 && p.W != 16 && (p.W % 32) != 0) return false;
    if (p.N % 32 != 0 || p.Nw < p.N || (p.Nw % 4) != 0) return false;
    const int kc = taps == 9 ? 8 : 16;
    if (p.Cin <= 0 || p.Cin % (2 * kc) != 0) return false;  // even chunk count (run_db)
    if (phaseb && (p.Cin2 <= 0 || p.Cin2 % 32 != 0)) return false;
    if (!p.in || !p.w || !p.out) return false;
    return true;
}

hipError_t lass_launch_conv(ConvKind kind, const ConvArgs& p, hipStream_t stream) {
    switch (kind) {
        case CONV1_ACT:  // 3x3, prologue act on x, epilogue act (conv2's BN+FiLM+leaky)
            if (!conv_args_ok(p, 9, false) || !p.pro_scale || !p.pro_shift || !p.epi_scale || !p.epi_shift)
                return hipErrorInvalidValue;
            return launch_geom<9, F_PRO | F_EPIACT>(p, stream);
        case CONV2_IDENT:  // 3x3 over pre-activated input, + residual
            if (!conv_args_ok(p, 9, false) || !p.res) return hipErrorInvalidValue;
            return launch_geom<9, F_RES>(p, stream);
        case CONV2_SHORTCUT:  // 3x3 over pre-activated input, + 1x1(in2) + bias
            if (!conv_args_ok(p, 9, true) || !p.in2 || !p.w2 || !p.bias) return hipErrorInvalidValue;
            return launch_geom<9, F_PHASEB | F_BIAS>(p, stream);
        case TCONV_ACT:  // kernel==stride transposed conv with prologue act
            if (!conv_args_ok(p, 1, false) || !p.pro_scale || !p.pro_shift || (p.up_h != 1 && p.up_h != 2))
                return hipErrorInvalidValue;
            return launch_geom<1, F_PRO | F_TCONV>(p, stream);
        default:  // the *_PRE kinds (pre_conv formed while staging) and the fused output head run on the Winograd and bf16 kernels
            return hipErrorInvalidValue;
    }
}
