// wino4.hip - Winograd F(4x4,3x3) 3x3 convolutions on the gfx950 f32 MFMA (the >= 32-channel layers at W >= 32, and split-K at
// the 32-frame x 16-bin level).
//
// Same reference semantics as wino.hip (models/resunet.py:101-119,147-165: 3x3 / stride 1 / pad 1 cross-correlation behind the
// BN+FiLM+leaky prologue, epilogue activation in front of conv2), one more step of the same algebra:
//      Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A      with 6x6 transforms (Lavin & Gray 2016, F(4x4,3x3))
// i.e. 36 independent GEMMs  M_xi[cout][tile] += U_xi[cout][cin] * V_xi[cin][tile]  per 4x4 output tile: 36 multiplies for 16
// outputs = 2.25 per output and (cin, cout) pair where F(2x2,3x3) needs 4 and the direct form 9 - 1.78x fewer MFMAs than
// wino.hip on an MFMA-bound path.  The price is conditioning (transform constants 4, 5, 8 and 1/24): ~6x the rounding error
// of F(2x2,3x3) per layer (2-5e-6 relative at K = 128..768), against a parity bar of 1e-4 RMS on waveforms.
//
// Mapping: v_mfma_f32_16x16x4_f32; a wave owns 16 couts x 16 tiles and keeps ALL 36 xi accumulators (144 registers), so the
// output transform is register-local.  Workgroup = 2 x 2 waves = 32 couts x 32 tiles (512 output pixels), two per CU.
// Per chunk of 8 input channels:
//   1. the weight slab U[36][8][32] arrives by LDS-DMA (36 KiB, the exact LDS image lass_finalize wrote);
//   2. every thread owns ONE (tile, channel) item: its 6x6 input patch comes straight from global memory (an aligned
//      16-byte load + two 4-byte loads per row, requested one chunk ahead), gets the BN+FiLM+leaky prologue and the zero
//      padding and is transformed in registers (144 add / fma), then written to V[36][4][32][2] in LDS;
//   3. 72 MFMAs per wave (36 xi x 2 k-steps), A and B fragments one ds_read_b64 each.
// Kinds: conv1 of a ConvBlockRes (prologue + epilogue activation), conv2 with the 1x1 shortcut (resunet.py:122-128,163),
// bias and the block's fused avg-pool (:197), and conv2 + a residual read from memory (+ the pool) for the wide layers whose
// shortcut runs as a GEMM of its own (pw_gemm.hip).  The shortcut is NOT taken through the transform domain: once the 36 xi are
// folded into this lane's 4 couts x 16 pixels, accumulator tile s = [16 couts][16 tiles] of sub-pixel s has exactly the MFMA
// D layout, so the 1x1 conv is 16 more MFMAs per 4 input channels with B operands straight from global memory (this lane's
// tile of channel 4 ks + kq: four 16-byte loads) and A = the shortcut weights - no transform, no LDS.
// decoder_block6's conv2 with the output head behind it has a kernel of its own, wino4_headfold_kernel: after_conv is composed into
// conv2's and the shortcut's weights (head_fold.h), so 3 logit rows are formed on one MFMA tile instead of 32 channels on two.
#include <hip/hip_runtime.h>
#include "head_fold.h"
#include "kernels.h"
#include "pixel_ops.h"
#include "wino4_transform.h"
#include "wino_common.h"

namespace {

constexpr int F_PRO = 1, F_PHASEB = 2, F_BIAS = 4, F_RES = 8, F_EPIACT = 16, F_PRECONV = 64, F_RESPRE = 128, F_MASK = 1024;  // as wino.hip
constexpr int F_SPLITK = 2048;  // this workgroup runs one share of the input channels and stores its partial sums (Wino4Split)
constexpr int F_SCLOGIT = 8192;  // encoder_block1.conv2 also writes the folded head's shortcut logits of the skip (HeadScPlanes)
constexpr int F_VPRE = 4096;    // the transformed input V is read from memory (Wino4VPre): wino4_vprep_kernel wrote it, once per layer
constexpr int NTHREADS = 256;
constexpr int KC = kWino4KC;
constexpr int NXI = kWino4NXI;
constexpr int U_F = NXI * 256;            // floats of one (8-channel chunk, 32-cout group) weight slab
constexpr int V_F = kWino4VFloats;        // [xi][kq][tile][k-step]

typedef float f32x2v __attribute__((ext_vector_type(2)));

// (bt6 / at6, the 1-D input and output transforms: wino4_transform.h, shared with wino4_gemm.hip)

// TC: tile columns of the block (32 tiles = (32 / TC) tile rows x TC tile columns; block = 4 * (32 / TC) rows x 4 * TC columns)
// A workgroup: 4 waves, 32 couts x 32 tiles; two workgroups per CU.
template <int TC, int FLAGS>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_kernel(ConvArgs p) {
    const Wino4Split sk;  // (unsplit)
    const Wino4VPre vp;   // (transforms its own input)
    const HeadScPlanes hs;
#include "wino4_body.h"
}
// ... and one share of the input channels, partial sums out (FLAGS0: F_PRO or nothing)
template <int TC, int FLAGS0>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_splitk_kernel(ConvArgs p, Wino4Split sk) {
    constexpr int FLAGS = FLAGS0 | F_SPLITK;
    const Wino4VPre vp;
    const HeadScPlanes hs;
#include "wino4_body.h"
}
// ... and both with the transformed input image V read from memory instead of formed here (FLAGS0: F_EPIACT, F_RES or F_SPLITK).
// The Cout / 32 workgroups of a 32-tile block all need the same V: formed in the kernel, each of them repeats the prologue, the
// padding and the 6x6 transform of its 32 tiles x 8 channels per chunk - 252 vector instructions per wave and chunk beside 72
// MFMAs on the datapath the two share.  Here the chunk loop is 9 + 9 LDS-DMA pieces per wave, a wait and the same MFMA phase.
template <int TC, int FLAGS0>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_vpre_kernel(ConvArgs p, Wino4Split sk, Wino4VPre vp) {
    constexpr int FLAGS = FLAGS0 | F_VPRE;
    const HeadScPlanes hs;
#include "wino4_body.h"
}
// ... and encoder_block1.conv2 of the head_sc_fold route (FLAGS0: F_RES | F_RESPRE): the unsplit kernel whose epilogue also forms
// the skip's share of the folded head's shortcut logits
template <int TC, int FLAGS0>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_sclogit_kernel(ConvArgs p, HeadScPlanes hs) {
    constexpr int FLAGS = FLAGS0 | F_SCLOGIT;
    const Wino4Split sk;
    const Wino4VPre vp;
#include "wino4_body.h"
}

// decoder_block6.conv2 with the output head, on weights composed with after_conv (head_fold.h): the 3 mask logits are one linear
// map of the conv input h and the shortcut input cat, so only 3 output rows are formed - padded to the 4 rows of the multi-block
// MFMA form (wino4_head_body.h) where wino4_kernel<.., F_MASK> forms 32 channels on two 16-row tiles and then reduces them 32 -> 3
// through 48 KiB of LDS.  Same workgroup (4 waves, 32 tiles, 8-channel chunks), same V image and input transform (wino4_input.h).
// A wave owns 9 of the 36 xi, for all tiles and both K-STEPS of a chunk: 36 MFMAs of 8 cycles per wave and chunk into 9
// accumulators (36 registers; 42 KiB of LDS: three workgroups per CU).  Behind the chunk loop the accumulators change hands once
// through LDS, every lane transforms one (k-step, logit, tile), and the shortcut's k-steps run half and half.  Each k-step ends
// with a partial logit set over its half of the channels; the two are summed through LDS in a fixed order (k-step 0 + k-step 1,
// then b'), so a clip's result depends on nothing but the clip.
// p: w_wino4 = the composed compact U images (kHeadFoldU4Floats per chunk), w2 = Wsc' [Cin2][16], bias = b' [16]; mask_w / mask_b unused.
template <int TC>
__global__ __launch_bounds__(NTHREADS, 3) void wino4_headfold_kernel(ConvArgs p) {
    constexpr bool PLANES = false;
    const HeadScPlanes hs;
#include "wino4_head_body.h"
}
// ... with the shortcut's logits read as planes (hs.skip + hs.up) that encoder_block1.conv2 and the transposed conv wrote: no shortcut
// phase, in2 / w2 are not read.  Final sum per pixel: (k-step 0 + k-step 1) + (skip + up) + b', in that order.
template <int TC>
__global__ __launch_bounds__(NTHREADS, 3) void wino4_headfold_planes_kernel(ConvArgs p, HeadScPlanes hs) {
    constexpr bool PLANES = true;
#include "wino4_head_body.h"
}

// The prep launch of those: one workgroup per (32-tile block, 8-channel chunk, clip), one (tile, channel) item per thread - the
// item mapping, loads, prologue, padding rule and transform of the conv kernels (wino4_input.h, the same text).  The 36-KiB image
// is staged in LDS exactly as the conv kernels lay it out (XOR swizzle included) and leaves as 16-byte rows, so the consumer's copy
// is linear: Vg[clip][block][chunk][36][256].  FLAGS: F_PRO or 0.
template <int TC, int FLAGS>
__global__ __launch_bounds__(NTHREADS) void wino4_vprep_kernel(ConvArgs p, Wino4VPre vp) {
    constexpr bool PRO = (FLAGS & F_PRO) != 0, PRE = false;
    static_assert((FLAGS & ~F_PRO) == 0, "a prologue at most");
    constexpr int TR = 32 / TC;
    constexpr int OR_ = 4 * TR, OC = 4 * TC;
    __shared__ __attribute__((aligned(16))) float lv[V_F];
    const int tid = threadIdx.x;
    const unsigned nchunk = (unsigned)(p.Cin / KC);
    const unsigned lin = blockIdx.x;  // chunk fastest: neighbouring workgroups write neighbouring slabs
    const int ch = (int)(lin % nchunk);
    const int bx_ = (int)(lin / nchunk % (unsigned)p.gx), b = (int)(lin / nchunk / (unsigned)p.gx);
    const int tiles_x = p.W / OC;
    const int y0 = (bx_ / tiles_x) * OR_, x0 = (bx_ % tiles_x) * OC;
    const int HW = p.H * p.W;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = PRO ? p.pro_scale : nullptr;
    const float* sh = PRO ? p.pro_shift + (size_t)b * p.pro_shift_bs : nullptr;
#include "wino4_input.h"
    pload(ch);
    pprocess();
    __syncthreads();
    float4* dst = reinterpret_cast<float4*>(vp.v + (((size_t)b * p.gx + bx_) * nchunk + ch) * V_F);
    const float4* src = reinterpret_cast<const float4*>(lv);
#pragma unroll
    for (int i = 0; i < V_F / 4 / NTHREADS; ++i) dst[i * NTHREADS + tid] = src[i * NTHREADS + tid];
}

// Combine of a split launch: out = epilogue(sum over the splits, in split order, of the partials wino4_splitk_kernel left in
// sk.part) - the same epilogue terms as the unsplit kernel: bn2 + FiLM + leaky (conv1), or the residual and the block's
// avg-pool, 2 x 2 or 1 x 2 (conv2).  A thread owns 2 rows x 4 columns of one channel; H is even and W a multiple of 4.
template <int FLAGS>
__global__ __launch_bounds__(256) void wino4_combine_kernel(ConvArgs p, Wino4Split sk) {
    constexpr bool EPI = (FLAGS & F_EPIACT) != 0, RES = (FLAGS & F_RES) != 0;
    static_assert(EPI != RES && (FLAGS & ~(F_EPIACT | F_RES)) == 0, "conv1 or the identity conv2");
    const int W4 = p.W / 4, H2 = p.H / 2, HW = p.H * p.W;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)p.B * p.N * H2 * W4) return;
    const int xq = (int)(idx % W4), yh = (int)(idx / W4 % H2), n = (int)(idx / ((long)W4 * H2) % p.N), b = (int)(idx / ((long)W4 * H2 * p.N));
    const size_t pix = (size_t)(2 * yh) * p.W + 4 * xq;
    const size_t split_pitch = (size_t)p.B * p.N * HW;
    const float* pp = sk.part + ((size_t)b * p.N + n) * HW + pix;
    float4 v[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] = *reinterpret_cast<const float4*>(pp + (size_t)i * p.W);
    for (int s = 1; s < sk.n; ++s)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float4 t = *reinterpret_cast<const float4*>(pp + (size_t)s * split_pitch + (size_t)i * p.W);
            v[i].x += t.x; v[i].y += t.y; v[i].z += t.z; v[i].w += t.w;
        }
    if (EPI) {  // bn2 + FiLM + leaky (resunet.py:151)
        const float es = p.epi_scale[n], eh = p.epi_shift[(size_t)b * p.epi_shift_bs + n];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            v[i].x = leaky(fmaf(v[i].x, es, eh)); v[i].y = leaky(fmaf(v[i].y, es, eh));
            v[i].z = leaky(fmaf(v[i].z, es, eh)); v[i].w = leaky(fmaf(v[i].w, es, eh));
        }
    }
    if (RES) {  // (may be `out` itself: every element is read and then written by this thread)
        const float* rr = p.res + (size_t)b * p.res_bs + (size_t)n * HW + pix;
        float4 t[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) t[i] = *reinterpret_cast<const float4*>(rr + (size_t)i * p.W);
#pragma unroll
        for (int i = 0; i < 2; ++i) { v[i].x += t[i].x; v[i].y += t[i].y; v[i].z += t[i].z; v[i].w += t[i].w; }
    }
    float* dst = p.out + (size_t)b * p.out_bs + (size_t)n * HW + pix;
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<float4*>(dst + (size_t)i * p.W) = v[i];
    if (RES && p.pool_out) {
        const int Wo = p.W / 2, Ho = p.H / p.pool_h;
        float* pd = p.pool_out + (size_t)b * (p.pool_bs ? (size_t)p.pool_bs : (size_t)p.N * Ho * Wo) + (size_t)n * Ho * Wo + 2 * xq;
        if (p.pool_h == 2) {  // row-major summation order of F.avg_pool2d
            float s0 = v[0].x + v[0].y, s1 = v[0].z + v[0].w;
            s0 += v[1].x; s0 += v[1].y;
            s1 += v[1].z; s1 += v[1].w;
            *reinterpret_cast<float2*>(pd + (size_t)yh * Wo) = make_float2(s0 * 0.25f, s1 * 0.25f);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                *reinterpret_cast<float2*>(pd + (size_t)(2 * yh + i) * Wo) = make_float2((v[i].x + v[i].y) * 0.5f, (v[i].z + v[i].w) * 0.5f);
        }
    }
}

// Transform-domain weights U = G g G^T (6x6) of g = w[cout][cin][3][3], stored as the LDS images the kernel DMAs: slab
// (chunk = cin / 8, group = cout / 32) of 36 * 256 floats, element [xi][t = (cout % 32) / 16][kq = cin % 4][l15 = cout % 16]
// [k = (cin % 8) / 4].
__global__ __launch_bounds__(256) void wino4_weights_kernel(const float* __restrict__ w, int Cout, int Cin, float* __restrict__ U) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (cin, cout), cout fastest
    if (i >= (long)Cout * Cin) return;
    const int co = (int)(i % Cout), ci = (int)(i / Cout);
    const float* g = w + ((size_t)co * Cin + ci) * 9;
    const double G[6][3] = {{0.25, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
    double t[6][3];
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 3; ++c) t[a][c] = G[a][0] * (double)g[0 * 3 + c] + G[a][1] * (double)g[1 * 3 + c] + G[a][2] * (double)g[2 * 3 + c];
    float* slab = U + ((size_t)(ci / 8) * (Cout / 32) + co / 32) * U_F;
    const int e = (((co & 31) >> 4) * 4 + (ci & 3)) * 32 + (co & 15) * 2 + ((ci & 7) >> 2);
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            const double u = t[a][0] * G[c][0] + t[a][1] * G[c][1] + t[a][2] * G[c][2];
            slab[(a * 6 + c) * 256 + e] = (float)u;
        }
}

template <int TC, int FLAGS>
hipError_t launch_wino4_tc(const ConvArgs& p0, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    p.gx = (p.W / OC) * ((p.H + OR_ - 1) / OR_);
    p.gy = p.N / 32;
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((wino4_kernel<TC, FLAGS>), dim3((unsigned)((long)p.gx * p.gy * p.B)), dim3(NTHREADS), 0, stream, p);
    return hipGetLastError();
}

template <int FLAGS>
hipError_t launch_wino4(const ConvArgs& p, hipStream_t stream) {
    const int tc = lass_wino4_block_tc(p.H, p.W);
    if (tc == 16) return launch_wino4_tc<16, FLAGS>(p, stream);  // 8 rows x 64 columns
    if (tc == 8) return launch_wino4_tc<8, FLAGS>(p, stream);    // 16 rows x 32 columns
    // 32 rows x 16 columns (lass_wino4_narrow): CONV1_ACT and CONV2_IDENT only (lass_wino4_supported)
    if constexpr (FLAGS == (F_PRO | F_EPIACT) || FLAGS == F_RES)
        if (tc == 4) return launch_wino4_tc<4, FLAGS>(p, stream);
    return hipErrorInvalidValue;
}

template <int TC>
hipError_t launch_wino4_headfold_tc(const ConvArgs& p0, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    p.gx = (p.W / OC) * (p.H / OR_);
    p.gy = 1;
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((wino4_headfold_kernel<TC>), dim3((unsigned)((long)p.gx * p.B)), dim3(NTHREADS), 0, stream, p);
    return hipGetLastError();
}

template <int TC>
hipError_t launch_wino4_headfold_planes_tc(const ConvArgs& p0, const HeadScPlanes& hs, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    p.gx = (p.W / OC) * (p.H / OR_);
    p.gy = 1;
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((wino4_headfold_planes_kernel<TC>), dim3((unsigned)((long)p.gx * p.B)), dim3(NTHREADS), 0, stream, p, hs);
    return hipGetLastError();
}

template <int TC>
hipError_t launch_wino4_sclogit_tc(const ConvArgs& p0, const HeadScPlanes& hs, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    p.gx = (p.W / OC) * (p.H / OR_);
    p.gy = p.N / 32;  // (1: all 32 channels of a pixel in one workgroup)
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    hipLaunchKernelGGL((wino4_sclogit_kernel<TC, F_RES | F_RESPRE>), dim3((unsigned)((long)p.gx * p.gy * p.B)), dim3(NTHREADS), 0, stream, p, hs);
    return hipGetLastError();
}

// V from memory: the prep launch (PRO: conv1's prologue), then the conv kernel of the same block geometry.  MAIN: F_EPIACT (conv1),
// F_RES (identity conv2) or F_SPLITK; a split launch is followed by its combine (COMB), as in launch_wino4_split.
template <int TC, int MAIN, int COMB>
hipError_t launch_wino4_vpre_tc(const ConvArgs& p0, const Wino4Split& sk, const Wino4VPre& vp, bool pro, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    constexpr bool SPLIT = (MAIN & F_SPLITK) != 0;
    const int n = SPLIT ? sk.n : 1;
    p.gx = (p.W / OC) * (p.H / OR_);
    p.gy = p.N / 32;
    p.xcd_map = ((long)p.gx * p.B * n) % 8 == 0;
    const dim3 pgrid((unsigned)((long)p.gx * (p.Cin / KC) * p.B));
    if (pro)
        hipLaunchKernelGGL((wino4_vprep_kernel<TC, F_PRO>), pgrid, dim3(NTHREADS), 0, stream, p, vp);
    else
        hipLaunchKernelGGL((wino4_vprep_kernel<TC, 0>), pgrid, dim3(NTHREADS), 0, stream, p, vp);
    if (hipError_t e = hipGetLastError()) return e;
    Wino4Split s1 = sk;
    if (!SPLIT) s1 = Wino4Split();
    hipLaunchKernelGGL((wino4_vpre_kernel<TC, MAIN>), dim3((unsigned)((long)p.gx * p.gy * p.B * n)), dim3(NTHREADS), 0, stream, p, s1, vp);
    if (hipError_t e = hipGetLastError()) return e;
    if constexpr (SPLIT) {
        const long items = (long)p.B * p.N * (p.H / 2) * (p.W / 4);
        hipLaunchKernelGGL((wino4_combine_kernel<COMB>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, p, sk);
        return hipGetLastError();
    }
    return hipSuccess;
}

// EPI: F_EPIACT (conv1, prologue in the prep launch) or F_RES (identity conv2, none)
template <int EPI>
hipError_t launch_wino4_vpre(const ConvArgs& p, const Wino4Split& sk, const Wino4VPre& vp, hipStream_t stream) {
    constexpr bool pro = EPI == F_EPIACT;
    const int tc = lass_wino4_block_tc(p.H, p.W);
    if (tc == 16) return launch_wino4_vpre_tc<16, EPI, 0>(p, sk, vp, pro, stream);
    if (tc == 8) return launch_wino4_vpre_tc<8, EPI, 0>(p, sk, vp, pro, stream);
    if (tc == 4)
        return sk.n > 1 ? launch_wino4_vpre_tc<4, F_SPLITK, EPI>(p, sk, vp, pro, stream) : launch_wino4_vpre_tc<4, EPI, 0>(p, sk, vp, pro, stream);
    return hipErrorInvalidValue;
}

// Split-K on the 32 x 16 blocks: a whole clip plane is ONE block there, so a launch has only B * N / 32 workgroups for the 512
// slots of the GPU; with the chunks dealt to sk.n workgroups each it has sk.n times as many.  MAIN: the partial-sum kernel
// (prologue or none), COMB: the epilogue of the combine.
template <int MAIN, int COMB>
hipError_t launch_wino4_split(const ConvArgs& p0, const Wino4Split& sk, hipStream_t stream) {
    ConvArgs p = p0;
    p.gx = (p.W / 16) * (p.H / 32);
    p.gy = p.N / 32;
    p.xcd_map = ((long)p.gx * p.B * sk.n) % 8 == 0;
    hipLaunchKernelGGL((wino4_splitk_kernel<4, MAIN>), dim3((unsigned)((long)p.gx * p.gy * p.B * sk.n)), dim3(NTHREADS), 0, stream, p, sk);
    if (hipError_t e = hipGetLastError()) return e;
    const long items = (long)p.B * p.N * (p.H / 2) * (p.W / 4);
    hipLaunchKernelGGL((wino4_combine_kernel<COMB>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, p, sk);
    return hipGetLastError();
}

}  // namespace

// lass_wino4_shape (conv_route.h) && the pointers of the kind are there
bool lass_wino4_supported(ConvKind kind, const ConvArgs& p, const Wino4Split& sk) {
    if (!lass_wino4_shape(kind, lass_conv_shape(p), sk.n) || !p.w_wino4 || (sk.n != 1 && !sk.part)) return false;
    switch (kind) {
        case CONV1_ACT:
            return true;
        case CONV1_ACT_PRE:
            return p.pre_w && p.pre_b;
        case CONV2_IDENT_PRE:
            return p.res && p.pre_w && p.pre_b;
        case CONV2_IDENT:  // (res may be `out` itself)
            return p.res != nullptr;
        case CONV2_SHORTCUT:
            if (!(p.in2 && p.w2 && p.bias)) return false;
            return !p.mask_re || (p.W + 1 == p.mask_nbins && p.mask_w && p.mask_b && p.mask_mag && p.mask_cos && p.mask_sin && p.mask_im &&
                                  p.mask_T > 0 && p.mask_T <= p.H);
        default:
            return false;
    }
}

bool lass_wino4_vpre_supported(ConvKind kind, const ConvArgs& p, const Wino4Split& sk) {
    return lass_wino4_vpre_shape(kind, lass_conv_shape(p), sk.n) && lass_wino4_supported(kind, p, sk);
}

hipError_t lass_launch_wino4(ConvKind kind, const ConvArgs& p, hipStream_t stream, const Wino4Split& sk, const Wino4VPre& vp) {
    if (!lass_wino4_supported(kind, p, sk) || !p.in || (!p.out && !p.mask_re)) return hipErrorInvalidValue;
    if (vp.v) {
        if (!lass_wino4_vpre_supported(kind, p, sk)) return hipErrorInvalidValue;
        if (kind == CONV1_ACT) {
            if (!p.pro_scale || !p.pro_shift || !p.epi_scale || !p.epi_shift) return hipErrorInvalidValue;
            return launch_wino4_vpre<F_EPIACT>(p, sk, vp, stream);
        }
        return launch_wino4_vpre<F_RES>(p, sk, vp, stream);
    }
    switch (kind) {
        case CONV1_ACT:
        case CONV1_ACT_PRE:
            if (!p.pro_scale || !p.pro_shift || !p.epi_scale || !p.epi_shift) return hipErrorInvalidValue;
            if (sk.n > 1) return launch_wino4_split<F_PRO, F_EPIACT>(p, sk, stream);
            return kind == CONV1_ACT ? launch_wino4<F_PRO | F_EPIACT>(p, stream) : launch_wino4<F_PRO | F_EPIACT | F_PRECONV>(p, stream);
        case CONV2_IDENT:
            if (sk.n > 1) return launch_wino4_split<0, F_RES>(p, sk, stream);
            return launch_wino4<F_RES>(p, stream);
        case CONV2_IDENT_PRE:
            return launch_wino4<F_RES | F_RESPRE>(p, stream);
        case CONV2_SHORTCUT:
            return p.mask_re ? launch_wino4<F_PHASEB | F_BIAS | F_MASK>(p, stream) : launch_wino4<F_PHASEB | F_BIAS>(p, stream);
        default:
            return hipErrorInvalidValue;
    }
}

// lass_wino4_headfold_shape (conv_route.h) && the pointers of the folded head are there: the composed images in w_wino4 / w2 / bias
bool lass_wino4_headfold_supported(const ConvArgs& p) {
    return lass_wino4_headfold_shape(lass_conv_shape(p)) && p.in && p.w_wino4 && p.in2 && p.w2 && p.bias && p.W + 1 == p.mask_nbins &&
           p.mask_mag && p.mask_cos && p.mask_sin && p.mask_re && p.mask_im && p.mask_T > 0 && p.mask_T <= p.H;
}

hipError_t lass_launch_wino4_headfold(const ConvArgs& p, hipStream_t stream) {
    if (!lass_wino4_headfold_supported(p)) return hipErrorInvalidValue;
    return launch_wino4_headfold_tc<16>(p, stream);  // (the shape rule admits the 8 x 64 blocks only)
}

bool lass_wino4_headfold_planes_supported(const ConvArgs& p, const HeadScPlanes& hs) {
    return lass_wino4_headfold_supported(p) && hs.skip && hs.up;
}

hipError_t lass_launch_wino4_headfold_planes(const ConvArgs& p, const HeadScPlanes& hs, hipStream_t stream) {
    if (!lass_wino4_headfold_planes_supported(p, hs)) return hipErrorInvalidValue;
    return launch_wino4_headfold_planes_tc<16>(p, hs, stream);
}

// encoder_block1.conv2 on the 8 x 64 blocks, one cout group (the 32 channels of a pixel meet in one workgroup's LDS)
bool lass_wino4_sclogit_supported(const ConvArgs& p, const HeadScPlanes& hs) {
    return lass_wino4_supported(CONV2_IDENT_PRE, p) && lass_wino4_block_tc(p.H, p.W) == 16 && p.in && p.out && hs.skip && hs.w;
}

hipError_t lass_launch_wino4_sclogit(const ConvArgs& p, const HeadScPlanes& hs, hipStream_t stream) {
    if (!lass_wino4_sclogit_supported(p, hs)) return hipErrorInvalidValue;
    return launch_wino4_sclogit_tc<16>(p, hs, stream);
}

hipError_t lass_launch_wino4_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream) {
    const long n = (long)Cout * Cin;
    hipLaunchKernelGGL(wino4_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, Cout, Cin, U);
    return hipGetLastError();
}
