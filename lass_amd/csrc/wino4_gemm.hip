// wino4_gemm.hip - Winograd F(4x4,3x3) in "scatter - batched GEMM - gather" form for the f32 convs with 384 output channels whose
// transformed input V comes from memory (conv_route.h: ConvRoute::gemm; both convs of encoder_block5-6 and decoder_block1-2).
//
// wino4.hip's conv kernel is, for these layers, 36 independent contractions M_xi[cout][tile] = sum_cin U_xi[cout][cin] V_xi[cin][tile]
// and an output transform.  It runs them on v_mfma_f32_16x16x4_f32 with a 16-couts x 16-tiles wave tile, because a wave keeps all
// 36 xi accumulators for the register-local output transform: both operands are re-read from LDS for every 16 MACs per element and
// the launch is bound by the f32 MFMA rate.  Here the 36 contractions are real GEMMs with pw_gemm.hip's split-bf16 body (text:
// pw_gemm_split_body.h) - a 128 x 128 workgroup tile, v_mfma_f32_32x32x16_bf16 over three exact bf16 pieces per operand, six piece
// products in one fixed order, f32 accuracy - at the price of M going through memory (2.25 x the output, written once, read once).
//   1. wino4_scatter_kernel: wino4_vprep_kernel with another store.  The same text forms V (wino4_input.h: loads, prologue, padding
//      rule, bt6 order), so its values are bit for bit those of the prep launch; the image leaves as V[xi][cin][p], p contiguous,
//      p = (clip * blocks + block) * 32 + tile-in-block over ALL clips of the launch.  lass_wino4_vpre_floats() floats, no padding.
//   2. wino4_gemm_kernel: xi is the body's batch index; X_xi = V[xi] (K = Cin rows of P columns, split where it is staged),
//      W_xi = the per-layer image [xi][3 pieces][Cin / 8][N][8] bf16 that lass_launch_wino4_gemm_weights split from exactly the f32
//      U of wino4_weights_kernel, M[xi][n][p] f32 out.  A 128-column tile may span clips; the last one may be partial (the body's
//      clamp).  A column's sum over K runs in one order whatever tile or batch it sits in: a clip's bits depend on the clip alone.
//   3. wino4_gather_kernel: one thread per (cout, p).  36 loads coalesced over tiles, at6 twice exactly as wino4_body.h orders it,
//      then the epilogue terms of wino4_combine_kernel - bn2 + FiLM + leaky (conv1), or the residual (possibly in place) and the
//      block's 2 x 2 or 1 x 2 avg-pool in F.avg_pool2d's summation order (conv2) - and 16-byte row stores.
// No atomics, no arrival order, no split-K: 36 xi x N / 128 x P / 128 workgroups fill the device at every level that takes the route.
#include <hip/hip_runtime.h>
#include "pw_gemm_split.h"
#include "wino4_transform.h"

namespace {

constexpr int F_PRO = 1, F_RES = 8, F_EPIACT = 16;  // as wino4.hip
constexpr int NXI = kWino4NXI;
constexpr int U_F = NXI * 256;      // floats of one (8-channel chunk, 32-cout group) slab of wino4.hip's weight image
constexpr int V_F = kWino4VFloats;  // floats of one (block, chunk) of V as wino4_input.h lays it out in LDS

// Tiles of the whole launch: the GEMMs' column count
__host__ __device__ inline unsigned tiles_of(const ConvArgs& p) { return (unsigned)p.B * (unsigned)p.gx * 32u; }

// One workgroup per (32-tile block, 8-channel chunk, clip), one (tile, channel) item per thread, exactly as wino4_vprep_kernel; the
// LDS image (wino4_input.h's layout, XOR swizzle included) leaves as 36 x 8 runs of 32 tiles (128 B each).  FLAGS: F_PRO or 0.
template <int TC, int FLAGS>
__global__ __launch_bounds__(NTHREADS) void wino4_scatter_kernel(ConvArgs p, Wino4VPre vp) {
    constexpr bool PRO = (FLAGS & F_PRO) != 0, PRE = false;
    static_assert((FLAGS & ~F_PRO) == 0, "a prologue at most");
    constexpr int KC = kWino4KC;  // (the input text's chunk: 8 channels, not the GEMM's 16 k rows)
    constexpr int TR = 32 / TC;
    constexpr int OR_ = 4 * TR, OC = 4 * TC;
    __shared__ __attribute__((aligned(16))) float lv[V_F];
    const int tid = threadIdx.x;
    const unsigned nchunk = (unsigned)(p.Cin / KC);
    const unsigned lin = blockIdx.x;  // chunk fastest, as in the prep launch
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
    const size_t Pt = tiles_of(p);
    float* dst = vp.v + (size_t)(ch * KC) * Pt + ((size_t)b * p.gx + bx_) * 32;
#pragma unroll
    for (int it = 0; it < NXI * KC * 8 / NTHREADS; ++it) {
        const int i = it * NTHREADS + tid;
        const int q = i & 7, c = (i >> 3) & 7, xi = i >> 6;  // four tiles 4 q .. 4 q + 3 of row (xi, channel c)
        const float* src = lv + xi * 256 + ((c & 3) * 32 + ((4 * q) ^ ((c & 1) << 4))) * 2 + (c >> 2);
        const float4 o = make_float4(src[0], src[2], src[4], src[6]);
        *reinterpret_cast<float4*>(dst + ((size_t)xi * p.Cin + c) * Pt + 4 * q) = o;
    }
}

// The 36 GEMMs: the body of pw_gemm_split_kernel with xi as its batch index.  p: in2 = V (batch stride Cin * P), Cin2 = Cin,
// N = Nw = couts, H * W = P, out = M (batch stride N * P), B = 36.
// ACC2, the 32 x 16 blocks: the f32 route they are held to sums K there in four parts of 24 MFMA steps (split-K), which makes it
// 1.8 x as accurate as its own unsplit form; six roundings of one accumulator per 16 k rows (144 at K = 384) measured 1.65 x that
// route's RMS error and 2.1 x its largest deviation.  With the small products apart the large sum is rounded 24 times.  A rule of
// the block geometry, never of B.
template <bool ACC2>
__global__ __launch_bounds__(NTHREADS, 2) void wino4_gemm_kernel(ConvArgs p, PwSplitW sw) {
    constexpr bool TCONV = false, XI = true;
#include "pw_gemm_split_body.h"
}

// FLAGS: F_EPIACT (conv1) or F_RES (the identity conv2).  p as the conv launch has it (gx set); m = M[36][N][P].
template <int TC, int FLAGS>
__global__ __launch_bounds__(256) void wino4_gather_kernel(ConvArgs p, const float* __restrict__ m) {
    constexpr bool EPI = (FLAGS & F_EPIACT) != 0, RES = (FLAGS & F_RES) != 0;
    static_assert(EPI != RES && (FLAGS & ~(F_EPIACT | F_RES)) == 0, "conv1 or the identity conv2");
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    const size_t Pt = tiles_of(p);
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)p.N * Pt) return;
    const unsigned pp = (unsigned)(idx % Pt);
    const int n = (int)(idx / Pt);
    const int pt = (int)(pp & 31u);
    const unsigned blk = pp >> 5;
    const int bx_ = (int)(blk % (unsigned)p.gx), b = (int)(blk / (unsigned)p.gx);
    const int tiles_x = p.W / OC;
    const int oy = (bx_ / tiles_x) * OR_ + 4 * (pt / TC), ox = (bx_ % tiles_x) * OC + 4 * (pt % TC);
    const int HW = p.H * p.W;
    float acc[NXI];
    const float* mp = m + (size_t)n * Pt + pp;
#pragma unroll
    for (int xi = 0; xi < NXI; ++xi) acc[xi] = mp[(size_t)xi * p.N * Pt];
    // Y = A^T M A in wino4_body.h's order: at6 down the six rows of every column, then along the rows
    float tmp[4][6];
#pragma unroll
    for (int jx = 0; jx < 6; ++jx) {
        const float mm[6] = {acc[0 + jx], acc[6 + jx], acc[12 + jx], acc[18 + jx], acc[24 + jx], acc[30 + jx]};
        float y[4];
        at6(mm, y);
#pragma unroll
        for (int a = 0; a < 4; ++a) tmp[a][jx] = y[a];
    }
    float ys[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) at6(tmp[a], ys[a]);
    if (EPI) {  // bn2 + FiLM + leaky (resunet.py:151)
        const float es = p.epi_scale[n], eh = p.epi_shift[(size_t)b * p.epi_shift_bs + n];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) ys[a][c] = leaky(fmaf(ys[a][c], es, eh));
    }
    const size_t pix = (size_t)n * HW + (size_t)oy * p.W + ox;
    if (RES) {  // (may be `out` itself: all 16 elements are read here and then written by this thread)
        const float* rr = p.res + (size_t)b * p.res_bs + pix;
        float4 t[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) t[a] = *reinterpret_cast<const float4*>(rr + (size_t)a * p.W);
#pragma unroll
        for (int a = 0; a < 4; ++a) { ys[a][0] += t[a].x; ys[a][1] += t[a].y; ys[a][2] += t[a].z; ys[a][3] += t[a].w; }
    }
    float* dst = p.out + (size_t)b * p.out_bs + pix;
#pragma unroll
    for (int a = 0; a < 4; ++a) *reinterpret_cast<float4*>(dst + (size_t)a * p.W) = make_float4(ys[a][0], ys[a][1], ys[a][2], ys[a][3]);
    if (RES && p.pool_out) {
        const int Wo = p.W / 2, Ho = p.H / p.pool_h;
        float* pd = p.pool_out + (size_t)b * (p.pool_bs ? (size_t)p.pool_bs : (size_t)p.N * Ho * Wo) + (size_t)n * Ho * Wo + (ox >> 1);
        if (p.pool_h == 2) {  // row-major summation order of F.avg_pool2d
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float s0 = ys[2 * i][0] + ys[2 * i][1], s1 = ys[2 * i][2] + ys[2 * i][3];
                s0 += ys[2 * i + 1][0]; s0 += ys[2 * i + 1][1];
                s1 += ys[2 * i + 1][2]; s1 += ys[2 * i + 1][3];
                *reinterpret_cast<float2*>(pd + (size_t)((oy >> 1) + i) * Wo) = make_float2(s0 * 0.25f, s1 * 0.25f);
            }
        } else {
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float2*>(pd + (size_t)(oy + a) * Wo) = make_float2((ys[a][0] + ys[a][1]) * 0.5f, (ys[a][2] + ys[a][3]) * 0.5f);
        }
    }
}

// U = wino4.hip's weight image (the f32 values both routes contract: G g G^T in double, rounded once) -> dst [xi][3 pieces h, m, l]
// [Cin / 8][Cout][8] bf16.  One thread per (xi, k octet, cout).
__global__ __launch_bounds__(256) void wino4_gemm_weights_kernel(const float* __restrict__ U, int Cout, int Cin, bf16x8* __restrict__ dst) {
    const size_t plane = (size_t)(Cin / 8) * Cout, u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= plane * NXI) return;
    const int xi = (int)(u / plane);
    const size_t r = u - (size_t)xi * plane;
    const int o = (int)(r / Cout), co = (int)(r - (size_t)o * Cout);
    const float* slab = U + ((size_t)o * (Cout / 32) + co / 32) * U_F + xi * 256;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = slab[(((co & 31) >> 4) * 4 + (j & 3)) * 32 + (co & 15) * 2 + (j >> 2)];
    bf16x8 h, mm, l;
    split3(x, h, mm, l);
    bf16x8* d = dst + (size_t)xi * 3 * plane + r;
    d[0] = h;
    d[plane] = mm;
    d[2 * plane] = l;
}

template <int TC, int EPI>
hipError_t launch_tc(const ConvArgs& p0, const Wino4VPre& vp, const Wino4Gemm& g, hipStream_t stream) {
    ConvArgs p = p0;
    constexpr int OR_ = 4 * (32 / TC), OC = 4 * TC;
    p.gx = (p.W / OC) * (p.H / OR_);
    p.gy = p.N / 32;
    const unsigned Pt = tiles_of(p);
    const dim3 sgrid((unsigned)((long)p.gx * (p.Cin / kWino4KC) * p.B));
    if (EPI == F_EPIACT)
        hipLaunchKernelGGL((wino4_scatter_kernel<TC, F_PRO>), sgrid, dim3(NTHREADS), 0, stream, p, vp);
    else
        hipLaunchKernelGGL((wino4_scatter_kernel<TC, 0>), sgrid, dim3(NTHREADS), 0, stream, p, vp);
    if (hipError_t e = hipGetLastError()) return e;
    ConvArgs q;  // the GEMMs as the body reads them
    q.in2 = vp.v; q.in2_bs = (long)p.Cin * Pt; q.Cin2 = p.Cin;
    q.N = q.Nw = p.N; q.H = 1; q.W = (int)Pt; q.B = NXI;
    q.out = g.m; q.out_bs = (long)p.N * Pt;
    q.gx = (int)((Pt + PB - 1) / PB);
    q.gy = p.N / NB;
    q.xcd_map = ((long)q.gx * q.B) % 8 == 0;  // the N / 128 cout tiles that share an X tile run on one XCD
    PwSplitW sw;
    sw.w = g.w3;
    hipLaunchKernelGGL(wino4_gemm_kernel<TC == 4>, dim3((unsigned)((long)q.gx * q.gy * q.B)), dim3(NTHREADS), 0, stream, q, sw);
    if (hipError_t e = hipGetLastError()) return e;
    const size_t items = (size_t)p.N * Pt;
    hipLaunchKernelGGL((wino4_gather_kernel<TC, EPI>), dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, p, (const float*)g.m);
    return hipGetLastError();
}

template <int EPI>
hipError_t launch_geom(const ConvArgs& p, const Wino4VPre& vp, const Wino4Gemm& g, hipStream_t stream) {
    const int tc = lass_wino4_block_tc(p.H, p.W);
    if (tc == 16) return launch_tc<16, EPI>(p, vp, g, stream);
    if (tc == 8) return launch_tc<8, EPI>(p, vp, g, stream);
    if (tc == 4) return launch_tc<4, EPI>(p, vp, g, stream);
    return hipErrorInvalidValue;
}

}  // namespace

// lass_wino4_gemm_shape (conv_route.h) && the pointers of the kind, the images and both workspaces are there; the tiles of the
// launch and the thread count of the gather fit their 32-bit indices
bool lass_wino4_gemm_supported(ConvKind kind, const ConvArgs& p, const Wino4VPre& vp, const Wino4Gemm& g) {
    if (!lass_wino4_gemm_shape(kind, lass_conv_shape(p)) || p.B <= 0 || !p.in || !p.out || !vp.v || !g.m || !g.w3 || ((uintptr_t)g.w3 & 15u) ||
        ((uintptr_t)vp.v & 15u) || ((uintptr_t)g.m & 15u))
        return false;
    const unsigned long long Pt = (unsigned long long)p.B * (unsigned long long)(p.H * p.W / 16);
    if (Pt >= 0x7FFFFFFFull || Pt * (unsigned long long)p.N / 256ull >= 0x7FFFFFFFull) return false;
    if (kind == CONV1_ACT) return p.pro_scale && p.pro_shift && p.epi_scale && p.epi_shift;
    return kind == CONV2_IDENT && p.res && (!p.pool_out || p.pool_h == 1 || p.pool_h == 2);
}

hipError_t lass_launch_wino4_gemm(ConvKind kind, const ConvArgs& p, const Wino4VPre& vp, const Wino4Gemm& g, hipStream_t stream) {
    if (!lass_wino4_gemm_supported(kind, p, vp, g)) return hipErrorInvalidValue;
    return kind == CONV1_ACT ? launch_geom<F_EPIACT>(p, vp, g, stream) : launch_geom<F_RES>(p, vp, g, stream);
}

hipError_t lass_launch_wino4_gemm_weights(const float* U, int Cout, int Cin, void* dst, hipStream_t stream) {
    if (!U || !dst || Cin <= 0 || Cin % 8 != 0 || Cout <= 0 || Cout % 32 != 0 || ((uintptr_t)dst & 15u)) return hipErrorInvalidValue;
    const size_t units = (size_t)(Cin / 8) * Cout * NXI;
    hipLaunchKernelGGL(wino4_gemm_weights_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, U, Cout, Cin,
                       reinterpret_cast<bf16x8*>(dst));
    return hipGetLastError();
}
