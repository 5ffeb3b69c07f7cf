// pw_gemm.hip - the f32 pointwise GEMMs of the ResUNet on the gfx950 f32 MFMA: D[n][p] = sum_k W[k][n] * X[k][p] over planar
// NCHW f32 (channel stride H*W, batch strides), with a wide cout tile so that X is fetched Cout/128 times per layer instead of
// Cout/32 times (the 32-cout workgroups of wino4.hip's fused shortcut phase).  Two epilogues:
//   CONV2_SHORTCUT: out[b][n][p] = bias[n] + sum_k Wsc[k][n] x[b][k][p]  (resunet.py:122-128,163: the 1x1 shortcut of a
//                   ConvBlockRes over the raw block input).  Written into the block's output slot, where conv2 (wino4.hip,
//                   CONV2_IDENT) then reads it as its residual and overwrites it in place.
//   TCONV_ACT:      kernel == stride ConvTranspose2d (resunet.py:223-262) behind the BN+FiLM+leaky prologue, which is applied
//                   once per staged element; n = (co, a, bb) scattered to (y * up_h + a, x * 2 + bb) as tconv_store does.
// Mapping: v_mfma_f32_32x32x2_f32, workgroup = 4 waves = 128 couts x 128 pixels, wave = 64 couts x 64 pixels (2 x 2 tiles,
// 64 accumulator registers).  Per chunk of 16 k rows every thread moves two 16-byte rows of W and of X global -> registers
// (requested two chunks ahead) -> LDS (double-buffered, one barrier per chunk); the A and
// B fragments are one ds_read_b32 each (row pitch 160 floats: the two k rows of a fragment sit 32 banks apart).
//
// pw_gemm_split_kernel: the same GEMM, tile, prefetch and epilogues with the contraction on v_mfma_f32_32x32x16_bf16 (16 x the
// f32 MFMA's rate).  Every f32 operand is split exactly into three bf16 pieces of 8 mantissa bits, x = h + m + l with h = bf16(x),
// m = bf16(x - h), l = bf16(x - h - m) (round to nearest even; both subtractions are exact in f32), and six of the nine piece
// products are accumulated in f32, smallest first: Wl Xh, Wh Xl, Wm Xm, Wm Xh, Wh Xm, Wh Xh.  The three dropped ones (ml, lm,
// ll) are ~2^-24 of the product: the result is limited by the f32 accumulation, as the f32 MFMA's is, at 0.375 x its MFMA
// cycles.  W arrives split (lass_launch_pw_split_weights, once per lass_finalize); X is split where it is staged, once per
// element, behind the unchanged f32 BN+FiLM+leaky of the transposed conv.  The LDS images are bf16, one plane per piece,
// [k octet][column] in 16-byte units: a fragment of a plane is ONE ds_read_b128, and 32 lanes read 512 contiguous bytes
// (conflict-free in the instruction's 16-lane groups; the octet pitch of 2 KiB separates lanes 0-31 from 32-63, which never
// share a group).  The staging thread owns one k octet of one column.  48 KiB of LDS, two workgroups per CU.
// Non-finite inputs are outside the split's contract (inf - inf): h = inf gives m = NaN where the f32 kernel gives inf.
#include <hip/hip_runtime.h>
#include "pw_gemm_split.h"  // the tile constants, acc_init, store_tile and split3: shared with wino4_gemm.hip

namespace {

constexpr int LP = NB + 32;  // LDS row pitch (floats) of both operand images

template <bool TCONV>
__global__ __launch_bounds__(NTHREADS, 2) void pw_gemm_kernel(ConvArgs p) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][KC * LP];  // [buffer][0 = W, 1 = X][k][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wp = wave & 1;  // this wave's 64 couts / 64 pixels of the workgroup tile
    int bx, by, b;
    block_coords(p, bx, by, b);
    const int n0 = by * NB;
    const unsigned P = (unsigned)p.H * (unsigned)p.W;  // pixels per channel (P % 4 == 0, host-checked)
    const unsigned p0 = (unsigned)bx * PB;
    const int K = TCONV ? p.Cin : p.Cin2;
    const unsigned Nw = (unsigned)p.Nw;

    // staging: thread = (row kr and kr + 8 of the chunk, 4 columns at c4); past the last pixel the columns are clamped to the
    // last aligned quad (loaded, never stored)
    const int kr = tid >> 5, c4 = (tid & 31) * 4;
    const float* xs = (TCONV ? p.in + (size_t)b * p.in_bs : p.in2 + (size_t)b * p.in2_bs) + min(p0 + (unsigned)c4, P - 4u) +
                      (size_t)kr * P;
    const float* ws = (TCONV ? p.w : p.w2) + n0 + c4 + (size_t)kr * Nw;
    const float* psc = TCONV ? p.pro_scale + kr : nullptr;
    const float* psh = TCONV ? p.pro_shift + (size_t)b * p.pro_shift_bs + kr : nullptr;
    // Two register stages (named fields, indexed only statically: the chunk loop is unrolled by two) keep the loads of a chunk
    // in flight for two chunks of MFMAs - one chunk (2 048 MFMA cycles per wave) is shorter than a memory round trip under load
    struct Stage {
        float4 x0, x1, w0, w1;
        float s0, s1, h0, h1;
    };
    Stage S0, S1;
    const auto gload = [&](Stage& st, int ch) {
        const size_t k = (size_t)ch * KC;
        st.x0 = *reinterpret_cast<const float4*>(xs + k * P);
        st.x1 = *reinterpret_cast<const float4*>(xs + (k + 8) * P);
        st.w0 = *reinterpret_cast<const float4*>(ws + k * Nw);
        st.w1 = *reinterpret_cast<const float4*>(ws + (k + 8) * Nw);
        if (TCONV) {
            st.s0 = psc[k];
            st.s1 = psc[k + 8];
            st.h0 = psh[k];
            st.h1 = psh[k + 8];
        }
    };
    const auto act = [](float4 v, float s, float h) {  // bn + FiLM + leaky of the transposed conv's input (resunet.py:247)
        return make_float4(leaky(fmaf(v.x, s, h)), leaky(fmaf(v.y, s, h)), leaky(fmaf(v.z, s, h)), leaky(fmaf(v.w, s, h)));
    };
    const auto sstore = [&](const Stage& st, int buf) {  // the prologue is applied here, once per staged element
        float* la = &lds[buf][0][kr * LP + c4];
        float* lb = &lds[buf][1][kr * LP + c4];
        *reinterpret_cast<float4*>(la) = st.w0;
        *reinterpret_cast<float4*>(la + 8 * LP) = st.w1;
        *reinterpret_cast<float4*>(lb) = TCONV ? act(st.x0, st.s0, st.h0) : st.x0;
        *reinterpret_cast<float4*>(lb + 8 * LP) = TCONV ? act(st.x1, st.s1, st.h1) : st.x1;
    };

    f32x16 acc[2][2];
    acc_init<TCONV>(p, acc, n0, wn, lane);

    // fragments: A[i = lane & 31][k = lane >> 5] = W[k][n], B[k = lane >> 5][j = lane & 31] = X[k][pixel]
    const int fo = (lane >> 5) * LP + (lane & 31);
    const auto mma = [&](int buf) {
        const float* la = &lds[buf][0][fo + wn * 64];
        const float* lb = &lds[buf][1][fo + wp * 64];
        float fa[KC / 2][2], fb[KC / 2][2];  // all fragments of the chunk requested up front: the reads overlap the MFMAs
#pragma unroll
        for (int ks = 0; ks < KC / 2; ++ks) {
            fa[ks][0] = la[2 * ks * LP];
            fa[ks][1] = la[2 * ks * LP + 32];
            fb[ks][0] = lb[2 * ks * LP];
            fb[ks][1] = lb[2 * ks * LP + 32];
        }
        __builtin_amdgcn_sched_barrier(0);  // (pinned: hipcc sinks each read to its MFMAs and waits lgkmcnt(0) in front of them)
#pragma unroll
        for (int ks = 0; ks < KC / 2; ++ks) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks][0], fb[ks][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks][0], fb[ks][1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks][1], fb[ks][0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks][1], fb[ks][1], acc[1][1], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // chunk c lives in stage c % 2 and LDS buffer c % 2; nch is even (host-checked).  LDS buffer b is rewritten only after the
    // barrier that follows every wave's MFMAs on it: one barrier per chunk.
    // The loads are unconditional (past the end: the last chunk again, never used) so that hipcc's wait in front of a stage's
    // LDS store counts only the younger stage's loads; a conditional load makes it vmcnt(0), one chunk of prefetch.
    const int nch = K / KC;
    gload(S0, 0);
    gload(S1, 1);
    sstore(S0, 0);
    gload(S0, min(2, nch - 1));
    __syncthreads();
    for (int ch = 0; ch < nch; ch += 2) {
        mma(0);  // chunk ch
        sstore(S1, 1);
        gload(S1, min(ch + 3, nch - 1));
        __syncthreads();
        mma(1);  // chunk ch + 1
        sstore(S0, 0);  // (behind the last chunk: unused)
        gload(S0, min(ch + 4, nch - 1));
        __syncthreads();
    }
    store_tile<TCONV>(p, acc, b, n0, p0, P, wn, wp, lane);
}

// ---- the split-bf16 form (its helpers: pw_gemm_split.h) ------------------------------------------------------------------------
// w [K][Nw] f32 -> dst [3 pieces h, m, l][K / 8][Nw][8] bf16: what a staging thread of the kernel below copies as one 16-byte load
// per piece.  One thread per (k octet, column).
__global__ __launch_bounds__(256) void pw_split_weights_kernel(const float* __restrict__ w, int K, int Nw, bf16x8* __restrict__ dst) {
    const size_t units = (size_t)(K / 8) * Nw, u = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    const size_t o = u / Nw, n = u - o * Nw;
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = w[(o * 8 + j) * Nw + n];
    bf16x8 h, m, l;
    split3(x, h, m, l);
    dst[u] = h;
    dst[units + u] = m;
    dst[2 * units + u] = l;
}

template <bool TCONV>
__global__ __launch_bounds__(NTHREADS, 2) void pw_gemm_split_kernel(ConvArgs p, PwSplitW sw) {
    constexpr bool XI = false, ACC2 = false;  // (one weight matrix for every clip, accumulators start at the bias, one set of them)
#include "pw_gemm_split_body.h"
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

bool lass_pw_gemm_supported(ConvKind kind, const ConvArgs& p) {
    const ConvShape s = lass_conv_shape(p);  // (the shape rules: conv_route.h)
    if (!(p.out && !p.out_bf16 && p.B > 0 && lass_pw_gemm_tile_shape(s))) return false;
    switch (kind) {
        case CONV2_SHORTCUT:
            return lass_pw_gemm_shortcut_shape(s) && p.in2 && p.w2 && p.bias && p.in2_bs % 4 == 0 && aligned16(p.in2) && aligned16(p.w2);
        case TCONV_ACT:
            return p.in && p.w && p.pro_scale && p.pro_shift && !p.in_bf16 && p.Cin > 0 && p.Cin % (2 * KC) == 0 && p.in_bs % 4 == 0 &&
                   (p.up_h == 1 || p.up_h == 2) && p.N % (2 * p.up_h) == 0 && p.out_bs % 2 == 0 && aligned16(p.in) && aligned16(p.w) &&
                   ((uintptr_t)p.out & 7u) == 0;
        default:
            return false;
    }
}

hipError_t lass_launch_pw_split_weights(const float* w, int K, int Nw, void* dst, hipStream_t stream) {
    if (!w || !dst || K <= 0 || K % 8 != 0 || Nw <= 0 || !aligned16(dst)) return hipErrorInvalidValue;
    const size_t units = (size_t)(K / 8) * Nw;
    hipLaunchKernelGGL(pw_split_weights_kernel, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, stream, w, K, Nw,
                       reinterpret_cast<bf16x8*>(dst));
    return hipGetLastError();
}

hipError_t lass_launch_pw_gemm(ConvKind kind, const ConvArgs& p0, hipStream_t stream, const PwSplitW& sw) {
    if (!lass_pw_gemm_supported(kind, p0) || (sw.w && !aligned16(sw.w))) return hipErrorInvalidValue;
    ConvArgs p = p0;
    p.gx = (int)(((long)p.H * p.W + PB - 1) / PB);
    p.gy = p.N / NB;
    p.xcd_map = ((long)p.gx * p.B) % 8 == 0;
    const dim3 grid((unsigned)((long)p.gx * p.gy * p.B));
    if (sw.w) {  // the plan's choice (conv_route.h: pw_split), never the batch's
        if (kind == TCONV_ACT)
            hipLaunchKernelGGL(pw_gemm_split_kernel<true>, grid, dim3(NTHREADS), 0, stream, p, sw);
        else
            hipLaunchKernelGGL(pw_gemm_split_kernel<false>, grid, dim3(NTHREADS), 0, stream, p, sw);
    } else if (kind == TCONV_ACT)
        hipLaunchKernelGGL(pw_gemm_kernel<true>, grid, dim3(NTHREADS), 0, stream, p);
    else
        hipLaunchKernelGGL(pw_gemm_kernel<false>, grid, dim3(NTHREADS), 0, stream, p);
    return hipGetLastError();
}
