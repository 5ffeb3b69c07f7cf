// tower_parts.h - the device parts the CLAP towers (text.hip, audio_clap.hip) share: the exact-f32 MFMA GEMM and its launcher, the
// row LayerNorm and the final L2 normalisation.  Shared by inclusion so that both translation units compile the same kernel
// text.  Include inside an anonymous namespace, after <hip/hip_runtime.h>.
#pragma once

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kProj = 512;       // width of the joint embedding both towers project to
constexpr float kLnEps = 1e-5f;  // roberta-base config.json layer_norm_eps (HF RobertaConfig() defaults to 1e-12); HTSAT: nn.LayerNorm's default

__device__ __forceinline__ float wave_sum(float v) {
    // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

enum Epi { EPI_BIAS = 0, EPI_GELU = 1, EPI_RESID = 2, EPI_TANH = 3, EPI_RELU = 4 };

constexpr int BM = 64, BN = 64, BK = 16, LDT = BM + 32;  // +32: the two k rows one MFMA reads land in different banks
constexpr int KC = 64;  // k per accumulation chunk: one 3072-long f32 chain carries about 5 x the rounding error of 48 chains of 64 summed

// Y[M,N] = epi(X[M,K] . W[N,K]^T + bias), row-major, N % 64 == 0, K % 16 == 0.  EPI_RESID adds Y's previous value
// (the residual stream, updated in place: each element is read and written by the same lane).  256 threads = 4 waves,
// each a 32x32 quarter of the 64x64 tile on v_mfma_f32_32x32x2_f32 (exact f32, k-ordered FMA chain).  One tile shape for
// every M, so a row's result does not depend on M or on where the row sits.  The chain restarts every KC of k and the
// finished chunks are summed in order: with one chain over all of K the towers' embeddings lay 2.5 to 3.5 x as far from a
// float64 reference as ATen's float32 does (K = 3072 in the FFN), chunked they lie as close as ATen's
// (tests/test_clap_text_edges_gpu.py); 16 VALU adds per 32 MFMAs.
template <int EPI>
__global__ __launch_bounds__(256) void k_gemm(const float* __restrict__ X, const float* __restrict__ W,
                                              const float* __restrict__ bias, float* Y, int M, int N, int K) {
    __shared__ __attribute__((aligned(16))) float As[BK * LDT], Bs[BK * LDT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wm = w & 1, wn = w >> 1;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int lr = t >> 2, lc = (t & 3) * 4;  // this thread's staging row and k quad
    const bool xrow = m0 + lr < M;
    const float* xp = X + (size_t)(xrow ? m0 + lr : 0) * K + lc;
    const float* wp = W + (size_t)(n0 + lr) * K + lc;
    float4 ra = xrow ? *(const float4*)xp : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 rb = *(const float4*)wp;
    f32x16 acc, part;  // part: the k-ordered chain of the current KC-long chunk of k; acc: the sum of the finished chunks
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = part[i] = 0.f;
    const int ai = wm * 32 + (lane & 31), bi = wn * 32 + (lane & 31), kh = lane >> 5;
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();
        As[(lc + 0) * LDT + lr] = ra.x;
        As[(lc + 1) * LDT + lr] = ra.y;
        As[(lc + 2) * LDT + lr] = ra.z;
        As[(lc + 3) * LDT + lr] = ra.w;
        Bs[(lc + 0) * LDT + lr] = rb.x;
        Bs[(lc + 1) * LDT + lr] = rb.y;
        Bs[(lc + 2) * LDT + lr] = rb.z;
        Bs[(lc + 3) * LDT + lr] = rb.w;
        __syncthreads();
        if (k0 + BK < K) {
            ra = xrow ? *(const float4*)(xp + k0 + BK) : make_float4(0.f, 0.f, 0.f, 0.f);
            rb = *(const float4*)(wp + k0 + BK);
        }
#pragma unroll
        for (int kk = 0; kk < BK / 2; ++kk) {
            const float a = As[(2 * kk + kh) * LDT + ai];
            const float bb = Bs[(2 * kk + kh) * LDT + bi];
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bb, part, 0, 0, 0);
        }
        if ((k0 + BK) % KC == 0 || k0 + BK >= K) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                acc[i] += part[i];
                part[i] = 0.f;
            }
        }
    }
    const int n = n0 + wn * 32 + (lane & 31);
    const float bn = bias[n];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int m = m0 + wm * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
        if (m >= M) continue;
        float v = acc[i] + bn;
        float* yp = Y + (size_t)m * N + n;
        if (EPI == EPI_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));
        if (EPI == EPI_RESID) v = v + *yp;
        if (EPI == EPI_TANH) v = tanhf(v);
        if (EPI == EPI_RELU) v = fmaxf(v, 0.f);
        *yp = v;
    }
}

template <int EPI>
void gemm(const float* X, const float* W, const float* b, float* Y, int M, int N, int K, hipStream_t st) {
    hipLaunchKernelGGL(k_gemm<EPI>, dim3(N / BN, (M + BM - 1) / BM), dim3(256), 0, st, X, W, b, Y, M, N, K);
}

template <int NPL>  // LayerNorm of a row of 64 * NPL values held as element lane + 64 j, written to y
__device__ __forceinline__ void ln_row(float (&x)[NPL], const float* __restrict__ g, const float* __restrict__ b,
                                       float* __restrict__ y, int lane) {
    constexpr float inv = 1.0f / (64 * NPL);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) s += x[j];
    const float mean = wave_sum(s) * inv;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const float d = x[j] - mean;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * inv + kLnEps);
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int k = lane + 64 * j;
        y[k] = (x[j] - mean) * rstd * g[k] + b[k];
    }
}

// F.normalize(x, dim=-1): x / max(||x||, 1e-12), one wave per row of 512.
__global__ __launch_bounds__(256) void k_l2norm(const float* __restrict__ x, int N, float* __restrict__ y) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;
    float v[kProj / 64], s = 0.f;
#pragma unroll
    for (int j = 0; j < kProj / 64; ++j) {
        v[j] = x[(size_t)r * kProj + lane + 64 * j];
        s += v[j] * v[j];
    }
    const float inv = 1.0f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);
#pragma unroll
    for (int j = 0; j < kProj / 64; ++j) y[(size_t)r * kProj + lane + 64 * j] = v[j] * inv;
}
