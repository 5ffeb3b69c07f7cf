// limiter.hip - the look-ahead limiter of the levelled export (lass_limit): planar float32 at the model rate -> the same planes under
// one gain curve per recording, linked across the channels, that holds gain x envelope under the ceiling.  lass_amd.loudness.limit
// is the float64 definition; DESIGN.md section 20.
//
// One workgroup makes kLimTile = LASS_LIMITER_TILE consecutive frames of one recording, in one launch and with no scratch: what a
// frame needs of its neighbours - the envelope of 2H frames on either side, the minima of H - the workgroup makes again for
// itself, so no tile reads what another wrote.  In LDS, beside polyphase.h's table of the (os, 1) filter and the 2H + 1 window taps,
//   X = the plane being staged over tile +- (2H + 10), zeros outside the row, one channel at a time (k_true_peak's stage: the
//       os - 1 interpolated phases of a frame are polyphase.h's fir_output over it, so e is bit-identical to lass_decode_resample
//       of the plane at (os, 1));
//   E = e over tile +- 2H, the maximum over the channels, a NaN counting as 0; later q = fl(g * G) over the tile;
//   A = r over tile +- 2H (1 outside the row).
// The minimum over |k - n| <= H costs O(log H) per frame: minima of 2^i neighbours are doubled between A and X (free once the
// envelope stands) up to p, the largest power of two in 2H + 1, and m[n] = min(A_p[n - H], A_p[n + H - p + 1]).  min is exact, so
// the scheme cannot change a bit.  The smoothing chain - one fmaf per tap, j = -H ... H, onto 0 - runs only in a wave that has
// some m' < 1 within reach of its 64 frames, and a frame of such a wave whose own 2H + 1 m' are all 1 still gets G = 1 exactly.
#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

#include "polyphase.h"

constexpr int kLimTile = LASS_LIMITER_TILE;
constexpr int kOsJ = 21;                // taps per phase of the (os, 1) filter: ceil((20*os + 1) / os)
constexpr int kOsHalo = (kOsJ - 1) / 2;
constexpr unsigned kOneBits = 0x3f800000u;

// The loops below that carry `#pragma clang loop ... interleave(disable)`: left alone, hipcc interleaves two of their iterations into
// v_pk_fma_f32 / v_pk_mul_f32, which no kernel of this library may carry (tests/test_host_cpu.py audits the ISA).

__host__ __device__ __forceinline__ size_t pad4(size_t n) { return (n + 3) & ~(size_t)3; }

// floats of LDS at reach H: table, window, X, E, A
__host__ __device__ __forceinline__ size_t limit_floats(int os, int H) {
    return pad4(os > 1 ? (size_t)os * (kOsJ | 1) : 0) + pad4(2 * (size_t)H + 1) + pad4((size_t)kLimTile + 4 * H + 2 * kOsHalo) +
           2 * pad4((size_t)kLimTile + 4 * H);
}

// |y|, a NaN counting as 0
__device__ __forceinline__ float magnitude(float y) {
    const unsigned a = __float_as_uint(y) & 0x7fffffffu;
    return a > 0x7f800000u ? 0.f : __uint_as_float(a);
}

// the gain frame n may have at most: 1 if fl(g * e) <= c, else fl(c / fl(g * e))
__device__ __forceinline__ float required(float g, float e, float c) {
    const float a = __fmul_rn(g, e);
    return a <= c ? 1.0f : __fdiv_rn(c, a);
}

// kTrue false: os == 1, the envelope is |x| alone (no table, no interpolated phase)
template <bool kTrue>
__global__ __launch_bounds__(kThreads) void k_limit(const float* __restrict__ planes, long long row_stride, long long plane_stride, int ch,
                                                    int L, int os, const float* __restrict__ os_taps, int n_os_taps,
                                                    const float* __restrict__ gain, float ceiling, int H,
                                                    const float* __restrict__ window, float* __restrict__ out, long long out_row_stride,
                                                    long long out_plane_stride, float* __restrict__ curve, float* __restrict__ envelope,
                                                    long long curve_row_stride, unsigned* __restrict__ min_gain, int* __restrict__ frames) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const long long n0 = (long long)blockIdx.x * kLimTile;
    const int nout = (int)(L - n0 < kLimTile ? L - n0 : kLimTile);
    const int R = nout + 4 * H;                 // frames of E and A: tile +- 2H
    const long long lo = n0 - 2 * H;            // the frame E[0] holds
    const int W = 2 * H + 1;
    float* tab = lds;
    float* win = tab + pad4(kTrue ? (size_t)os * (kOsJ | 1) : 0);
    float* X = win + pad4((size_t)W);
    float* E = X + pad4((size_t)kLimTile + 4 * H + 2 * kOsHalo);
    float* A = E + pad4((size_t)kLimTile + 4 * H);
    const float* rec = planes + (size_t)blockIdx.y * row_stride;
    const float g = gain[blockIdx.y];

    FirTile T2;
    T2.J = kOsJ;
    T2.Jp = kOsJ | 1;
    T2.up = os;
    T2.down = 1;
    T2.tab = tab;
    T2.span = X;
    T2.r0 = 0;
    T2.n0 = 0;
    T2.mlo = 0;
    T2.nout = T2.S = 0;
    if constexpr (kTrue) fir_table(T2, os_taps, n_os_taps);
    for (int k = tid; k < W; k += kThreads) win[k] = window[k];

    // e: every thread keeps its own frames of E over the channels, so only X is handed over between them
    for (int c = 0; c < ch; ++c) {
        const float* x0 = rec + (size_t)c * plane_stride;
        if (c) __syncthreads();                           // the previous channel's reads of X
        for (int s = tid; s < R + 2 * kOsHalo; s += kThreads) {
            const long long f = lo - kOsHalo + s;
            X[s] = (f >= 0 && f < L) ? x0[f] : 0.f;
        }
        __syncthreads();
        for (int s = tid; s < R; s += kThreads) {
            const long long f = lo + s;
            float e = 0.f;
            if (f >= 0 && f < L) {
                e = magnitude(X[s + kOsHalo]);
                if constexpr (kTrue) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                    for (int p = 1; p < os; ++p) e = fmaxf(e, magnitude(fir_output(T2, s * os + p)));
                }
            }
            E[s] = c ? fmaxf(E[s], e) : e;
        }
    }
    // r, 1 outside the row
#pragma clang loop vectorize(disable) interleave(disable)
    for (int s = tid; s < R; s += kThreads) {
        const long long f = lo + s;
        A[s] = (f >= 0 && f < L) ? required(g, E[s], ceiling) : 1.0f;
    }
    __syncthreads();                                      // A stands, and X is free
    // src[s] = min r[s ... s + p - 1] (cut at the region's end), p doubling
    float *src = A, *dst = X;
    int p = 1;
    for (; 2 * p <= W; p *= 2) {
        for (int s = tid; s < R; s += kThreads) dst[s] = s + p < R ? fminf(src[s], src[s + p]) : src[s];
        __syncthreads();
        float* t = src;
        src = dst;
        dst = t;
    }
    // m' over tile +- H: the two overlapping minima of p that cover |k - n| <= H; 1 outside the row
    float* M = dst;
    for (int s = H + tid; s < R - H; s += kThreads) {
        const long long f = lo + s;
        M[s] = (f >= 0 && f < L) ? fminf(src[s - H], src[s + H - p + 1]) : 1.0f;
    }
    __syncthreads();

    // G and q = fl(g * G) of the tile's frames, 64 consecutive frames per wave
    unsigned lowest = kOneBits;
    int limited = 0;
    float* crow = curve ? curve + (size_t)blockIdx.y * curve_row_stride + n0 : nullptr;
    float* erow = envelope ? envelope + (size_t)blockIdx.y * curve_row_stride + n0 : nullptr;
    for (int base = tid - lane; base < nout; base += kThreads) {
        const int i = base + lane;
        const bool mine = i < nout;
        const int s = 2 * H + i;
        // whether any m' within reach of the wave's frames is below 1 (wave-uniform)
        const int last = (base + 63 < nout - 1 ? base + 63 : nout - 1) + 3 * H;
        bool some = false;
        for (int k = base + H + lane; k <= last; k += 64) some |= M[k] < 1.0f;
        float G = 1.0f;
        if (__ballot(some) != 0ull && mine) {
            const float* m = M + s - H;
            float acc = 0.f, least = 1.0f;
            for (int j = 0; j < W; ++j) {
                const float v = m[j];
                acc = fmaf(win[j], v, acc);
                least = fminf(least, v);
            }
            if (least < 1.0f) G = acc;
        }
        bool bit = false;
        if (mine) {
            const float e = E[s];
            G = fminf(G, required(g, e, ceiling));
            bit = M[s] < 1.0f;
            if (crow) crow[i] = G;
            if (erow) erow[i] = e;
            E[s] = __fmul_rn(g, G);                       // read again by this thread alone
            const unsigned u = __float_as_uint(G);
            lowest = u < lowest ? u : lowest;
        }
        limited += __popcll(__ballot(bit));
    }
    for (int w = 32; w > 0; w >>= 1) {
        const unsigned o = (unsigned)__shfl_xor((int)lowest, w);
        lowest = o < lowest ? o : lowest;
    }
    if (lane == 0) {
        if (min_gain && lowest < kOneBits) atomicMin(min_gain + blockIdx.y, lowest);
        if (frames && limited) atomicAdd(frames + blockIdx.y, limited);
    }

    // v = fl(q * x)
    float* orow = out + (size_t)blockIdx.y * out_row_stride + n0;
    for (int c = 0; c < ch; ++c) {
        const float* x0 = rec + (size_t)c * plane_stride + n0;
        float* o = orow + (size_t)c * out_plane_stride;
#pragma clang loop vectorize(disable) interleave(disable)
        for (int i = tid; i < nout; i += kThreads) o[i] = __fmul_rn(E[2 * H + i], x0[i]);
    }
}

}  // namespace

hipError_t lass_launch_limit(const PlaneRows& P, const Oversampler& O, const float* gain, float ceiling, int H, const float* window,
                             const PlaneRows& out, float* curve, float* envelope, long long curve_row_stride, float* min_gain,
                             int* frames, hipStream_t stream) {
    const int B = P.B, L = P.L, os = O.os;
    if (B <= 0 || B > 65535 || P.ch < 1 || P.ch > 8 || L <= 0 || H < 1 || H > LASS_LIMITER_MAX_H || (os != 1 && os != 2 && os != 4) ||
        (os > 1 && O.n_taps != 20 * os + 1))
        return hipErrorInvalidValue;
    hipError_t e;
    if (min_gain) {
        e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(min_gain), (int)kOneBits, (size_t)B, stream);
        if (e != hipSuccess) return e;
    }
    if (frames) {
        e = hipMemsetAsync(frames, 0, (size_t)B * sizeof(int), stream);
        if (e != hipSuccess) return e;
    }
    const size_t lds = limit_floats(os, H) * sizeof(float);   // 41 KiB at H = 512, os = 4: under the 64 KiB that need no attribute
    const dim3 grid((unsigned)(((long long)L + kLimTile - 1) / kLimTile), B);
    hipLaunchKernelGGL(os > 1 ? k_limit<true> : k_limit<false>, grid, dim3(kThreads), lds, stream, P.p, P.row_stride, P.plane_stride, P.ch, L,
                       os, O.taps, O.n_taps, gain, ceiling, H, window, const_cast<float*>(out.p), out.row_stride, out.plane_stride, curve,
                       envelope, curve_row_stride, reinterpret_cast<unsigned*>(min_gain), frames);
    return hipGetLastError();
}
