// pw_gemm_split.h - what pw_gemm.hip's kernels and wino4_gemm.hip's batched GEMM share: the workgroup tile, the accumulator and
// epilogue helpers, and the exact three-way bf16 split of an f32 operand.  The body of the split-bf16 kernel itself is text
// (pw_gemm_split_body.h), included once per kernel.
#pragma once
#include <hip/hip_runtime.h>
#include "kernels.h"
#include "pixel_ops.h"
#include "wino_common.h"

namespace {

constexpr int NTHREADS = 256;
constexpr int NB = kPwGemmNB;  // couts of a workgroup
constexpr int PB = 128;      // pixels of a workgroup
constexpr int KC = kPwGemmKC;  // k rows of a chunk

typedef float f32x16 __attribute__((ext_vector_type(16)));

// accumulators start at the shortcut's bias (loaded in the shadow of the first chunk: read in the epilogue, every load would wait
// behind the store before it)
template <bool TCONV>
__device__ __forceinline__ void acc_init(const ConvArgs& p, f32x16 (&acc)[2][2], int n0, int wn, int lane) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = TCONV ? 0.f : p.bias[n0 + wn * 64 + i * 32 + 4 * (lane >> 5) + (r & 3) + 8 * (r >> 2)];
            acc[i][0][r] = v;
            acc[i][1][r] = v;
        }
}

__device__ __forceinline__ void acc_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][0][r] = acc[i][1][r] = 0.f;
}

// Both kernels' epilogue: D row (cout) = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), column (pixel) = lane & 31
template <bool TCONV>
__device__ __forceinline__ void store_tile(const ConvArgs& p, const f32x16 (&acc)[2][2], int b, int n0, unsigned p0, unsigned P, int wn,
                                           int wp, int lane) {
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
        const unsigned pj = p0 + (unsigned)(wp * 64 + tp * 32 + (lane & 31));
        if (pj >= P) continue;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            const int nb = n0 + wn * 64 + tn * 32 + 4 * (lane >> 5);
            if (!TCONV) {
                float* dst = p.out + (size_t)b * p.out_bs + pj;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int n = nb + (r & 3) + 8 * (r >> 2);
                    dst[(size_t)n * P] = acc[tn][tp][r];
                }
            } else {
                // n = co * (2 up_h) + a * 2 + bb: registers (r, r + 1), r even, are bb = 0 / 1 of one (co, a) - 8 contiguous bytes
                const unsigned y = pj / (unsigned)p.W, x = pj - y * (unsigned)p.W;
                const int uhw = p.up_h * 2;
                const size_t oHW = (size_t)P * uhw;
                const unsigned oW = 2u * (unsigned)p.W;
                float* ob = p.out + (size_t)b * p.out_bs + (size_t)(y * p.up_h) * oW + 2u * x;
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int n = nb + (r & 3) + 8 * (r >> 2);
                    const int co = n / uhw, a = (n % uhw) >> 1;
                    *reinterpret_cast<float2*>(ob + (size_t)co * oHW + (size_t)a * oW) = make_float2(acc[tn][tp][r], acc[tn][tp][r + 1]);
                }
            }
        }
    }
}

// ---- the split-bf16 form ---------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int SPLANE = (KC / 8) * NB;  // 16-byte units of one piece's LDS plane: [k octet][column]  (NB == PB)
static_assert(NB == PB, "both operand images have 128 columns");

// x[i] = h[i] + m[i] + l[i] exactly, 8 mantissa bits each.  The conversions are gfx950's packed round-to-nearest-even, one per
// pair; a piece goes back to f32 as its 16 bits in the upper half of a dword.
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pair(float a, float b, float& fa, float& fb) {
    const f32x2 v = {a, b};
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
    fa = __uint_as_float(u << 16);
    fb = __uint_as_float(u & 0xffff0000u);
    return u;
}
__device__ __forceinline__ void split3(const float (&x)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    u32x4 hu, mu, lu;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float f0, f1, g0, g1;
        hu[i] = cvt_pair(x[2 * i], x[2 * i + 1], f0, f1);
        const float r0 = x[2 * i] - f0, r1 = x[2 * i + 1] - f1;
        mu[i] = cvt_pair(r0, r1, g0, g1);
        lu[i] = cvt_pair(r0 - g0, r1 - g1, f0, f1);
    }
    h = __builtin_bit_cast(bf16x8, hu);
    m = __builtin_bit_cast(bf16x8, mu);
    l = __builtin_bit_cast(bf16x8, lu);
}

}  // namespace
