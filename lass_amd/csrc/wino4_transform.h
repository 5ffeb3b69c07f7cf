// wino4_transform.h - the 1-D transforms of F(4x4,3x3) that wino4.hip's kernels and wino4_gemm.hip's scatter and gather share:
// one text, so that both routes form the same V bit for bit and fold M in the same order.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// 1-D input transform r = B^T d (6 -> 6), B^T of F(4,3): 12 instructions
__device__ __forceinline__ void bt6(const float (&d)[6], float (&r)[6]) {
    const float t0 = fmaf(-4.f, d[2], d[4]);   // d4 - 4 d2
    const float t1 = fmaf(-4.f, d[1], d[3]);   // d3 - 4 d1
    const float t2 = d[4] - d[2];
    const float u = d[3] - d[1];
    r[0] = fmaf(4.f, d[0], fmaf(-5.f, d[2], d[4]));
    r[1] = t0 + t1;
    r[2] = t0 - t1;
    r[3] = fmaf(2.f, u, t2);
    r[4] = fmaf(-2.f, u, t2);
    r[5] = fmaf(4.f, d[1], fmaf(-5.f, d[3], d[5]));
}

// 1-D output transform y = A^T m (6 -> 4)
__device__ __forceinline__ void at6(const float (&m)[6], float (&y)[4]) {
    const float s12 = m[1] + m[2], d12 = m[1] - m[2], s34 = m[3] + m[4], d34 = m[3] - m[4];
    y[0] = m[0] + s12 + s34;
    y[1] = fmaf(2.f, d34, d12);
    y[2] = fmaf(4.f, s34, s12);
    y[3] = fmaf(8.f, d34, d12) + m[5];
}

}  // namespace
