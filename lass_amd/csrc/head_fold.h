// head_fold.h - decoder_block6's conv2 and 1x1 shortcut composed with after_conv (resunet.py:163,568-570).  Nothing non-linear
// sits between x12 = shortcut(cat) + conv2(h) and after_conv(x12), so the Q = 3 mask logits are one linear map of h and cat:
//      logit[q] = sum_{c,tap} W2'[q][c][tap] h[c] + sum_k Wsc'[q][k] cat[k] + b'[q]
//      W2' = Wa W2,   Wsc' = Wa Wsc,   b' = Wa bsc + ba
// formed here in double from the f32 checkpoint, rounded to f32 ONCE and zero-padded to the 16 rows of one MFMA tile; W2' then
// goes through the F(4x4,3x3) weight transform G g G^T (double, as wino4_weights_kernel) into the LDS images that
// wino4_headfold_kernel copies in by LDS-DMA.  The images depend on the checkpoint only: lass_finalize prepares them once.
// Host only and free of HIP, as conv_route.h: tools/head_fold_check.cpp holds the algebra and the padding on the CPU.
#pragma once
#include <stddef.h>

#include <vector>

#include "conv_route.h"

// floats of one 8-channel chunk's image: [xi pair 18][k-step 2][kq = cin % 4][row 16][xi & 1] - a lane's 8-byte read at
// ((pair * 2 + k) * 64 + kq * 16 + row) * 2 is the A operand of xi = 2 pair and 2 pair + 1 for k-step k
constexpr int kHeadFoldUFloats = kWino4NXI * kWino4KC * kHeadFoldRows;

inline size_t head_fold_u_index(int cin, int xi, int row) {
    const int k = (cin & 7) >> 2, kq = cin & 3;
    return (size_t)(cin / kWino4KC) * kHeadFoldUFloats + (size_t)(((xi >> 1) * 2 + k) * 64 + kq * kHeadFoldRows + row) * 2 + (xi & 1);
}

struct HeadFold {
    int Q = 0, C = 0, K = 0;
    std::vector<float> w2;    // W2'  [16][C][3][3], rows >= Q zero
    std::vector<float> wsc;   // Wsc' [K][16], columns >= Q zero (the kernel's A operand of input channel k is one row)
    std::vector<float> bias;  // b'   [16]
    std::vector<float> u;     // G W2' G^T as LDS images: C / 8 chunks of kHeadFoldUFloats (head_fold_u_index)
};

// w2 (N, C, 3, 3), wsc (N, K), bsc (N), wa (Q, N), ba (Q): PyTorch layouts.  false: a shape the images cannot hold.
inline bool compose_head_fold(const float* w2, const float* wsc, const float* bsc, const float* wa, const float* ba, int N, int C, int K,
                              int Q, HeadFold* out) {
    if (!w2 || !wsc || !bsc || !wa || !ba || !out || N <= 0 || C <= 0 || C % kWino4KC != 0 || K <= 0 || Q <= 0 || Q > kHeadFoldRows)
        return false;
    HeadFold& f = *out;
    f.Q = Q; f.C = C; f.K = K;
    f.w2.assign((size_t)kHeadFoldRows * C * 9, 0.f);
    f.wsc.assign((size_t)K * kHeadFoldRows, 0.f);
    f.bias.assign(kHeadFoldRows, 0.f);
    f.u.assign((size_t)(C / kWino4KC) * kHeadFoldUFloats, 0.f);
    for (int q = 0; q < Q; ++q) {
        for (int i = 0; i < C * 9; ++i) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)w2[(size_t)n * C * 9 + i];
            f.w2[(size_t)q * C * 9 + i] = (float)s;
        }
        for (int k = 0; k < K; ++k) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)wsc[(size_t)n * K + k];
            f.wsc[(size_t)k * kHeadFoldRows + q] = (float)s;
        }
        double s = ba[q];
        for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)bsc[n];
        f.bias[q] = (float)s;
    }
    const double G[6][3] = {{0.25, 0, 0},           {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                            {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6},  {0, 0, 1}};
    for (int q = 0; q < Q; ++q)
        for (int ci = 0; ci < C; ++ci) {
            const float* g = &f.w2[((size_t)q * C + ci) * 9];
            double t[6][3];
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 3; ++c) t[a][c] = G[a][0] * (double)g[0 * 3 + c] + G[a][1] * (double)g[1 * 3 + c] + G[a][2] * (double)g[2 * 3 + c];
            for (int a = 0; a < 6; ++a)
                for (int c = 0; c < 6; ++c)
                    f.u[head_fold_u_index(ci, a * 6 + c, q)] = (float)(t[a][0] * G[c][0] + t[a][1] * G[c][1] + t[a][2] * G[c][2]);
        }
    return true;
}
