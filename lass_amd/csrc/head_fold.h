// head_fold.h - decoder_block6's conv2 and 1x1 shortcut composed with after_conv (resunet.py:163,568-570).  Nothing non-linear
// sits between x12 = shortcut(cat) + conv2(h) and after_conv(x12), so the Q = 3 mask logits are one linear map of h and cat:
//      logit[q] = sum_{c,tap} W2'[q][c][tap] h[c] + sum_k Wsc'[q][k] cat[k] + b'[q]
//      W2' = Wa W2,   Wsc' = Wa Wsc,   b' = Wa bsc + ba
// formed here in double from the f32 checkpoint, rounded to f32 ONCE and zero-padded to 16 rows (Wsc': one 16x16x4 MFMA tile); W2' then
// goes through the F(4x4,3x3) weight transform G g G^T (double, as wino4_weights_kernel) into the LDS images that
// wino4_headfold_kernel copies in by LDS-DMA (the compact 4-row form, u4; the 16-row form holds the same values).  The images
// depend on the checkpoint only: lass_finalize prepares them once.
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

// The compact image of the same values, which the folded-head kernels copy in: their contraction runs on 4-row MFMA blocks
// (v_mfma_f32_4x4x1_16b_f32: rows = the 3 logits and ONE zero row), so only rows 0 .. 3 of the 16 exist here.  One 8-channel
// chunk: [k-step 2][row 4][xi 36][kq = cin % 4] - a lane's A operands of one chunk, the 9 xi of its wave x 4 channels of its
// k-step, are 36 consecutive floats (9 16-byte reads) - followed by zeros up to a whole number of 1-KiB LDS-DMA pieces.
constexpr int kHeadFoldRows4 = 4;
constexpr int kHeadFoldU4Live = kWino4NXI * kWino4KC * kHeadFoldRows4;      // 1 152 floats addressed by head_fold_u4_index
constexpr int kHeadFoldU4Floats = (kHeadFoldU4Live + 255) / 256 * 256;      // 1 280: five pieces

inline size_t head_fold_u4_index(int cin, int xi, int row) {
    const int k = (cin & 7) >> 2, kq = cin & 3;
    return (size_t)(cin / kWino4KC) * kHeadFoldU4Floats + (size_t)((k * kHeadFoldRows4 + row) * kWino4NXI + xi) * 4 + kq;
}

struct HeadFold {
    int Q = 0, C = 0, K = 0;
    std::vector<float> w2;    // W2'  [16][C][3][3], rows >= Q zero
    std::vector<float> wsc;   // Wsc' [K][16], columns >= Q zero (the kernel's A operand of input channel k is one row)
    std::vector<float> bias;  // b'   [16]
    std::vector<float> u;     // G W2' G^T as LDS images: C / 8 chunks of kHeadFoldUFloats (head_fold_u_index)
    std::vector<float> u4;    // ... rows 0 .. 3 of it, compact: C / 8 chunks of kHeadFoldU4Floats (head_fold_u4_index); empty if Q > 3
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
    f.u4.clear();
    if (Q < kHeadFoldRows4) f.u4.assign((size_t)(C / kWino4KC) * kHeadFoldU4Floats, 0.f);  // (row 3 stays the zero row)
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
            if (!f.u4.empty())  // the same rounded values, not a second rounding
                for (int xi = 0; xi < kWino4NXI; ++xi) f.u4[head_fold_u4_index(ci, xi, q)] = f.u[head_fold_u_index(ci, xi, q)];
        }
    return true;
}

// ---- the composed shortcut at the producers of its inputs (conv_route.h: plan_head_sc_fold) ------------------------------------
// cat = (up, skip) in api.hip's concat order, up = Wt act(x11) a kernel == stride transposed conv without a bias and with nothing
// non-linear behind it.  So Wsc' cat = Wsc'_skip x1 + Wt' act(x11) with
//      Wt'[k][q][a][bb] = sum_c Wsc'_up[q][c] Wt[k][c][a][bb]          (Wsc' = Wa Wsc, split at channel Cup)
// again in double from the f32 checkpoint and rounded to f32 ONCE (Wsc' enters in double, not as HeadFold::wsc).  b' is untouched.
constexpr int kHeadScCols = 64;   // columns (the pitch) of the slab, as a cout block of the transposed conv has
constexpr int kHeadScLive = 32;   // ... of which at most the first 32 are live: Q * uh * uw columns, the rest zero (the kernel reads 16)

struct HeadScFold {
    int Q = 0, Cup = 0, Cskip = 0, Kt = 0;
    std::vector<float> wt;     // Wt' [Kt][64], column (q * uh + a) * uw + bb as the transposed conv's own (co, a, bb); the rest zero
    std::vector<float> wskip;  // Wsc'_skip [Q][Cskip]: the table of encoder_block1.conv2's epilogue
};

// wsc (N, Cup + Cskip), wa (Q, N), wt (Kt, Cup, uh, uw): PyTorch layouts (ConvTranspose2d: input channel first).  false: a shape
// the slab cannot hold.
inline bool compose_head_sc_fold(const float* wsc, const float* wa, const float* wt, int N, int Cup, int Cskip, int Q, int Kt, int uh, int uw,
                                 HeadScFold* out) {
    if (!wsc || !wa || !wt || !out || N <= 0 || Cup <= 0 || Cskip <= 0 || Q <= 0 || Kt <= 0 || uh <= 0 || uw <= 0 || Q * uh * uw > kHeadScLive)
        return false;
    HeadScFold& f = *out;
    f.Q = Q; f.Cup = Cup; f.Cskip = Cskip; f.Kt = Kt;
    f.wt.assign((size_t)Kt * kHeadScCols, 0.f);
    f.wskip.assign((size_t)Q * Cskip, 0.f);
    const int K = Cup + Cskip, S = uh * uw;
    std::vector<double> wq(K);  // row q of Wsc' = Wa Wsc, in double
    for (int q = 0; q < Q; ++q) {
        for (int k = 0; k < K; ++k) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)wsc[(size_t)n * K + k];
            wq[k] = s;
        }
        for (int c = 0; c < Cskip; ++c) f.wskip[(size_t)q * Cskip + c] = (float)wq[Cup + c];
        for (int k = 0; k < Kt; ++k)
            for (int s = 0; s < S; ++s) {
                double t = 0;
                for (int c = 0; c < Cup; ++c) t += wq[c] * (double)wt[((size_t)k * Cup + c) * S + s];
                f.wt[(size_t)k * kHeadScCols + q * S + s] = (float)t;
            }
    }
    return true;
}
