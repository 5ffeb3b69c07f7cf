// head_fold_check.cpp - the composition of lass_amd/csrc/head_fold.h on the CPU: decoder_block6's conv2 + 1x1 shortcut composed
// with after_conv must give after_conv(conv2(h) + shortcut(cat)) on random small weights, in double, and the padded images
// must be zero outside the 3 logit rows; the compact 4-row image the kernels copy in must hold the 16-row image's rows 0 .. 3, value
// for value.  Host only:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I lass_amd/csrc tools/head_fold_check.cpp -o tools/bin/head_fold_check
// Prints one line per check and "ok"; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "head_fold.h"

namespace {

unsigned long long g_state = 0x9E3779B97F4A7C15ull;
float rnd() {  // uniform in [-1, 1), 24 bits
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(g_state >> 40) / (double)(1ull << 23) - 1.0);
}
std::vector<float> rnd_vec(size_t n, float scale) {
    std::vector<float> v(n);
    for (auto& x : v) x = rnd() * scale;
    return v;
}

constexpr int H = 8, W = 8;

// out[n][y][x] = sum_{c,ky,kx} w[n][c][ky][kx] in[c][y + ky - 1][x + kx - 1], zero padding (cross-correlation, as F.conv2d)
std::vector<double> conv3x3(const float* w, int N, int C, const std::vector<float>& in) {
    std::vector<double> out((size_t)N * H * W, 0.0);
    for (int n = 0; n < N; ++n)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double s = 0;
                for (int c = 0; c < C; ++c)
                    for (int ky = 0; ky < 3; ++ky)
                        for (int kx = 0; kx < 3; ++kx) {
                            const int yy = y + ky - 1, xx = x + kx - 1;
                            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                            s += (double)w[(((size_t)n * C + c) * 3 + ky) * 3 + kx] * (double)in[((size_t)c * H + yy) * W + xx];
                        }
                out[((size_t)n * H + y) * W + x] = s;
            }
    return out;
}

int fail(const char* what) {
    printf("FAILED: %s\n", what);
    return 1;
}

int check(int N, int C, int K, int Q) {
    const std::vector<float> w2 = rnd_vec((size_t)N * C * 9, 0.2f), wsc = rnd_vec((size_t)N * K, 0.3f), bsc = rnd_vec(N, 0.5f);
    const std::vector<float> wa = rnd_vec((size_t)Q * N, 0.4f), ba = rnd_vec(Q, 0.5f);
    const std::vector<float> h = rnd_vec((size_t)C * H * W, 1.f), cat = rnd_vec((size_t)K * H * W, 1.f);
    HeadFold f;
    if (!compose_head_fold(w2.data(), wsc.data(), bsc.data(), wa.data(), ba.data(), N, C, K, Q, &f)) return fail("compose_head_fold refused the shape");
    if (f.w2.size() != (size_t)kHeadFoldRows * C * 9 || f.wsc.size() != (size_t)K * kHeadFoldRows || f.bias.size() != (size_t)kHeadFoldRows ||
        f.u.size() != (size_t)(C / kWino4KC) * kHeadFoldUFloats)
        return fail("image sizes");

    // ---- the algebra: reference = after_conv(conv2(h) + shortcut(cat) + bsc) + ba, all in double from the f32 weights --------
    const std::vector<double> x12c = conv3x3(w2.data(), N, C, h);
    const std::vector<double> folded = conv3x3(f.w2.data(), kHeadFoldRows, C, h);
    double worst = 0, scale = 0;
    for (int q = 0; q < Q; ++q)
        for (int px = 0; px < H * W; ++px) {
            double ref = ba[q];
            for (int n = 0; n < N; ++n) {
                double x12 = x12c[(size_t)n * H * W + px] + (double)bsc[n];
                for (int k = 0; k < K; ++k) x12 += (double)wsc[(size_t)n * K + k] * (double)cat[(size_t)k * H * W + px];
                ref += (double)wa[q * N + n] * x12;
            }
            double got = folded[(size_t)q * H * W + px] + (double)f.bias[q];
            for (int k = 0; k < K; ++k) got += (double)f.wsc[(size_t)k * kHeadFoldRows + q] * (double)cat[(size_t)k * H * W + px];
            worst = std::fmax(worst, std::fabs(got - ref));
            scale = std::fmax(scale, std::fabs(ref));
        }
    // The composed weights are rounded to f32 ONCE (2^-24 relative each); the sums over C * 9 + K + 1 of them carry that rounding
    // and nothing else.  The composition itself, before the rounding, is held to the 1e-12 below.
    printf("N=%d C=%d K=%d Q=%d: f32-rounded images against the reference: max |diff| %.3e of %.3e\n", N, C, K, Q, worst, scale);
    if (!(worst <= scale * 2e-6)) return fail("the rounded images are off by more than f32 rounding of the weights");

    // ---- ... and the composition before the one rounding: recomputed here in double and compared with the double reference -----
    worst = 0;
    {
        std::vector<double> w2d((size_t)Q * C * 9), wscd((size_t)Q * K), bd(Q);
        for (int q = 0; q < Q; ++q) {
            for (int i = 0; i < C * 9; ++i) {
                double s = 0;
                for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)w2[(size_t)n * C * 9 + i];
                w2d[(size_t)q * C * 9 + i] = s;
                // the image holds exactly this value, rounded once
                if (f.w2[(size_t)q * C * 9 + i] != (float)s) return fail("W2' is not the f32 rounding of the double composition");
            }
            for (int k = 0; k < K; ++k) {
                double s = 0;
                for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)wsc[(size_t)n * K + k];
                wscd[(size_t)q * K + k] = s;
                if (f.wsc[(size_t)k * kHeadFoldRows + q] != (float)s) return fail("Wsc' is not the f32 rounding of the double composition");
            }
            double s = ba[q];
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)bsc[n];
            bd[q] = s;
            if (f.bias[q] != (float)s) return fail("b' is not the f32 rounding of the double composition");
        }
        for (int q = 0; q < Q; ++q)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const int px = y * W + x;
                    double ref = ba[q];
                    for (int n = 0; n < N; ++n) {
                        double x12 = x12c[(size_t)n * H * W + px] + (double)bsc[n];
                        for (int k = 0; k < K; ++k) x12 += (double)wsc[(size_t)n * K + k] * (double)cat[(size_t)k * H * W + px];
                        ref += (double)wa[q * N + n] * x12;
                    }
                    double got = bd[q];
                    for (int c = 0; c < C; ++c)
                        for (int ky = 0; ky < 3; ++ky)
                            for (int kx = 0; kx < 3; ++kx) {
                                const int yy = y + ky - 1, xx = x + kx - 1;
                                if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                                got += w2d[(((size_t)q * C + c) * 3 + ky) * 3 + kx] * (double)h[((size_t)c * H + yy) * W + xx];
                            }
                    for (int k = 0; k < K; ++k) got += wscd[(size_t)q * K + k] * (double)cat[(size_t)k * H * W + px];
                    worst = std::fmax(worst, std::fabs(got - ref));
                }
    }
    printf("N=%d C=%d K=%d Q=%d: conv(W2') + Wsc' cat + b' against after_conv(conv(W2) + Wsc cat + bsc), double: max |diff| %.3e of %.3e\n",
           N, C, K, Q, worst, scale);
    if (!(worst <= scale * 1e-12)) return fail("the composition is off by more than 1e-12 relative");

    // ---- the padding: rows Q .. 15 of every image are exactly zero -----------------------------------------------------------
    for (int r = Q; r < kHeadFoldRows; ++r) {
        for (int i = 0; i < C * 9; ++i)
            if (f.w2[(size_t)r * C * 9 + i] != 0.f) return fail("W2' has a non-zero padding row");
        for (int k = 0; k < K; ++k)
            if (f.wsc[(size_t)k * kHeadFoldRows + r] != 0.f) return fail("Wsc' has a non-zero padding row");
        if (f.bias[r] != 0.f) return fail("b' has a non-zero padding row");
        for (int c = 0; c < C; ++c)
            for (int xi = 0; xi < kWino4NXI; ++xi)
                if (f.u[head_fold_u_index(c, xi, r)] != 0.f) return fail("the U image has a non-zero padding row");
    }
    // ---- the U image: every element is addressed exactly once, and a live row is G g G^T of W2' (the centre tap of the 6 x 6
    // domain pins the transform: U[(0,0)] = g[0][0] / 16, U[(5,5)] = g[2][2]) --------------------------------------------------
    std::vector<int> hit(f.u.size(), 0);
    for (int c = 0; c < C; ++c)
        for (int xi = 0; xi < kWino4NXI; ++xi)
            for (int r = 0; r < kHeadFoldRows; ++r) {
                const size_t i = head_fold_u_index(c, xi, r);
                if (i >= f.u.size()) return fail("head_fold_u_index leaves the image");
                ++hit[i];
            }
    for (int v : hit)
        if (v != 1) return fail("head_fold_u_index is not a bijection onto the image");
    for (int q = 0; q < Q; ++q)
        for (int c = 0; c < C; ++c) {
            const float* g = &f.w2[((size_t)q * C + c) * 9];
            if (f.u[head_fold_u_index(c, 0, q)] != (float)((double)g[0] / 16.0) || f.u[head_fold_u_index(c, 35, q)] != g[8])
                return fail("the U image is not G g G^T of W2'");
        }
    // ---- the compact image the kernels copy in: rows 0 .. 3 of the U image, the SAME f32 values (not a second rounding), every
    // live element addressed exactly once, row 3 (and every row >= Q) zero, the tail of each chunk up to whole DMA pieces zero;
    // with more than 3 logits there is no zero row and no compact image ---------------------------------------------------------
    if (Q >= kHeadFoldRows4) {
        if (!f.u4.empty()) return fail("a compact image without a zero row");
        printf("N=%d C=%d K=%d Q=%d: no compact image\n", N, C, K, Q);
        return 0;
    }
    if (f.u4.size() != (size_t)(C / kWino4KC) * kHeadFoldU4Floats) return fail("compact image size");
    std::vector<int> hit4(f.u4.size(), 0);
    size_t same = 0;
    for (int c = 0; c < C; ++c)
        for (int xi = 0; xi < kWino4NXI; ++xi)
            for (int r = 0; r < kHeadFoldRows4; ++r) {
                const size_t i = head_fold_u4_index(c, xi, r), chunk = (size_t)(c / kWino4KC) * kHeadFoldU4Floats;
                if (i < chunk || i >= chunk + kHeadFoldU4Live) return fail("head_fold_u4_index leaves its chunk's live part");
                ++hit4[i];
                if (f.u4[i] != f.u[head_fold_u_index(c, xi, r)]) return fail("the compact image differs from the U image");
                if (r >= Q && f.u4[i] != 0.f) return fail("the compact image has a non-zero padding row");
                ++same;
            }
    for (size_t i = 0; i < f.u4.size(); ++i) {
        const bool live = i % kHeadFoldU4Floats < (size_t)kHeadFoldU4Live;
        if (hit4[i] != (live ? 1 : 0)) return fail("head_fold_u4_index is not a bijection onto the live part");
        if (!live && f.u4[i] != 0.f) return fail("the compact image's tail is not zero");
    }
    printf("N=%d C=%d K=%d Q=%d: compact image: %zu values equal to the U image's rows 0..3, row 3 zero\n", N, C, K, Q, same);
    return 0;
}

}  // namespace

int main() {
    // decoder_block6's own shape (32 -> 3 over 32 + 64 channels), a smaller one, and one with all 16 rows live
    if (check(32, 32, 64, 3) || check(8, 8, 16, 3) || check(8, 16, 8, 16)) return 1;
    // shapes the images cannot hold are refused, not truncated
    HeadFold f;
    const std::vector<float> z(4096, 0.f);
    if (compose_head_fold(z.data(), z.data(), z.data(), z.data(), z.data(), 8, 8, 8, 17, &f)) return fail("17 logits accepted");
    if (compose_head_fold(z.data(), z.data(), z.data(), z.data(), z.data(), 8, 12, 8, 3, &f)) return fail("12 input channels accepted");
    printf("ok\n");
    return 0;
}
