// head_sc_fold_check.cpp - the composition of lass_amd/csrc/head_fold.h for the head_sc_fold route on the CPU: with the composed
// shortcut split at the concat and its up-sampled half folded through the transposed conv,
//      conv(W2') h + Wsc'_skip x1 + Wt' a + b'  ==  after_conv(conv2(h) + shortcut(cat(tconv(a), x1)))
// on random small tensors, in double; Wt' and Wsc'_skip are the f32 rounding of the double composition and Wt' is zero outside its
// live columns.  Host only:
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I lass_amd/csrc tools/head_sc_fold_check.cpp -o tools/bin/head_sc_fold_check
// Prints one line per check and "ok"; exit status 1 on the first failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "head_fold.h"

namespace {

unsigned long long g_state = 0xD1B54A32D192ED03ull;
float rnd() {  // uniform in [-1, 1), 24 bits
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (float)((double)(g_state >> 40) / (double)(1ull << 23) - 1.0);
}
std::vector<float> rnd_vec(size_t n, float scale) {
    std::vector<float> v(n);
    for (auto& x : v) x = rnd() * scale;
    return v;
}

constexpr int H = 8, W = 8, UH = 2, UW = 2, S = UH * UW;  // the full-resolution image; the transposed conv's input is H/2 x W/2

// out[n][y][x] = sum_{c,ky,kx} w[n][c][ky][kx] in[c][y + ky - 1][x + kx - 1], zero padding (cross-correlation, as F.conv2d)
template <typename TW>
std::vector<double> conv3x3(const TW* w, int N, int C, const std::vector<float>& in) {
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

// N: channels of the block, Cup / Cskip: the two halves of the concat, Kt: input channels of the transposed conv, Q: logits
int check(int N, int Cup, int Cskip, int Kt, int Q) {
    const int C = N, K = Cup + Cskip;
    const std::vector<float> w2 = rnd_vec((size_t)N * C * 9, 0.2f), wsc = rnd_vec((size_t)N * K, 0.3f), bsc = rnd_vec(N, 0.5f);
    const std::vector<float> wa = rnd_vec((size_t)Q * N, 0.4f), ba = rnd_vec(Q, 0.5f), wt = rnd_vec((size_t)Kt * Cup * S, 0.3f);
    const std::vector<float> h = rnd_vec((size_t)C * H * W, 1.f), x1 = rnd_vec((size_t)Cskip * H * W, 1.f);
    const std::vector<float> a = rnd_vec((size_t)Kt * (H / UH) * (W / UW), 1.f);
    HeadFold f;
    HeadScFold g;
    if (!compose_head_fold(w2.data(), wsc.data(), bsc.data(), wa.data(), ba.data(), N, C, K, Q, &f)) return fail("compose_head_fold refused the shape");
    if (!compose_head_sc_fold(wsc.data(), wa.data(), wt.data(), N, Cup, Cskip, Q, Kt, UH, UW, &g)) return fail("compose_head_sc_fold refused the shape");
    if (g.wt.size() != (size_t)Kt * kHeadScCols || g.wskip.size() != (size_t)Q * Cskip) return fail("image sizes");

    // ---- the reference: up = tconv(a) (kernel == stride, no bias), cat = (up, x1), after_conv(conv2(h) + Wsc cat + bsc) + ba ---
    std::vector<double> cat((size_t)K * H * W, 0.0);
    for (int c = 0; c < Cup; ++c)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                double s = 0;
                for (int k = 0; k < Kt; ++k)
                    s += (double)a[((size_t)k * (H / UH) + y / UH) * (W / UW) + x / UW] * (double)wt[((size_t)k * Cup + c) * S + (y % UH) * UW + x % UW];
                cat[((size_t)c * H + y) * W + x] = s;
            }
    for (size_t i = 0; i < x1.size(); ++i) cat[(size_t)Cup * H * W + i] = x1[i];
    const std::vector<double> x12c = conv3x3(w2.data(), N, C, h);
    std::vector<double> ref((size_t)Q * H * W);
    double scale = 0;
    for (int q = 0; q < Q; ++q)
        for (int px = 0; px < H * W; ++px) {
            double r = ba[q];
            for (int n = 0; n < N; ++n) {
                double x12 = x12c[(size_t)n * H * W + px] + (double)bsc[n];
                for (int k = 0; k < K; ++k) x12 += (double)wsc[(size_t)n * K + k] * cat[(size_t)k * H * W + px];
                r += (double)wa[q * N + n] * x12;
            }
            ref[(size_t)q * H * W + px] = r;
            scale = std::fmax(scale, std::fabs(r));
        }

    // ---- the composition in double, recomputed here; the images hold exactly its f32 rounding -------------------------------------
    std::vector<double> w2d((size_t)Q * C * 9), wq((size_t)Q * K), wtd((size_t)Kt * Q * S), bd(Q);
    for (int q = 0; q < Q; ++q) {
        for (int i = 0; i < C * 9; ++i) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)w2[(size_t)n * C * 9 + i];
            w2d[(size_t)q * C * 9 + i] = s;
        }
        for (int k = 0; k < K; ++k) {
            double s = 0;
            for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)wsc[(size_t)n * K + k];
            wq[(size_t)q * K + k] = s;
        }
        for (int c = 0; c < Cskip; ++c)
            if (g.wskip[(size_t)q * Cskip + c] != (float)wq[(size_t)q * K + Cup + c]) return fail("Wsc'_skip is not the f32 rounding of the double composition");
        for (int k = 0; k < Kt; ++k)
            for (int s = 0; s < S; ++s) {
                double t = 0;
                for (int c = 0; c < Cup; ++c) t += wq[(size_t)q * K + c] * (double)wt[((size_t)k * Cup + c) * S + s];
                wtd[((size_t)k * Q + q) * S + s] = t;
                if (g.wt[(size_t)k * kHeadScCols + q * S + s] != (float)t) return fail("Wt' is not the f32 rounding of the double composition");
            }
        double s = ba[q];
        for (int n = 0; n < N; ++n) s += (double)wa[q * N + n] * (double)bsc[n];
        bd[q] = s;
    }
    // got = conv(W2') h + Wsc'_skip x1 + Wt' a + b': once from the double composition (the algebra), once from the f32 images
    const std::vector<double> cd = conv3x3(w2d.data(), Q, C, h), cf = conv3x3(f.w2.data(), kHeadFoldRows, C, h);
    double worst = 0, worst32 = 0;
    for (int q = 0; q < Q; ++q)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                const int px = y * W + x, s = (y % UH) * UW + x % UW;
                const size_t lo = (size_t)(y / UH) * (W / UW) + x / UW;
                double got = cd[(size_t)q * H * W + px] + bd[q], got32 = cf[(size_t)q * H * W + px] + (double)f.bias[q];
                for (int c = 0; c < Cskip; ++c) {
                    got += wq[(size_t)q * K + Cup + c] * (double)x1[(size_t)c * H * W + px];
                    got32 += (double)g.wskip[(size_t)q * Cskip + c] * (double)x1[(size_t)c * H * W + px];
                }
                for (int k = 0; k < Kt; ++k) {
                    got += wtd[((size_t)k * Q + q) * S + s] * (double)a[(size_t)k * (H / UH) * (W / UW) + lo];
                    got32 += (double)g.wt[(size_t)k * kHeadScCols + q * S + s] * (double)a[(size_t)k * (H / UH) * (W / UW) + lo];
                }
                worst = std::fmax(worst, std::fabs(got - ref[(size_t)q * H * W + px]));
                worst32 = std::fmax(worst32, std::fabs(got32 - ref[(size_t)q * H * W + px]));
            }
    printf("N=%d Cup=%d Cskip=%d Kt=%d Q=%d: conv(W2') h + Wsc'_skip x1 + Wt' a + b' against after_conv(conv2(h) + shortcut(cat(tconv(a), x1))), "
           "double: max |diff| %.3e of %.3e (relative %.3e)\n", N, Cup, Cskip, Kt, Q, worst, scale, worst / scale);
    if (!(worst <= scale * 1e-12)) return fail("the composition is off by more than 1e-12 relative");
    printf("N=%d Cup=%d Cskip=%d Kt=%d Q=%d: the f32-rounded images against the reference: max |diff| %.3e of %.3e\n", N, Cup, Cskip, Kt, Q, worst32, scale);
    if (!(worst32 <= scale * 2e-6)) return fail("the rounded images are off by more than f32 rounding of the weights");

    // ---- the padding: every column of Wt' from Q * S on is exactly zero -----------------------------------------------------------
    for (int k = 0; k < Kt; ++k)
        for (int n = Q * S; n < kHeadScCols; ++n)
            if (g.wt[(size_t)k * kHeadScCols + n] != 0.f) return fail("Wt' has a non-zero padding column");
    return 0;
}

}  // namespace

int main() {
    // decoder_block6's own shape (32 channels, cat = 32 + 32, transposed conv from 64 channels, 3 logits), a smaller one, and one
    // with every live column of the tile in use (8 logits x 4 sub-pixels)
    if (check(32, 32, 32, 64, 3) || check(8, 8, 16, 16, 3) || check(8, 16, 8, 8, 8)) return 1;
    // shapes the extra block cannot hold are refused, not truncated
    HeadScFold g;
    const std::vector<float> z(4096, 0.f);
    if (compose_head_sc_fold(z.data(), z.data(), z.data(), 8, 8, 8, 9, 8, 2, 2, &g)) return fail("9 logits x 4 sub-pixels accepted");
    if (compose_head_sc_fold(z.data(), z.data(), z.data(), 8, 8, 0, 3, 8, 2, 2, &g)) return fail("an empty skip accepted");
    printf("ok\n");
    return 0;
}
