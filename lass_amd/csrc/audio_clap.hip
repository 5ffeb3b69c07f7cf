// audio_clap.hip - the CLAP audio tower on the device: 32 -> 48 kHz resampler, repeat-pad + log-mel front end, HTSAT (a Swin
// transformer over the 256 x 256 fold of the spectrogram, CLAP/open_clip/htsat.py:1012-1149) + audio projection + L2
// normalisation (CLAP/open_clip/model.py:566-570, 754-781), behind its own lass_audioq_ctx.  f32 throughout; every
// contraction of the tower runs on v_mfma_f32_32x32x2_f32 (the GEMM of tower_parts.h, shared with text.hip, and the two
// products of the window attention).
//
// Batch invariance: every kernel computes a frame, a token row, a window or a clip from that unit's inputs alone in a fixed
// order - one GEMM tile shape for every M, per-row reductions, no atomics - so a clip's embedding is bit-identical whatever
// batch or position it comes with.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/lass_hip.h"
#include "ctx_parts.h"

namespace {

#include "tower_parts.h"

constexpr int kClip = 480000, kFft = 1024, kHop = 480, kFrames = 1001, kBins = 513, kMel = 64, kMelTaps = 32;
constexpr int kGrid = 64, kWin = 8, kTok = 64, kDh = 32, kEmbed = 128, kMaxStages = 4;
constexpr int kMax32k = 320000, kRsTaps = 16;
constexpr double kBnEps = 1e-5;

// ---- resampler: y[3i + p] = sum_k taps[p][k] x[2i + k - 7], zero outside the clip; rows past a clip's end are zero -------
__global__ __launch_bounds__(256) void k_resample32(const float* __restrict__ x, int L32, const int* __restrict__ len32,
                                                    const float* __restrict__ taps, float* __restrict__ y, int L48) {
    const int b = blockIdx.y, o = blockIdx.x * 256 + threadIdx.x;
    if (o >= L48) return;
    const int len = len32[b];
    float acc = 0.f;
    if (o < (3 * len + 1) / 2) {
        const int i = o / 3, p = o - 3 * i;
        const float* xr = x + (size_t)b * L32;
#pragma unroll
        for (int k = 0; k < kRsTaps; ++k) {
            const int j = 2 * i + k - 7;
            const float v = (j >= 0 && j < len) ? xr[j] : 0.f;
            acc = fmaf(taps[p * kRsTaps + k], v, acc);
        }
    }
    y[(size_t)b * L48 + o] = acc;
}

// ---- front end: one frame of one clip per workgroup -----------------------------------------------------------------------
// The 480 000-sample repeat-padded clip is never materialised: sample j of it is x[j % len] for j < (480000 / len) * len,
// else 0, and the reflect padding of 512 is an index map in front of that.  Periodic Hann, 1024-point radix-2 FFT in LDS
// (twiddles from the host's float64), power, 64 slaney bands as (start, count, weights) runs, 10 log10(max(p, 1e-10)), bn0
// as scale / base.  A band at or below the floor is exactly -100 dB.
__global__ __launch_bounds__(256) void k_logmel(const float* __restrict__ wave, int stride, const int* __restrict__ lens,
                                                const float* __restrict__ win, const float2* __restrict__ tw,
                                                const int* __restrict__ mstart, const int* __restrict__ mcount,
                                                const float* __restrict__ mw, const float* __restrict__ bscale,
                                                const float* __restrict__ bbase, float* __restrict__ out) {
    __shared__ float re[kFft], im[kFft], pw[kBins + 7];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int len = lens[b];
    const int lim = (kClip / len) * len;
    const float* x = wave + (size_t)b * stride;
    for (int n = tid; n < kFft; n += 256) {
        int j = kHop * t + n - kFft / 2;
        j = j < 0 ? -j : (j >= kClip ? 2 * (kClip - 1) - j : j);
        const float v = j < lim ? x[j % len] : 0.f;
        const int r = (int)(__brev((unsigned)n) >> 22);
        re[r] = v * win[n];
        im[r] = 0.f;
    }
    __syncthreads();
    for (int half = 1; half < kFft; half <<= 1) {
        for (int k = tid; k < kFft / 2; k += 256) {
            const int pos = k & (half - 1);
            const int i0 = ((k - pos) << 1) + pos, i1 = i0 + half;
            const float2 w = tw[pos * (kFft / 2 / half)];
            const float ar = re[i1], ai = im[i1];
            const float pr = ar * w.x - ai * w.y, pi = ar * w.y + ai * w.x;
            const float ur = re[i0], ui = im[i0];
            re[i0] = ur + pr;
            im[i0] = ui + pi;
            re[i1] = ur - pr;
            im[i1] = ui - pi;
        }
        __syncthreads();
    }
    for (int k = tid; k < kBins; k += 256) pw[k] = re[k] * re[k] + im[k] * im[k];
    __syncthreads();
    if (tid < kMel) {
        const int s = mstart[tid], c = mcount[tid];
        float p = 0.f;
        for (int k = 0; k < c; ++k) p = fmaf(mw[tid * kMelTaps + k], pw[s + k], p);
        const float db = p > 1e-10f ? 10.0f * log10f(p) : -100.0f;
        {   // product and sum rounded separately (no fused multiply-add), so a floor band is exactly -100 * scale + base
#pragma clang fp contract(off)
            const float scaled = db * bscale[tid];
            out[((size_t)b * kFrames + t) * kMel + tid] = scaled + bbase[tid];
        }
    }
}

// ---- image + patch embedding: one wave per token ---------------------------------------------------------------------------
// Token (i, j) of the 64 x 64 grid covers image rows 4i .. 4i+3, columns 4j .. 4j+3; image row R = 64 q + f is mel bin f of
// time chunk q, image column c is frame 256 q + c of the 1024-frame axis, itself the bicubic (A = -0.75, align_corners)
// resampling of the 1001 log-mel frames (4 clamped source frames and weights per target frame, tabulated by the host).
// Lanes 0..15 gather one pixel each; every lane then convolves two output channels and the wave normalises the row.
__global__ __launch_bounds__(256) void k_patch_embed(const float* __restrict__ logmel, const int4* __restrict__ bidx,
                                                     const float4* __restrict__ bw, const float* __restrict__ w,
                                                     const float* __restrict__ bias, const float* __restrict__ g,
                                                     const float* __restrict__ beta, float* __restrict__ tok, int rows) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = r / (kGrid * kGrid), i = (r / kGrid) % kGrid, j = r % kGrid;
    float pix = 0.f;
    if (lane < 16) {
        const int R = 4 * i + (lane >> 2), c = 4 * j + (lane & 3);
        const int q = R >> 6, f = R & 63, t = 256 * q + c;
        const int4 ix = bidx[t];
        const float4 cw = bw[t];
        const float* m = logmel + (size_t)b * kFrames * kMel + f;
        pix = ((cw.x * m[ix.x * kMel] + cw.y * m[ix.y * kMel]) + cw.z * m[ix.z * kMel]) + cw.w * m[ix.w * kMel];
    }
    float x[2] = {bias[lane], bias[lane + 64]};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float p = __shfl(pix, k);
        x[0] = fmaf(w[lane * 16 + k], p, x[0]);
        x[1] = fmaf(w[(lane + 64) * 16 + k], p, x[1]);
    }
    ln_row<2>(x, g, beta, tok + (size_t)r * kEmbed, lane);
}

template <int NPL>  // y = LayerNorm(x) for M rows of 64 * NPL
__global__ __launch_bounds__(256) void k_ln(const float* __restrict__ x, float* __restrict__ y, int M,
                                            const float* __restrict__ g, const float* __restrict__ b) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    float v[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) v[j] = x[(size_t)r * (64 * NPL) + lane + 64 * j];
    ln_row<NPL>(v, g, b, y + (size_t)r * (64 * NPL), lane);
}

// PatchMerging's gather + LayerNorm(4C): output row (b, i, j) of the res/2 grid is [x(2i,2j) | x(2i+1,2j) | x(2i,2j+1) |
// x(2i+1,2j+1)], C = 16 * NPL each.
template <int NPL>
__global__ __launch_bounds__(256) void k_merge_ln(const float* __restrict__ x, float* __restrict__ y, int M, int res,
                                                  const float* __restrict__ g, const float* __restrict__ b) {
    constexpr int C = 16 * NPL;
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int h = res / 2;
    const int n = r / (h * h), i = (r / h) % h, j = r % h;
    float v[NPL];
#pragma unroll
    for (int u = 0; u < NPL; ++u) {
        const int k = lane + 64 * u;
        const int seg = k / C, c = k % C;
        const int si = 2 * i + (seg & 1), sj = 2 * j + (seg >> 1);
        v[u] = x[((size_t)n * res * res + (size_t)si * res + sj) * C + c];
    }
    ln_row<NPL>(v, g, b, y + (size_t)r * (4 * C), lane);
}

// ---- window attention: one wave per (window, head, clip) -----------------------------------------------------------------
// 64 tokens x head dim 32.  The cyclic shift and the window partition are address arithmetic: token t of window (wi, wj)
// sits at shifted coordinates (8 wi + t / 8, 8 wj + t % 8), i.e. at ((.. + shift) % res, (.. + shift) % res) of the grid,
// and its result goes back there.  S = (q * 32^-1/2) k^T is four 32x32x32 MFMA products; the relative-position bias
// (table row (ri - rj + 7) * 15 + (ci - cj + 7)) and, in shifted blocks, the -100 mask between tokens from different sides
// of the wrap-around are added as S goes to LDS; lane r then holds row r for the softmax, writes P back, and P is the A
// operand of the 64x32x64 product with V.
constexpr int QS = kDh + 1, PS = kTok + 1;
__global__ __launch_bounds__(64) void k_win_attn(const float* __restrict__ qkv, const float* __restrict__ table, int heads,
                                                 int res, int shift, float* __restrict__ out) {
    __shared__ float Qs[kTok * QS], Ks[kTok * QS], Vs[kTok * QS], Ps[kTok * PS], Bt[232];
    __shared__ int pos[kTok], reg[kTok];
    const int lane = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int nw = res / kWin, wi = blockIdx.x / nw, wj = blockIdx.x % nw;
    const int C = heads * kDh;
    {
        const int hs = wi * kWin + (lane >> 3), ws = wj * kWin + (lane & 7);
        pos[lane] = ((hs + shift) % res) * res + (ws + shift) % res;
        const int rh = (hs >= res - kWin) + (hs >= res - shift), rw = (ws >= res - kWin) + (ws >= res - shift);
        reg[lane] = shift ? rh * 3 + rw : 0;
    }
    for (int k = lane; k < 225; k += 64) Bt[k] = table[k * heads + h];
    __syncthreads();
    const float scale = 0.17677669529663687f;  // 32^-1/2
    const float* base = qkv + (size_t)b * res * res * 3 * C + h * kDh;
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int t = pass * 8 + (lane >> 3), c = (lane & 7) * 4;
        const float* p = base + (size_t)pos[t] * 3 * C + c;
        const float4 q = *(const float4*)p, k = *(const float4*)(p + C), v = *(const float4*)(p + 2 * C);
        float* d = Qs + t * QS + c;
        d[0] = q.x * scale; d[1] = q.y * scale; d[2] = q.z * scale; d[3] = q.w * scale;
        d = Ks + t * QS + c;
        d[0] = k.x; d[1] = k.y; d[2] = k.z; d[3] = k.w;
        d = Vs + t * QS + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
    __syncthreads();
    const int l31 = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int kk = 0; kk < kDh / 2; ++kk)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Qs[(mi * 32 + l31) * QS + 2 * kk + kh],
                                                           Ks[(ni * 32 + l31) * QS + 2 * kk + kh], acc, 0, 0, 0);
            const int j = ni * 32 + l31;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
                const int rel = ((r >> 3) - (j >> 3) + kWin - 1) * (2 * kWin - 1) + ((r & 7) - (j & 7) + kWin - 1);
                float s = acc[i] + Bt[rel];
                if (shift) s += reg[r] != reg[j] ? -100.0f : 0.0f;
                Ps[r * PS + j] = s;
            }
        }
    }
    __syncthreads();
    {
        float* row = Ps + lane * PS;
        float m = row[0];
        for (int j = 1; j < kTok; ++j) m = fmaxf(m, row[j]);
        float sum = 0.f;
        for (int j = 0; j < kTok; ++j) {
            const float e = expf(row[j] - m);
            row[j] = e;
            sum += e;
        }
        for (int j = 0; j < kTok; ++j) row[j] = row[j] / sum;
    }
    __syncthreads();
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
        for (int kk = 0; kk < kTok / 2; ++kk)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ps[(mi * 32 + l31) * PS + 2 * kk + kh], Vs[(2 * kk + kh) * QS + l31],
                                                       acc, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = mi * 32 + (i & 3) + 8 * (i >> 2) + 4 * kh;
            out[((size_t)b * res * res + pos[r]) * C + h * kDh + l31] = acc[i];
        }
    }
}

// "embedding": mean over the T tokens of a clip, channel by channel, in token order.
__global__ __launch_bounds__(256) void k_token_mean(const float* __restrict__ x, int T, int C, float* __restrict__ y) {
    const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += x[((size_t)b * T + t) * C + c];
    y[(size_t)b * C + c] = s / (float)T;
}

struct ABlock {
    const float *g1, *b1, *table, *wqkv, *bqkv, *wo, *bo, *g2, *b2, *w1, *bb1, *w2, *bb2;
};

struct AStage {
    std::vector<ABlock> blocks;
    const float *red = nullptr, *mg = nullptr, *mb = nullptr;  // PatchMerging (absent after the last stage)
};

// device constants built by lass_audioq_finalize, one allocation
struct AConst {
    float *taps, *win, *mw, *bscale, *bbase, *zero;
    float2* tw;
    int *mstart, *mcount;
    int4* bidx;
    float4* bw;
};

thread_local std::string g_audioq_create_err;

const char* kBlockKeys[] = {"norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.qkv.weight", "attn.qkv.bias",
                            "attn.proj.weight", "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias",
                            "mlp.fc2.weight", "mlp.fc2.bias"};
const char* kMergeKeys[] = {"reduction.weight", "norm.weight", "norm.bias"};
const char* kFixedKeys[] = {"audio_branch.bn0.weight", "audio_branch.bn0.bias", "audio_branch.bn0.running_mean",
                            "audio_branch.bn0.running_var", "audio_branch.patch_embed.proj.weight",
                            "audio_branch.patch_embed.proj.bias", "audio_branch.patch_embed.norm.weight",
                            "audio_branch.patch_embed.norm.bias", "audio_branch.norm.weight", "audio_branch.norm.bias",
                            "audio_projection.0.weight", "audio_projection.0.bias", "audio_projection.2.weight",
                            "audio_projection.2.bias"};
const char* kLayers = "audio_branch.layers.";

// Is `name` a parameter the kernels read?  (layers.<i>.blocks.<j>.<block key>, layers.<i>.downsample.<merge key>, fixed keys)
bool known_key(const std::string& name) {
    for (const char* k : kFixedKeys)
        if (name == k) return true;
    if (name.rfind(kLayers, 0) != 0) return false;
    int i = -1, j = -1, used = 0;
    const char* rest = name.c_str() + strlen(kLayers);
    if (sscanf(rest, "%d.blocks.%d.%n", &i, &j, &used) == 2 && used > 0 && i >= 0 && i < kMaxStages && j >= 0) {
        for (const char* k : kBlockKeys)
            if (strcmp(rest + used, k) == 0) return true;
        return false;
    }
    used = 0;
    if (sscanf(rest, "%d.downsample.%n", &i, &used) == 1 && used > 0 && i >= 0 && i < kMaxStages - 1)
        for (const char* k : kMergeKeys)
            if (strcmp(rest + used, k) == 0) return true;
    return false;
}

}  // namespace

struct lass_audioq_ctx {
    int device = 0;
    std::string err;
    ParamStore raw;
    bool finalized = false;
    std::vector<AStage> stages;
    int features = 0;
    void* consts = nullptr;
    AConst K{};
    PinnedInts len;  // staging of the clip lengths and their 48 kHz lengths (2 B ints)
};

namespace {

void layer_norm(const float* x, float* y, int M, int C, const float* g, const float* b, hipStream_t st) {
    const dim3 grid((M + 3) / 4), blk(256);
    switch (C / 64) {
        case 2: hipLaunchKernelGGL(k_ln<2>, grid, blk, 0, st, x, y, M, g, b); break;
        case 4: hipLaunchKernelGGL(k_ln<4>, grid, blk, 0, st, x, y, M, g, b); break;
        case 8: hipLaunchKernelGGL(k_ln<8>, grid, blk, 0, st, x, y, M, g, b); break;
        default: hipLaunchKernelGGL(k_ln<16>, grid, blk, 0, st, x, y, M, g, b); break;
    }
}

void merge_ln(const float* x, float* y, int M, int res, int C, const float* g, const float* b, hipStream_t st) {
    const dim3 grid((M + 3) / 4), blk(256);
    switch (C / 16) {
        case 8: hipLaunchKernelGGL(k_merge_ln<8>, grid, blk, 0, st, x, y, M, res, g, b); break;
        case 16: hipLaunchKernelGGL(k_merge_ln<16>, grid, blk, 0, st, x, y, M, res, g, b); break;
        default: hipLaunchKernelGGL(k_merge_ln<32>, grid, blk, 0, st, x, y, M, res, g, b); break;
    }
}

struct APlan {  // workspace carve-up for B clips
    size_t lens, wave48, logmel, x, ln, qkv, attn, ffn, emb, p1, p2, total;
};

APlan audio_plan(int B) {
    const size_t rows = (size_t)B * kGrid * kGrid;
    APlan p;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.lens = take(2 * (size_t)B * sizeof(int));  // the clips' lengths, then their 48 kHz lengths ceil(1.5 len)
    p.wave48 = take((size_t)B * kClip * sizeof(float));
    p.logmel = take((size_t)B * kFrames * kMel * sizeof(float));
    p.x = take(rows * kEmbed * sizeof(float));
    p.ln = take(rows * kEmbed * sizeof(float));
    p.qkv = take(rows * 3 * kEmbed * sizeof(float));
    p.attn = take(rows * kEmbed * sizeof(float));
    p.ffn = take(rows * 4 * kEmbed * sizeof(float));
    p.emb = take((size_t)B * kEmbed * 8 * sizeof(float));
    p.p1 = take((size_t)B * kProj * sizeof(float));
    p.p2 = take((size_t)B * kProj * sizeof(float));
    p.total = o;
    return p;
}

double cubic1(double x, double A) { return ((A + 2) * x - (A + 3)) * x * x + 1; }
double cubic2(double x, double A) { return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A; }
double hz_to_mel(double f) { return f >= 1000.0 ? 15.0 + std::log(f / 1000.0) * (27.0 / std::log(6.4)) : 3.0 * f / 200.0; }
double mel_to_hz(double m) { return m >= 15.0 ? 1000.0 * std::exp(std::log(6.4) / 27.0 * (m - 15.0)) : 200.0 * m / 3.0; }

// Everything from the 48 kHz waveform on.  wave rows are `stride` apart; d_len holds the clips' lengths on the device.
int encode48(lass_audioq_ctx* c, const float* wave, int stride, const int* d_len, int B, float* out,
             const lass_audioq_taps* taps, char* ws, const APlan& P, hipStream_t st) {
    const AConst& K = c->K;
    auto tp = [&](const char* k) { return c->raw.get(k); };
    float* logmel = (float*)(ws + P.logmel);
    float* x = (float*)(ws + P.x);
    float* ln = (float*)(ws + P.ln);
    float* qkv = (float*)(ws + P.qkv);
    float* attn = (float*)(ws + P.attn);
    float* ffn = (float*)(ws + P.ffn);
    hipLaunchKernelGGL(k_logmel, dim3(kFrames, B), dim3(256), 0, st, wave, stride, d_len, K.win, K.tw, K.mstart, K.mcount, K.mw,
                       K.bscale, K.bbase, logmel);
    int rows = B * kGrid * kGrid;
    hipLaunchKernelGGL(k_patch_embed, dim3((rows + 3) / 4), dim3(256), 0, st, logmel, K.bidx, K.bw,
                       tp("audio_branch.patch_embed.proj.weight"), tp("audio_branch.patch_embed.proj.bias"),
                       tp("audio_branch.patch_embed.norm.weight"), tp("audio_branch.patch_embed.norm.bias"), x, rows);
    if (taps && taps->logmel)
        HIP_TRY(c, hipMemcpyAsync(taps->logmel, logmel, (size_t)B * kFrames * kMel * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (taps && taps->tokens)
        HIP_TRY(c, hipMemcpyAsync(taps->tokens, x, (size_t)rows * kEmbed * sizeof(float), hipMemcpyDeviceToDevice, st));
    int res = kGrid, C = kEmbed;
    for (size_t si = 0; si < c->stages.size(); ++si) {
        const AStage& S = c->stages[si];
        const int heads = C / kDh;
        rows = B * res * res;
        for (size_t bi = 0; bi < S.blocks.size(); ++bi) {
            const ABlock& L = S.blocks[bi];
            const int shift = (bi % 2 == 1 && res > kWin) ? kWin / 2 : 0;
            layer_norm(x, ln, rows, C, L.g1, L.b1, st);
            gemm<EPI_BIAS>(ln, L.wqkv, L.bqkv, qkv, rows, 3 * C, C, st);
            hipLaunchKernelGGL(k_win_attn, dim3((res / kWin) * (res / kWin), heads, B), dim3(64), 0, st, qkv, L.table, heads, res,
                               shift, attn);
            gemm<EPI_RESID>(attn, L.wo, L.bo, x, rows, C, C, st);
            layer_norm(x, ln, rows, C, L.g2, L.b2, st);
            gemm<EPI_GELU>(ln, L.w1, L.bb1, ffn, rows, 4 * C, C, st);
            gemm<EPI_RESID>(ffn, L.w2, L.bb2, x, rows, C, 4 * C, st);
        }
        if (S.red) {
            rows /= 4;
            merge_ln(x, ln, rows, res, C, S.mg, S.mb, st);
            gemm<EPI_BIAS>(ln, S.red, K.zero, x, rows, 2 * C, 4 * C, st);
            res /= 2;
            C *= 2;
        }
        if (taps && taps->stage[si])
            HIP_TRY(c, hipMemcpyAsync(taps->stage[si], x, (size_t)rows * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    float* emb = taps && taps->embedding ? taps->embedding : (float*)(ws + P.emb);
    float* p1 = (float*)(ws + P.p1);
    float* p2 = (float*)(ws + P.p2);
    layer_norm(x, ln, rows, C, tp("audio_branch.norm.weight"), tp("audio_branch.norm.bias"), st);
    hipLaunchKernelGGL(k_token_mean, dim3((C + 255) / 256, B), dim3(256), 0, st, ln, res * res, C, emb);
    gemm<EPI_RELU>(emb, tp("audio_projection.0.weight"), tp("audio_projection.0.bias"), p1, B, kProj, C, st);
    gemm<EPI_BIAS>(p1, tp("audio_projection.2.weight"), tp("audio_projection.2.bias"), p2, B, kProj, kProj, st);
    hipLaunchKernelGGL(k_l2norm, dim3((B + 3) / 4), dim3(256), 0, st, p2, B, out);
    HIP_TRY(c, hipGetLastError());
    return LASS_OK;
}

// Argument checks shared by the two entry points, then the lengths' upload.  Nothing is launched before they pass.
int begin_encode(lass_audioq_ctx* c, const char* what, const float* wave, const int* lengths, int B, int L, int maxL, float* out,
                 void* ws, size_t ws_bytes, hipStream_t st, int** d_len) {
    const std::string w(what);
    if (!c->finalized) return fail(c, LASS_ERR_STATE, "lass_audioq_finalize has not been called (or a parameter changed since)");
    if (!wave || !out || !ws) return fail(c, LASS_ERR_ARG, w + ": wave, out and workspace must be non-NULL");
    if (B < 1) return fail(c, LASS_ERR_ARG, w + ": B must be >= 1");
    if (L < 1 || L > maxL) return fail(c, LASS_ERR_ARG, w + ": clips hold 1 .. " + std::to_string(maxL) + " samples (10 s)");
    if (lengths)
        for (int n = 0; n < B; ++n)
            if (lengths[n] < 1 || lengths[n] > L) return fail(c, LASS_ERR_ARG, w + ": lengths must lie in [1, L]");
    const APlan P = audio_plan(B);
    if (ws_bytes < P.total) return fail(c, LASS_ERR_ARG, w + ": workspace too small (lass_audioq_workspace_bytes)");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = c->len.reserve(c, 2 * (size_t)B)) return rc;
    int* len = c->len.host;
    for (int n = 0; n < B; ++n) {
        len[n] = lengths ? lengths[n] : L;
        len[B + n] = (3 * len[n] + 1) / 2;
    }
    *d_len = (int*)((char*)ws + P.lens);
    HIP_TRY(c, hipMemcpyAsync(*d_len, len, 2 * (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    return c->len.record(c, st);
}

}  // namespace

extern "C" {

int lass_audioq_create(lass_audioq_ctx** out, int device_id) {
    if (!out) return LASS_ERR_ARG;
    *out = nullptr;
    if (int rc = open_device(device_id, g_audioq_create_err)) return rc;
    lass_audioq_ctx* c = new lass_audioq_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || c->len.create() != hipSuccess) {
        g_audioq_create_err = "hipSetDevice / hipEventCreate failed";
        delete c;
        return LASS_ERR_HIP;
    }
    *out = c;
    return LASS_OK;
}

int lass_audioq_destroy(lass_audioq_ctx* c) {
    if (!c) return LASS_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->raw.free_all();
    if (c->consts) (void)hipFree(c->consts);
    c->len.destroy();
    delete c;
    return LASS_OK;
}

const char* lass_audioq_last_error(const lass_audioq_ctx* c) { return c ? c->err.c_str() : g_audioq_create_err.c_str(); }

int lass_audioq_set_param(lass_audioq_ctx* c, const char* name, const void* data, const int64_t* shape, int ndim) {
    if (!c) return LASS_ERR_ARG;
    if (!name || !data || !shape || ndim < 1 || ndim > 4) return fail(c, LASS_ERR_ARG, "lass_audioq_set_param: bad arguments");
    if (!known_key(name)) return fail(c, LASS_ERR_ARG, std::string("unknown audio-tower parameter '") + name + "'");
    for (int i = 0; i < ndim; ++i)
        if (shape[i] < 1) return fail(c, LASS_ERR_ARG, std::string(name) + ": empty dimension");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = c->raw.put(c, name, data, shape, ndim)) return rc;
    c->finalized = false;
    return LASS_OK;
}

int lass_audioq_finalize(lass_audioq_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    c->stages.clear();
    c->finalized = false;
    std::string bad;
    // a present key with the expected shape, or nullptr with `bad` set
    auto need = [&](const std::string& k, std::vector<int64_t> shape) -> const float* {
        const Param* p = c->raw.find(k);
        if (!p) {
            if (bad.empty()) bad = "missing parameter " + k;
            return nullptr;
        }
        if (p->shape != shape) {
            std::string s;
            for (int64_t d : shape) s += (s.empty() ? "" : ", ") + std::to_string(d);
            if (bad.empty()) bad = k + ": expected shape (" + s + ")";
            return nullptr;
        }
        return p->d;
    };
    int nstage = 0;
    std::vector<int> depth(kMaxStages, 0);
    for (const auto& kv : c->raw.by_name) {
        int i = -1, j = -1;
        if (kv.first.rfind(kLayers, 0) == 0 && sscanf(kv.first.c_str() + strlen(kLayers), "%d.blocks.%d.", &i, &j) == 2) {
            nstage = std::max(nstage, i + 1);
            depth[i] = std::max(depth[i], j + 1);
        }
    }
    if (nstage < 1) return fail(c, LASS_ERR_STATE, "no block parameters (audio_branch.layers.<i>.blocks.<j>.*)");
    int C = kEmbed;
    for (int i = 0; i < nstage; ++i, C *= 2) {
        if (depth[i] < 1) return fail(c, LASS_ERR_STATE, "missing parameter audio_branch.layers." + std::to_string(i) + ".blocks.0.*");
        AStage S;
        const int heads = C / kDh;
        for (int j = 0; j < depth[i]; ++j) {
            const std::string p = kLayers + std::to_string(i) + ".blocks." + std::to_string(j) + ".";
            ABlock L;
            L.g1 = need(p + "norm1.weight", {C});
            L.b1 = need(p + "norm1.bias", {C});
            L.table = need(p + "attn.relative_position_bias_table", {225, heads});
            L.wqkv = need(p + "attn.qkv.weight", {3 * C, C});
            L.bqkv = need(p + "attn.qkv.bias", {3 * C});
            L.wo = need(p + "attn.proj.weight", {C, C});
            L.bo = need(p + "attn.proj.bias", {C});
            L.g2 = need(p + "norm2.weight", {C});
            L.b2 = need(p + "norm2.bias", {C});
            L.w1 = need(p + "mlp.fc1.weight", {4 * C, C});
            L.bb1 = need(p + "mlp.fc1.bias", {4 * C});
            L.w2 = need(p + "mlp.fc2.weight", {C, 4 * C});
            L.bb2 = need(p + "mlp.fc2.bias", {C});
            S.blocks.push_back(L);
        }
        if (i < nstage - 1) {
            const std::string p = kLayers + std::to_string(i) + ".downsample.";
            S.red = need(p + "reduction.weight", {2 * C, 4 * C});
            S.mg = need(p + "norm.weight", {4 * C});
            S.mb = need(p + "norm.bias", {4 * C});
        }
        c->stages.push_back(S);
    }
    const int F = kEmbed << (nstage - 1);
    for (const char* k : {"weight", "bias", "running_mean", "running_var"}) need(std::string("audio_branch.bn0.") + k, {kMel});
    need("audio_branch.patch_embed.proj.weight", {kEmbed, 1, 4, 4});
    need("audio_branch.patch_embed.proj.bias", {kEmbed});
    need("audio_branch.patch_embed.norm.weight", {kEmbed});
    need("audio_branch.patch_embed.norm.bias", {kEmbed});
    need("audio_branch.norm.weight", {F});
    need("audio_branch.norm.bias", {F});
    need("audio_projection.0.weight", {kProj, F});
    need("audio_projection.0.bias", {kProj});
    need("audio_projection.2.weight", {kProj, kProj});
    need("audio_projection.2.bias", {kProj});
    if (!bad.empty()) {
        c->stages.clear();
        return fail(c, bad.rfind("missing", 0) == 0 ? LASS_ERR_STATE : LASS_ERR_ARG, bad);
    }
    c->features = F;

    // ---- host-built constants, float64 then rounded once ----
    const double pi = 3.14159265358979323846;
    std::vector<float> taps(3 * kRsTaps), win(kFft), mw(kMel * kMelTaps, 0.f), bscale(kMel), bbase(kMel), twf(kFft), bwf(4 * kFft);
    std::vector<int> mstart(kMel), mcount(kMel), bidx(4 * kFft);
    {   // torchaudio.functional.resample(32000 -> 48000) defaults: sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99
        const double base = 2 * 0.99, lowpass = 6;
        const int width = (int)std::ceil(lowpass * 2 / base);  // 7
        for (int p = 0; p < 3; ++p)
            for (int k = 0; k < kRsTaps; ++k) {
                double t = (-(double)p / 3 + (double)(k - width) / 2) * base;
                t = std::min(std::max(t, -lowpass), lowpass);
                const double w = std::cos(t * pi / lowpass / 2), a = t * pi;
                taps[p * kRsTaps + k] = (float)((a == 0 ? 1.0 : std::sin(a) / a) * w * w * (base / 2));
            }
    }
    for (int n = 0; n < kFft; ++n) win[n] = (float)(0.5 - 0.5 * std::cos(2 * pi * n / kFft));
    for (int k = 0; k < kFft / 2; ++k) {
        twf[2 * k] = (float)std::cos(2 * pi * k / kFft);
        twf[2 * k + 1] = (float)-std::sin(2 * pi * k / kFft);
    }
    {   // slaney mel filter bank, sr 48000, 50 .. 14000 Hz, slaney normalisation; band m is nonzero on a run of bins
        std::vector<double> edge(kMel + 2);
        const double m0 = hz_to_mel(50.0), m1 = hz_to_mel(14000.0);
        for (int i = 0; i < kMel + 2; ++i) edge[i] = mel_to_hz(m0 + (m1 - m0) * i / (kMel + 1));
        for (int m = 0; m < kMel; ++m) {
            int first = -1, count = 0;
            for (int k = 0; k < kBins; ++k) {
                const double f = 24000.0 * k / (kBins - 1);
                const double v = std::max(0.0, std::min((f - edge[m]) / (edge[m + 1] - edge[m]), (edge[m + 2] - f) / (edge[m + 2] - edge[m + 1])));
                if (v > 0) {
                    if (first < 0) first = k;
                    if (k - first >= kMelTaps) return fail(c, LASS_ERR_STATE, "mel band wider than its tap run");
                    mw[m * kMelTaps + (k - first)] = (float)(v * 2.0 / (edge[m + 2] - edge[m]));
                    count = k - first + 1;
                }
            }
            mstart[m] = std::max(first, 0);
            mcount[m] = count;
        }
    }
    {   // bn0 (eval) folded to scale / base
        std::vector<float> w(kMel), b(kMel), mu(kMel), var(kMel);
        HIP_TRY(c, hipMemcpy(w.data(), c->raw.get("audio_branch.bn0.weight"), kMel * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(b.data(), c->raw.get("audio_branch.bn0.bias"), kMel * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(mu.data(), c->raw.get("audio_branch.bn0.running_mean"), kMel * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(var.data(), c->raw.get("audio_branch.bn0.running_var"), kMel * sizeof(float), hipMemcpyDeviceToHost));
        for (int m = 0; m < kMel; ++m) {
            if (!(var[m] + kBnEps > 0)) return fail(c, LASS_ERR_ARG, "audio_branch.bn0.running_var must be positive");
            const double s = (double)w[m] / std::sqrt((double)var[m] + kBnEps);
            bscale[m] = (float)s;
            bbase[m] = (float)((double)b[m] - (double)mu[m] * s);
        }
    }
    for (int t = 0; t < kFft; ++t) {  // bicubic 1001 -> 1024 frames, align_corners, A = -0.75, clamped taps
        const double src = (double)t * (kFrames - 1) / (kFft - 1);
        const int i0 = (int)std::floor(src);
        const double f = src - i0, A = -0.75;
        const double w[4] = {cubic2(f + 1, A), cubic1(f, A), cubic1(1 - f, A), cubic2(2 - f, A)};
        for (int k = 0; k < 4; ++k) {
            bidx[4 * t + k] = std::min(std::max(i0 - 1 + k, 0), kFrames - 1);
            bwf[4 * t + k] = (float)w[k];
        }
    }
    // one allocation, carved
    if (c->consts) (void)hipFree(c->consts);
    c->consts = nullptr;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    const size_t o_taps = take(taps.size() * 4), o_win = take(win.size() * 4), o_tw = take(twf.size() * 4), o_mw = take(mw.size() * 4),
                 o_ms = take(mstart.size() * 4), o_mc = take(mcount.size() * 4), o_bs = take(bscale.size() * 4),
                 o_bb = take(bbase.size() * 4), o_bi = take(bidx.size() * 4), o_bw = take(bwf.size() * 4), o_zero = take(2048 * 4);
    HIP_TRY(c, hipMalloc(&c->consts, o));
    char* d = (char*)c->consts;
    HIP_TRY(c, hipMemset(d, 0, o));
    HIP_TRY(c, hipMemcpy(d + o_taps, taps.data(), taps.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_win, win.data(), win.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_tw, twf.data(), twf.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_mw, mw.data(), mw.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_ms, mstart.data(), mstart.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_mc, mcount.data(), mcount.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_bs, bscale.data(), bscale.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_bb, bbase.data(), bbase.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_bi, bidx.data(), bidx.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(d + o_bw, bwf.data(), bwf.size() * 4, hipMemcpyHostToDevice));
    c->K.taps = (float*)(d + o_taps);
    c->K.win = (float*)(d + o_win);
    c->K.tw = (float2*)(d + o_tw);
    c->K.mw = (float*)(d + o_mw);
    c->K.mstart = (int*)(d + o_ms);
    c->K.mcount = (int*)(d + o_mc);
    c->K.bscale = (float*)(d + o_bs);
    c->K.bbase = (float*)(d + o_bb);
    c->K.bidx = (int4*)(d + o_bi);
    c->K.bw = (float4*)(d + o_bw);
    c->K.zero = (float*)(d + o_zero);
    c->finalized = true;
    return LASS_OK;
}

int lass_audioq_stages(const lass_audioq_ctx* c) { return c && c->finalized ? (int)c->stages.size() : 0; }

int lass_audioq_workspace_bytes(const lass_audioq_ctx* c, int B, size_t* bytes) {
    if (!c || !bytes || B < 1) return LASS_ERR_ARG;
    *bytes = audio_plan(B).total;
    return LASS_OK;
}

int lass_audioq_encode_wave48k(lass_audioq_ctx* c, const float* wave, const int* lengths, int B, int L, float* out,
                               const lass_audioq_taps* taps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* d_len = nullptr;
    const int rc = begin_encode(c, "lass_audioq_encode_wave48k", wave, lengths, B, L, kClip, out, workspace, workspace_bytes, st, &d_len);
    if (rc != LASS_OK) return rc;
    return encode48(c, wave, L, d_len, B, out, taps, (char*)workspace, audio_plan(B), st);
}

int lass_audioq_encode_wave32k(lass_audioq_ctx* c, const float* wave, const int* lengths, int B, int L, float* out,
                               const lass_audioq_taps* taps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int* d_len = nullptr;
    const int rc = begin_encode(c, "lass_audioq_encode_wave32k", wave, lengths, B, L, kMax32k, out, workspace, workspace_bytes, st, &d_len);
    if (rc != LASS_OK) return rc;
    char* ws = (char*)workspace;
    const APlan P = audio_plan(B);
    const int L48 = (3 * L + 1) / 2;
    float* wave48 = (float*)(ws + P.wave48);
    int* d_len48 = d_len + B;
    hipLaunchKernelGGL(k_resample32, dim3((L48 + 255) / 256, B), dim3(256), 0, st, wave, L, d_len, c->K.taps, wave48, L48);
    if (taps && taps->wave48k)
        HIP_TRY(c, hipMemcpyAsync(taps->wave48k, wave48, (size_t)B * L48 * sizeof(float), hipMemcpyDeviceToDevice, st));
    return encode48(c, wave48, L48, d_len48, B, out, taps, ws, P, st);
}

}  // extern "C"
