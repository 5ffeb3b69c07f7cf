// text.hip - the CLAP text tower on the device: RoBERTa-base encoder + pooler + text projection + L2 normalisation
// (CLAP/open_clip/model.py:516-531, 658-665, 732-751 for text_branch_type "roberta"), behind its own lass_text_ctx.
//
// Every launch works on a PACKED token matrix: the M = sum of real tokens rows of all captions (attention_mask != 0),
// caption n owning rows [cap_off[n], cap_off[n+1]).  Dropping the masked positions is exact: position ids are computed
// from the full id row (HF create_position_ids_from_input_ids) and a masked key has weight exactly zero in the reference
// softmax, so no real row ever depends on a padded one.  No work is spent on padding.
//
// Batch invariance: every kernel computes a row (a token, or a caption in the head) from that row's inputs alone in a
// fixed order - the GEMM tile is one shape for all M and each output element is the in-order sum of k-ordered chains of
// f32 MFMA FMAs, one per 64 of k, reductions are per row, attention is per (caption, head, query) - so a caption's
// embedding is bit-identical whatever batch, padding length or packed position it comes with.
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

constexpr int kHid = 768, kHeads = 12, kDh = 64, kFF = 3072, kMaxLen = 512, kPad = 1;

#include "tower_parts.h"

__device__ __forceinline__ int wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Embeddings (RobertaEmbeddings.forward): word[id] + token_type[0] + position[pos], then LayerNorm.  One wave per packed
// row; pos = (id != pad) ? #{c <= s : ids[n][c] != pad} + 1 : pad, counted over the caller's full id row.
__global__ __launch_bounds__(256) void k_embed_ln(const int64_t* __restrict__ ids, int S, const int* __restrict__ src, int M,
                                                  const float* __restrict__ we, int vocab, const float* __restrict__ pe,
                                                  int npos, const float* __restrict__ te, const float* __restrict__ g,
                                                  const float* __restrict__ b, float* __restrict__ h) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int n = src[r] / S, s = src[r] % S;
    const int64_t* row = ids + (size_t)n * S;
    int cnt = 0;
    for (int c = lane; c <= s; c += 64) cnt += row[c] != kPad;
    cnt = wave_isum(cnt);
    const int64_t id64 = row[s];
    // ids are range-checked by the host (ClapTextEncoder.encode_ids); the clamps only keep a bad id from reading outside
    const int id = (int)(id64 < 0 ? 0 : (id64 >= vocab ? vocab - 1 : id64));
    int pos = id64 != kPad ? cnt + 1 : kPad;
    pos = pos < npos ? pos : npos - 1;
    float x[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int k = lane + 64 * j;
        x[j] = (we[(size_t)id * kHid + k] + te[k]) + pe[(size_t)pos * kHid + k];
    }
    ln_row<12>(x, g, b, h + (size_t)r * kHid, lane);
}

// In-place LayerNorm of M rows of 768 (the residual sum was added by the GEMM epilogue).
__global__ __launch_bounds__(256) void k_ln(float* __restrict__ h, int M, const float* __restrict__ g,
                                            const float* __restrict__ b) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    float* row = h + (size_t)r * kHid;
    float x[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) x[j] = row[lane + 64 * j];
    ln_row<12>(x, g, b, row, lane);
}

constexpr int AQ = 64;  // queries per workgroup (one per lane) and keys per LDS block
constexpr int AC = 16;  // keys per online-softmax step

// Self-attention of one (query block, head, caption): softmax(q k^T / 8) v over the caption's real tokens only.  One wave;
// lane = query.  K/V of the caption stream through LDS in blocks of 64 keys with an online softmax, so any length <= 512
// fits.  qkv rows: [q | k | v], 768 each, head h at columns 64h.
__global__ __launch_bounds__(64) void k_attn(const float* __restrict__ qkv, const int* __restrict__ cap_off,
                                             float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float Ks[AQ * kDh], Vs[AQ * kDh];
    const int lane = threadIdx.x, h = blockIdx.y, n = blockIdx.z;
    const int off = cap_off[n], len = cap_off[n + 1] - off;
    const int q0 = blockIdx.x * AQ;
    if (q0 >= len) return;
    const int qi = q0 + lane;
    const bool live = qi < len;
    float q[kDh], o[kDh];
    const float* qp = qkv + (size_t)(off + (live ? qi : 0)) * (3 * kHid) + h * kDh;
#pragma unroll
    for (int d = 0; d < kDh; d += 4) {
        const float4 v = *(const float4*)(qp + d);
        q[d] = v.x; q[d + 1] = v.y; q[d + 2] = v.z; q[d + 3] = v.w;
    }
#pragma unroll
    for (int d = 0; d < kDh; ++d) o[d] = 0.f;
    float mrun = -INFINITY, lrun = 0.f;
    for (int k0 = 0; k0 < len; k0 += AQ) {
        const int nk = min(AQ, len - k0);
        __syncthreads();
        for (int j = 0; j < AQ; ++j) {  // coalesced: row j of K and V, element `lane`; rows past the caption are zero
            const float* kp = qkv + (size_t)(off + k0 + j) * (3 * kHid) + kHid + h * kDh + lane;
            Ks[j * kDh + lane] = j < nk ? kp[0] : 0.f;
            Vs[j * kDh + lane] = j < nk ? kp[kHid] : 0.f;
        }
        __syncthreads();
        for (int c0 = 0; c0 < nk; c0 += AC) {
            float s[AC];
            float cmax = -INFINITY;
#pragma unroll
            for (int j = 0; j < AC; ++j) {
                const float* kr = Ks + (c0 + j) * kDh;
                float dot = 0.f;
#pragma unroll
                for (int d = 0; d < kDh; d += 4) {
                    const float4 kv = *(const float4*)(kr + d);
                    dot = fmaf(q[d], kv.x, dot);
                    dot = fmaf(q[d + 1], kv.y, dot);
                    dot = fmaf(q[d + 2], kv.z, dot);
                    dot = fmaf(q[d + 3], kv.w, dot);
                }
                s[j] = c0 + j < nk ? dot * 0.125f : -INFINITY;
                cmax = fmaxf(cmax, s[j]);
            }
            const float mnew = fmaxf(mrun, cmax);
            const float scale = expf(mrun - mnew);
            float psum = 0.f;
#pragma unroll
            for (int j = 0; j < AC; ++j) {
                s[j] = expf(s[j] - mnew);
                psum += s[j];
            }
            lrun = lrun * scale + psum;
#pragma unroll
            for (int d = 0; d < kDh; ++d) o[d] *= scale;
#pragma unroll
            for (int j = 0; j < AC; ++j) {
                const float* vr = Vs + (c0 + j) * kDh;
#pragma unroll
                for (int d = 0; d < kDh; d += 4) {
                    const float4 vv = *(const float4*)(vr + d);
                    o[d] = fmaf(s[j], vv.x, o[d]);
                    o[d + 1] = fmaf(s[j], vv.y, o[d + 1]);
                    o[d + 2] = fmaf(s[j], vv.z, o[d + 2]);
                    o[d + 3] = fmaf(s[j], vv.w, o[d + 3]);
                }
            }
            mrun = mnew;
        }
    }
    if (!live) return;
    const float inv = 1.0f / lrun;
    float* op = out + (size_t)(off + qi) * kHid + h * kDh;
#pragma unroll
    for (int d = 0; d < kDh; d += 4) *(float4*)(op + d) = make_float4(o[d] * inv, o[d + 1] * inv, o[d + 2] * inv, o[d + 3] * inv);
}

// h[:, 0] of every caption (its first packed row: attention_mask[:, 0] == 1) -> cls (N, 768).
__global__ __launch_bounds__(256) void k_gather_cls(const float* __restrict__ h, const int* __restrict__ cap_off, int N,
                                                    float* __restrict__ cls) {
    const int n = blockIdx.x;
    if (n >= N) return;
    const float* row = h + (size_t)cap_off[n] * kHid;
    for (int k = threadIdx.x; k < kHid; k += 256) cls[(size_t)n * kHid + k] = row[k];
}

struct TLayer {
    float *wqkv = nullptr, *bqkv = nullptr;  // fused (2304, 768) / (2304): query, key, value rows in that order
    const float *wo, *bo, *g1, *b1, *wi, *bi, *w2, *b2, *g2, *b22;
};

// per-layer keys (HF RobertaLayer) and their shapes; 0 stands for "one dimension"
struct LayerKey { const char* name; int d0, d1; };
const LayerKey kLayerKeys[] = {
    {"attention.self.query.weight", kHid, kHid},   {"attention.self.query.bias", kHid, 0},
    {"attention.self.key.weight", kHid, kHid},     {"attention.self.key.bias", kHid, 0},
    {"attention.self.value.weight", kHid, kHid},   {"attention.self.value.bias", kHid, 0},
    {"attention.output.dense.weight", kHid, kHid}, {"attention.output.dense.bias", kHid, 0},
    {"attention.output.LayerNorm.weight", kHid, 0}, {"attention.output.LayerNorm.bias", kHid, 0},
    {"intermediate.dense.weight", kFF, kHid},      {"intermediate.dense.bias", kFF, 0},
    {"output.dense.weight", kHid, kFF},            {"output.dense.bias", kHid, 0},
    {"output.LayerNorm.weight", kHid, 0},          {"output.LayerNorm.bias", kHid, 0},
};
const LayerKey kFixedKeys[] = {
    {"text_branch.embeddings.LayerNorm.weight", kHid, 0}, {"text_branch.embeddings.LayerNorm.bias", kHid, 0},
    {"text_branch.pooler.dense.weight", kHid, kHid},      {"text_branch.pooler.dense.bias", kHid, 0},
    {"text_projection.0.weight", kProj, kHid},            {"text_projection.0.bias", kProj, 0},
    {"text_projection.2.weight", kProj, kProj},           {"text_projection.2.bias", kProj, 0},
};
const char* kLayerPrefix = "text_branch.encoder.layer.";

thread_local std::string g_text_create_err;

}  // namespace

struct lass_text_ctx {
    int device = 0;
    mutable std::string err;  // mutable: lass_text_workspace_bytes takes a const context and still reports why it refused
    ParamStore raw;
    bool finalized = false;
    int vocab = 0, npos = 0;
    std::vector<TLayer> layers;
    std::vector<void*> owned;  // fused QKV buffers
    PinnedInts plan;  // staging of the packed-row plan
};

namespace {

const float* tp(const lass_text_ctx* c, const std::string& k) { return c->raw.get(k); }

// Expected shape of a key, or false if the name is not a text-tower parameter.  Vocabulary and position-table sizes
// come from the tensors themselves; layer indices from the names.
bool expected_shape(const std::string& name, const int64_t* shape, int ndim, std::string& why) {
    auto want = [&](int d0, int d1) {
        const int nd = d1 ? 2 : 1;
        if (ndim != nd || shape[0] != d0 || (nd == 2 && shape[1] != d1)) {
            why = name + ": expected shape (" + std::to_string(d0) + (d1 ? ", " + std::to_string(d1) : std::string(",")) + ")";
            return false;
        }
        return true;
    };
    if (name == "text_branch.embeddings.word_embeddings.weight" || name == "text_branch.embeddings.position_embeddings.weight" ||
        name == "text_branch.embeddings.token_type_embeddings.weight") {
        if (ndim != 2 || shape[1] != kHid || shape[0] < 1) {
            why = name + ": expected shape (rows, 768)";
            return false;
        }
        return true;
    }
    for (const auto& k : kFixedKeys)
        if (name == k.name) return want(k.d0, k.d1);
    if (name.rfind(kLayerPrefix, 0) == 0) {
        const std::string rest = name.substr(strlen(kLayerPrefix));
        const size_t dot = rest.find('.');
        if (dot != std::string::npos && dot > 0 && rest.find_first_not_of("0123456789") == dot) {
            const std::string suffix = rest.substr(dot + 1);
            for (const auto& k : kLayerKeys)
                if (suffix == k.name) return want(k.d0, k.d1);
        }
    }
    why = "unknown text-tower parameter '" + name + "'";
    return false;
}

struct TPlan {  // workspace carve-up for (N, S): everything sized for M = N*S rows, the packed batch uses the first M_real
    size_t src, cap, h, qkv, attn, ffn, cls, pool, p1, p2, total;
};

TPlan text_plan(int N, int S) {
    const size_t M = (size_t)N * S;
    TPlan p;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    p.src = take(M * sizeof(int));
    p.cap = take((N + 1) * sizeof(int));
    p.h = take(M * kHid * sizeof(float));
    p.qkv = take(M * 3 * kHid * sizeof(float));
    p.attn = take(M * kHid * sizeof(float));
    p.ffn = take(M * kFF * sizeof(float));
    p.cls = take((size_t)N * kHid * sizeof(float));
    p.pool = take((size_t)N * kHid * sizeof(float));
    p.p1 = take((size_t)N * kProj * sizeof(float));
    p.p2 = take((size_t)N * kProj * sizeof(float));
    p.total = o;
    return p;
}

}  // namespace

extern "C" {

int lass_text_create(lass_text_ctx** out, int device_id) {
    if (!out) return LASS_ERR_ARG;
    *out = nullptr;
    if (int rc = open_device(device_id, g_text_create_err)) return rc;
    lass_text_ctx* c = new lass_text_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || c->plan.create() != hipSuccess) {
        g_text_create_err = "hipSetDevice / hipEventCreate failed";
        delete c;
        return LASS_ERR_HIP;
    }
    *out = c;
    return LASS_OK;
}

int lass_text_destroy(lass_text_ctx* c) {
    if (!c) return LASS_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    c->raw.free_all();
    for (void* p : c->owned) (void)hipFree(p);
    c->plan.destroy();
    delete c;
    return LASS_OK;
}

const char* lass_text_last_error(const lass_text_ctx* c) { return c ? c->err.c_str() : g_text_create_err.c_str(); }

int lass_text_set_param(lass_text_ctx* c, const char* name, const void* data, const int64_t* shape, int ndim) {
    if (!c) return LASS_ERR_ARG;
    if (!name || !data || !shape || ndim < 1 || ndim > 2) return fail(c, LASS_ERR_ARG, "lass_text_set_param: bad arguments");
    std::string why;
    if (!expected_shape(name, shape, ndim, why)) return fail(c, LASS_ERR_ARG, why);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = c->raw.put(c, name, data, shape, ndim)) return rc;
    c->finalized = false;
    return LASS_OK;
}

int lass_text_finalize(lass_text_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());
    for (void* p : c->owned) (void)hipFree(p);
    c->owned.clear();
    c->layers.clear();
    c->finalized = false;
    for (const char* k : {"text_branch.embeddings.word_embeddings.weight", "text_branch.embeddings.position_embeddings.weight",
                          "text_branch.embeddings.token_type_embeddings.weight"})
        if (!tp(c, k)) return fail(c, LASS_ERR_STATE, std::string("missing parameter ") + k);
    for (const auto& k : kFixedKeys)
        if (!tp(c, k.name)) return fail(c, LASS_ERR_STATE, std::string("missing parameter ") + k.name);
    c->vocab = (int)c->raw.by_name["text_branch.embeddings.word_embeddings.weight"].shape[0];
    c->npos = (int)c->raw.by_name["text_branch.embeddings.position_embeddings.weight"].shape[0];
    if (c->npos < 3) return fail(c, LASS_ERR_ARG, "position_embeddings needs at least 3 rows");
    // layer count = number of distinct layer indices; they must be 0 .. L-1, each complete
    int nl = 0;
    for (const auto& kv : c->raw.by_name)
        if (kv.first.rfind(kLayerPrefix, 0) == 0) nl = std::max(nl, atoi(kv.first.c_str() + strlen(kLayerPrefix)) + 1);
    if (nl < 1) return fail(c, LASS_ERR_STATE, "no encoder layer parameters (text_branch.encoder.layer.<i>.*)");
    for (int l = 0; l < nl; ++l) {
        const std::string pre = kLayerPrefix + std::to_string(l) + ".";
        const float* p[16];
        for (int i = 0; i < 16; ++i) {
            p[i] = tp(c, pre + kLayerKeys[i].name);
            if (!p[i]) return fail(c, LASS_ERR_STATE, "missing parameter " + pre + kLayerKeys[i].name);
        }
        TLayer L;
        HIP_TRY(c, hipMalloc(&L.wqkv, (size_t)3 * kHid * kHid * sizeof(float)));
        c->owned.push_back(L.wqkv);
        HIP_TRY(c, hipMalloc(&L.bqkv, (size_t)3 * kHid * sizeof(float)));
        c->owned.push_back(L.bqkv);
        for (int j = 0; j < 3; ++j) {
            HIP_TRY(c, hipMemcpy(L.wqkv + (size_t)j * kHid * kHid, p[2 * j], (size_t)kHid * kHid * sizeof(float),
                                  hipMemcpyDeviceToDevice));
            HIP_TRY(c, hipMemcpy(L.bqkv + j * kHid, p[2 * j + 1], kHid * sizeof(float), hipMemcpyDeviceToDevice));
        }
        L.wo = p[6]; L.bo = p[7]; L.g1 = p[8]; L.b1 = p[9];
        L.wi = p[10]; L.bi = p[11]; L.w2 = p[12]; L.b2 = p[13]; L.g2 = p[14]; L.b22 = p[15];
        c->layers.push_back(L);
    }
    c->finalized = true;
    return LASS_OK;
}

int lass_text_layers(const lass_text_ctx* c) { return c && c->finalized ? (int)c->layers.size() : 0; }

int lass_text_workspace_bytes(const lass_text_ctx* c, int N, int S, size_t* bytes) {
    if (!c) return LASS_ERR_ARG;
    if (!bytes || N < 1 || S < 1 || S > kMaxLen)
        return fail(c, LASS_ERR_ARG, "lass_text_workspace_bytes: bad arguments (N >= 1, 1 <= S <= 512, non-NULL bytes)");
    *bytes = text_plan(N, S).total;
    return LASS_OK;
}

int lass_text_encode(lass_text_ctx* c, const int64_t* input_ids, const int64_t* attention_mask, int N, int S, float* out,
                     float* pooler_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (!c->finalized) return fail(c, LASS_ERR_STATE, "lass_text_finalize has not been called (or a parameter changed since)");
    if (!input_ids || !attention_mask || !out || !workspace || N < 1 || S < 1 || S > kMaxLen)
        return fail(c, LASS_ERR_ARG, "lass_text_encode: bad arguments (N >= 1, 1 <= S <= 512, non-NULL buffers)");
    if (S + 1 >= c->npos) return fail(c, LASS_ERR_ARG, "S too long for the position table (needs S + 2 rows)");
    const TPlan P = text_plan(N, S);
    if (workspace_bytes < P.total) return fail(c, LASS_ERR_ARG, "workspace too small (lass_text_workspace_bytes)");
    HIP_TRY(c, hipSetDevice(c->device));
    hipStream_t st = (hipStream_t)stream;
    // packed-row plan from the host mask: src[r] = n*S + s for every real token, cap_off[n] = first row of caption n
    if (int rc = c->plan.reserve(c, (size_t)N * S + N + 1)) return rc;
    int* src = c->plan.host;
    int* cap = c->plan.host + (size_t)N * S;
    int M = 0, maxlen = 0;
    for (int n = 0; n < N; ++n) {
        cap[n] = M;
        if (attention_mask[(size_t)n * S] == 0)
            return fail(c, LASS_ERR_ARG, "attention_mask[:, 0] must be 1 (the <s> token of every caption is real)");
        for (int s = 0; s < S; ++s)
            if (attention_mask[(size_t)n * S + s] != 0) src[M++] = n * S + s;
        maxlen = std::max(maxlen, M - cap[n]);
    }
    cap[N] = M;
    char* ws = (char*)workspace;
    int* d_src = (int*)(ws + P.src);
    int* d_cap = (int*)(ws + P.cap);
    HIP_TRY(c, hipMemcpyAsync(d_src, src, (size_t)M * sizeof(int), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(d_cap, cap, (N + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    if (int rc = c->plan.record(c, st)) return rc;

    float* h = (float*)(ws + P.h);
    float* qkv = (float*)(ws + P.qkv);
    float* attn = (float*)(ws + P.attn);
    float* ffn = (float*)(ws + P.ffn);
    const dim3 rows4((M + 3) / 4);
    hipLaunchKernelGGL(k_embed_ln, rows4, dim3(256), 0, st, input_ids, S, d_src, M,
                       tp(c, "text_branch.embeddings.word_embeddings.weight"), c->vocab,
                       tp(c, "text_branch.embeddings.position_embeddings.weight"), c->npos,
                       tp(c, "text_branch.embeddings.token_type_embeddings.weight"),
                       tp(c, "text_branch.embeddings.LayerNorm.weight"), tp(c, "text_branch.embeddings.LayerNorm.bias"), h);
    for (const TLayer& L : c->layers) {
        gemm<EPI_BIAS>(h, L.wqkv, L.bqkv, qkv, M, 3 * kHid, kHid, st);
        hipLaunchKernelGGL(k_attn, dim3((maxlen + AQ - 1) / AQ, kHeads, N), dim3(AQ), 0, st, qkv, d_cap, attn);
        gemm<EPI_RESID>(attn, L.wo, L.bo, h, M, kHid, kHid, st);
        hipLaunchKernelGGL(k_ln, rows4, dim3(256), 0, st, h, M, L.g1, L.b1);
        gemm<EPI_GELU>(h, L.wi, L.bi, ffn, M, kFF, kHid, st);
        gemm<EPI_RESID>(ffn, L.w2, L.b2, h, M, kHid, kFF, st);
        hipLaunchKernelGGL(k_ln, rows4, dim3(256), 0, st, h, M, L.g2, L.b22);
    }
    float* cls = (float*)(ws + P.cls);
    float* pool = pooler_out ? pooler_out : (float*)(ws + P.pool);
    float* p1 = (float*)(ws + P.p1);
    float* p2 = (float*)(ws + P.p2);
    hipLaunchKernelGGL(k_gather_cls, dim3(N), dim3(256), 0, st, h, d_cap, N, cls);
    gemm<EPI_TANH>(cls, tp(c, "text_branch.pooler.dense.weight"), tp(c, "text_branch.pooler.dense.bias"), pool, N, kHid, kHid, st);
    gemm<EPI_RELU>(pool, tp(c, "text_projection.0.weight"), tp(c, "text_projection.0.bias"), p1, N, kProj, kHid, st);
    gemm<EPI_BIAS>(p1, tp(c, "text_projection.2.weight"), tp(c, "text_projection.2.bias"), p2, N, kProj, kProj, st);
    hipLaunchKernelGGL(k_l2norm, dim3((N + 3) / 4), dim3(256), 0, st, p2, N, out);
    HIP_TRY(c, hipGetLastError());
    return LASS_OK;
}

}  // extern "C"
