// api.hip - the C-ABI of include/lass_hip.h: context, weight ingestion/folding, workspace plan, forward orchestration.
//
// Forward order mirrors /root/reference/models/resunet.py:522-595 (ResUNet30_Base.forward) with FiLM (:59-81) hoisted to
// one launch.  torch.cat of the decoder (:258) is virtual: encoder blocks write their skip output straight into the
// second channel half of the decoder's concat buffer and the transposed conv writes the first half.
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
#include "graph_cache.h"
#include "head_fold.h"
#include "kernels.h"
#include "weight_plan.h"
#include "workspace_plan.h"

namespace {

constexpr float kBnEps = 1e-5f;
constexpr int kMaxBranches = LASS_MAX_STFT_WINDOWS;

struct Site {
    std::string film;  // "encoder_block1->conv_block1->beta1"
    std::string bn;    // "base.encoder_block1.conv_block1.bn1"
    int C = 0;
    int off = 0;
};

struct ResBlock {  // one ConvBlockRes
    std::string prefix;  // "base.encoder_block1.conv_block1"
    int cin = 0, cout = 0;
    int width = 0;         // bins of the level the block runs at (fcrop >> level): known at finalize, the frame count is not
    int s1 = -1, s2 = -1;  // site indices
    WeightImages img;      // the block slots of weight_plan.h, as lass_finalize made them
};

struct ProfEntry {
    const char* name;
    double ms = 0;
    int launches = 0;
};

thread_local std::string g_create_err;

}  // namespace

struct lass_ctx {
    int device = 0;
    std::string err;
    Geometry g;
    ModelTable m;  // encoder / decoder table of THIS model (conv_route.h)
    std::string pre_name[kMaxBranches];  // "base.pre_conv" / "base.pre_convs.<win>"
    ParamStore raw;
    bool finalized = false;
    float2* tw2k = nullptr;  // (cos, sin)(2 pi k / 2048): twiddles of every transform size + the Hann windows
    std::vector<Site> sites;
    std::map<std::string, int> site_idx;
    int n_shift = 0;
    float *film_W = nullptr, *film_b = nullptr, *bn_scale = nullptr, *bn_base = nullptr;
    float *bn0_s = nullptr, *bn0_h = nullptr;
    std::vector<ResBlock> enc, dec;  // enc: nbr branch blocks (encoder_block1[s]) then the 6 trunk blocks; dec: 6
    int dec_site[6] = {0};           // decoder_blockN->beta1
    WeightImages up_img[6], img;     // the decoder slots of weight_plan.h per transposed conv, and the context's (lass_finalize)
    int head_rows = 0;               // rows of after_conv as lass_finalize saw them: the Q of weight_plan.h's head rules
    std::vector<void*> owned;        // derived device buffers to free
    // the compute mode (lass_finalize) and every switch a route depends on, as the value conv_route.h's rules read: LASS_WINO4,
    // lass_set_wino4_splits, lass_set_wino4_vprep / LASS_WINO4_VPREP, lass_set_head_fold / LASS_HEAD_FOLD, lass_set_head_sc_fold /
    // LASS_HEAD_SC_FOLD, lass_set_pw_split / LASS_PW_SPLIT, LASS_FUSE_CATB / _BLOCK / _UP
    RouteCfg cfg;
    float* stage_v = nullptr;      // the V image of the V-from-memory layers in the stage calls, grown on demand like stage_part (Plan::vprep in lass_separate)
    size_t stage_v_floats = 0;
    float* stage_m = nullptr;      // ... and the product image of the gemm route, grown on demand (Plan::mgemm in lass_separate)
    size_t stage_m_floats = 0;
    float* stage_v_user = nullptr; // lass_set_wino4_vprep_buffer: a caller-owned image buffer for the stage calls instead
    size_t stage_v_user_floats = 0;
    float* stage_part = nullptr;   // split-K partials of the stage calls (lass_convblock, lass_encoder_block), grown on demand;
    size_t stage_part_floats = 0;  // lass_separate takes its own from the caller's workspace (Plan::kpart)
    // hipGraph replay of lass_separate (LASS_GRAPH=0 disables): the ~40 launches of one (pointers, shape) combination are
    // captured once on an internal stream and replayed on the caller's stream
    bool use_graph = true;
    // A key is captured on the third call that presents it; the bookkeeping is graph_cache.h's.  Replaced execs may still be
    // replaying on some stream: they are destroyed only behind a device synchronisation (separate_call / lass_finalize / lass_destroy)
    GraphCache<hipGraphExec_t> graphs;
    // (B, L) -> did the LAST lass_separate of that shape run as half-batches?  lass_workspace_tensor refuses only then: eager
    // calls (the first calls of a key, LASS_GRAPH=0, changing pointers) leave the whole-batch layout, taps stay readable.
    std::map<std::pair<int, int>, bool> last_split;
    hipStream_t g_stream = nullptr;
    // Half-batch overlap: an even batch of >= 8 clips runs as two independent half-batches on two streams (clips are
    // independent: eval-mode BN) - the second on `s2`, forked from / joined to the caller's stream by events - so that one
    // half's small launches (the 16-/8-bin layers: a few hundred workgroups) and launch tails run beside the other half's
    // full-size launches.  Same kernels, same per-clip arithmetic (bit-identical: batch invariance), same workspace size.
    // Measured: bf16 +3.4 %, f32 +0.5 ... +2.1 % depending on the box, split-bf16 +1.1 %.
    // 1 (default): only inside the captured hipGraph that lass_separate replays - an EAGER two-stream launch depends on the
    // process having a free hardware queue for `s2` (with an RCCL communicator alive in the process it measured 8 % SLOWER than
    // the unsplit launch, without one 2 % faster; a graph's branches do not care).  LASS_SPLIT=2: eager launches too; 0: never.
    // DESIGN.md section 5b has the measurements and the co-residency hazard found on the way.
    int split_batch = 1;
    hipStream_t s2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    unsigned long gen = 0;         // bumped by lass_finalize: a graph holds weight pointers (GraphKey::gen)
    long g_replays = 0, g_captures = 0;
    bool profiling = false;
    std::vector<ProfEntry> prof;
    std::vector<hipEvent_t> ev_pool;
    struct Pending { int cls; hipEvent_t a, b; };
    std::vector<Pending> pending;
    size_t ev_used = 0;
};

namespace {

bool starts_with(const std::string& s, const char* p) { return s.rfind(p, 0) == 0; }
bool ends_with(const std::string& s, const char* p) {
    const size_t n = strlen(p);
    return s.size() >= n && s.compare(s.size() - n, n, p) == 0;
}

std::string film_to_bn(const std::string& film) {  // 'a->b->beta1' -> 'base.a.b.bn1'
    std::string s = "base.";
    for (size_t i = 0; i < film.size(); ++i) {
        if (film[i] == '-' && i + 1 < film.size() && film[i + 1] == '>') {
            s += '.';
            ++i;
        } else {
            s += film[i];
        }
    }
    const size_t p = s.rfind("beta");
    s.replace(p, 4, "bn");
    return s;
}

int add_site(lass_ctx* c, const std::string& film, int C) {
    Site s;
    s.film = film;
    s.bn = film_to_bn(film);
    s.C = C;
    s.off = c->n_shift;
    c->n_shift += C;
    c->site_idx[film] = (int)c->sites.size();
    c->sites.push_back(s);
    return (int)c->sites.size() - 1;
}

void build_arch(lass_ctx* c) {
    const Geometry& g = c->g;
    c->sites.clear();
    c->site_idx.clear();
    c->n_shift = 0;
    c->enc.clear();
    c->dec.clear();
    c->m = model_table(g.variant == 0 ? 0 : g.nbr, g.fcrop);
    for (int k = 0; k < g.nbr; ++k) {  // analysis branches
        ResBlock rb;
        std::string film;
        if (g.variant == 0) {
            rb.prefix = "base.encoder_block1.conv_block1";
            film = "encoder_block1->conv_block1";
            c->pre_name[k] = "base.pre_conv";
        } else {
            const std::string w = std::to_string(g.wins[k]);
            rb.prefix = "base.encoder_block1s." + w + ".conv_block1";
            film = "encoder_block1s->" + w + "->conv_block1";
            c->pre_name[k] = "base.pre_convs." + w;
        }
        rb.cin = rb.cout = kPreCh;
        rb.width = g.fcrop;
        rb.s1 = add_site(c, film + "->beta1", kPreCh);
        rb.s2 = add_site(c, film + "->beta2", kPreCh);
        c->enc.push_back(rb);
    }
    for (int i = 1; i < 7; ++i) {
        const EncSpec& e = c->m.E[i];
        ResBlock rb;
        rb.prefix = std::string("base.") + e.name + ".conv_block1";
        rb.cin = e.cin;
        rb.cout = e.cout;
        rb.width = g.fcrop >> i;  // encoder i (0-based) runs behind i frequency halvings: 512, 256, ..., 16, 8 bins at n_fft 1024
        rb.s1 = add_site(c, std::string(e.name) + "->conv_block1->beta1", e.cin);
        rb.s2 = add_site(c, std::string(e.name) + "->conv_block1->beta2", e.cout);
        c->enc.push_back(rb);
    }
    for (int i = 0; i < 6; ++i) {
        const auto& d = c->m.D[i];
        const int e = 5 - i;
        c->dec_site[i] = add_site(c, std::string(d.name) + "->beta1", d.cin);
        ResBlock rb;
        rb.prefix = std::string("base.") + d.name + ".conv_block2";
        rb.cin = c->m.dec_cat[i];
        rb.cout = d.cout;
        rb.width = g.fcrop >> e;  // decoder i runs at its skip's level: 16, 32, ..., 512 bins
        rb.s1 = add_site(c, std::string(d.name) + "->conv_block2->beta1", rb.cin);
        rb.s2 = add_site(c, std::string(d.name) + "->conv_block2->beta2", d.cout);
        c->dec.push_back(rb);
    }
}

// Expected shape of a required parameter, or empty if the name is not one.
std::vector<int64_t> expected_shape(const lass_ctx* c, const std::string& name) {
    auto bn_field = [](const std::string& n) {
        return ends_with(n, ".weight") || ends_with(n, ".bias") || ends_with(n, ".running_mean") ||
               ends_with(n, ".running_var");
    };
    if (starts_with(name, "base.bn0.") && bn_field(name)) return {c->g.nbins};
    for (int k = 0; k < c->g.nbr; ++k) {
        if (name == c->pre_name[k] + ".weight") return {kPreCh, 1, 1, 1};
        if (name == c->pre_name[k] + ".bias") return {kPreCh};
    }
    if (name == "base.after_conv.weight") return {3, kPreCh, 1, 1};
    if (name == "base.after_conv.bias") return {3};
    auto res_block = [&](const ResBlock& rb) -> std::vector<int64_t> {
        const std::string& p = rb.prefix;
        if (!starts_with(name, (p + ".").c_str())) return {};
        const std::string f = name.substr(p.size() + 1);
        if (starts_with(f, "bn1.") && bn_field(f)) return {rb.cin};
        if (starts_with(f, "bn2.") && bn_field(f)) return {rb.cout};
        if (f == "conv1.weight") return {rb.cout, rb.cin, 3, 3};
        if (f == "conv2.weight") return {rb.cout, rb.cout, 3, 3};
        if (rb.cin != rb.cout && f == "shortcut.weight") return {rb.cout, rb.cin, 1, 1};
        if (rb.cin != rb.cout && f == "shortcut.bias") return {rb.cout};
        return {};
    };
    for (const auto& rb : c->enc) {
        auto s = res_block(rb);
        if (!s.empty()) return s;
    }
    for (int i = 0; i < 6; ++i) {
        auto s = res_block(c->dec[i]);
        if (!s.empty()) return s;
        const DecSpec& d = c->m.D[i];
        const std::string p = std::string("base.") + d.name;
        if (name == p + ".conv1.weight") return {d.cin, d.cout, d.uh, d.uw};
        if (starts_with(name, (p + ".bn1.").c_str()) && bn_field(name)) return {d.cin};
    }
    if (starts_with(name, "film.")) {
        for (const auto& s : c->sites) {
            if (name == "film." + s.film + ".weight") return {s.C, LASS_COND};
            if (name == "film." + s.film + ".bias") return {s.C};
        }
    }
    return {};
}

bool ignorable(const std::string& name) {
    if (starts_with(name, "base.stft.") || starts_with(name, "base.istft.")) return true;
    if (ends_with(name, "num_batches_tracked")) return true;
    for (const auto& d : kDec) {
        if (starts_with(name, (std::string("base.") + d.name + ".bn2.").c_str())) return true;      // resunet.py:230
        if (starts_with(name, (std::string("film.") + d.name + "->beta2.").c_str())) return true;  // never read
    }
    return false;
}

const float* rawp(const lass_ctx* c, const std::string& name) { return c->raw.get(name); }

template <typename T>
int dev_alloc(lass_ctx* c, T** p, size_t count) {
    void* v = nullptr;
    HIP_TRY(c, hipMalloc(&v, count * sizeof(T)));
    c->owned.push_back(v);
    *p = (T*)v;
    return 0;
}

void free_owned(lass_ctx* c) {
    for (void* p : c->owned) (void)hipFree(p);
    c->owned.clear();
}

// The slots of `want` (weight_plan.h: route_images) that lass_finalize has not made: the block's in `blk`, its decoder's in `up`
// (either may be null: such a slot counts as missing), the context's in c->img
SlotSet missing_images(const lass_ctx* c, const WeightImages* blk, const WeightImages* up, SlotSet want) {
    SlotSet miss = 0;
    for (int s = 0; s < kWeightSlots; ++s) {
        const WeightImages* im = s < kBlockSlots ? blk : s < kDecoderSlotsEnd ? up : &c->img;
        if ((want >> s & 1) && !(im && im->p[s])) miss |= SlotSet(1) << s;
    }
    return miss;
}

// ---- profiling ----------------------------------------------------------------------------------------------------
enum ProfClass { P_STFT = 0, P_FILM, P_PRECONV, P_CONV3X3, P_TCONV, P_POOL, P_MASK, P_ISTFT, P_COUNT };
const char* kProfNames[P_COUNT] = {"stft_magphase", "film", "pre_conv", "conv3x3_mfma", "tconv_mfma",
                                   "avg_pool",      "mask_apply", "istft"};

// Event pairs come from a pool that lass_set_profiling sizes up front: nothing is created (or allocated) inside
// lass_separate.  When a caller lets more than kProfPairs scopes accumulate without collecting them
// (lass_profile_get / lass_profile_reset), the surplus scopes are simply not timed.
constexpr size_t kProfPairs = 512;

struct ProfScope {
    lass_ctx* c;
    hipStream_t s;
    int cls;
    hipEvent_t b = nullptr;
    bool on = false;
    ProfScope(lass_ctx* ctx, hipStream_t st, int k) : c(ctx), s(st), cls(k) {
        if (!c->profiling || c->ev_used + 2 > c->ev_pool.size()) return;
        hipEvent_t a = c->ev_pool[c->ev_used++];
        b = c->ev_pool[c->ev_used++];
        (void)hipEventRecord(a, s);
        c->pending.push_back({cls, a, b});
        on = true;
    }
    ~ProfScope() {
        if (on) (void)hipEventRecord(b, s);
    }
};

void prof_collect(lass_ctx* c) {
    for (auto& p : c->pending) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            c->prof[p.cls].ms += ms;
            c->prof[p.cls].launches += 1;
        }
    }
    c->pending.clear();
    c->ev_used = 0;
}

// ---- one residual block ---------------------------------------------------------------------------------------------
// x: (B,cin,H,W) batch stride x_bs; out: batch stride out_bs (may be a channel slice of a concat buffer).
// bf16 mode: a decoder's concat input (transposed-conv output | encoder skip) kept as two blocked bf16 copies in the
// concat buffer's storage - `act` (consumer prologue applied) for conv1, `raw` for the 1x1 shortcut (ConvArgs::out_bf16_act)
struct CatCopies {
    void* act;
    void* raw;
    int noct;            // octets per clip = 2C / 8
    const float* scale;  // conv_block2.bn1 (+ FiLM shift below) of the decoder, at concat channel 0
    const float* shift;
};

// Output head fused into the last decoder block's conv2 (after_conv + complex ratio mask): inputs / outputs of the mask
struct MaskHead {
    const float* mag;
    const float* cosv;
    const float* sinv;
    float* oreal;
    float* oimag;
    int T;
    int nbins;
};

// encoder_block1[s] input: the block input is pre_conv(x0) (1 -> 32 channels, resunet.py:555), formed while staging
struct PreConv {
    const float* x0;
    const float* w;
    const float* b;
};

// bf16 mode, decoder_block6: the transposed conv in front of the block runs inside the fused kernel (conv_bf16_fused.hip)
struct UpFuse {
    const void* xin;     // previous decoder's output, that conv's prologue applied, blocked bf16 (B, cin/8, h, w, 8)
    int cin, h, w;
    const void* w16;     // transposed-conv weights, bf16
    const void* wsc16;   // shortcut (up-sampled half) composed with the transposed conv, bf16
};

// What lass_separate fuses into one block beyond the plain ConvBlockRes; a default-constructed value fuses nothing.
struct BlockFusions {
    float* pool_out = nullptr;              // the block's avg-pooled output (B,cout,H/pool_h,W/2), from conv2's epilogue
    int pool_h = 2;
    long pool_bs = 0;                       // pool_out's batch stride (0: dense)
    int cofs = 0;                           // this branch's channel offset inside the concatenated skip / pool
    const PreConv* pre = nullptr;           // encoder_block1: the input is pre_conv(x0), formed on the fly - x is ignored
    const MaskHead* head = nullptr;         // decoder_block6: after_conv + mask in conv2's epilogue, `out` is not written
    const CatCopies* skip_out = nullptr;    // bf16: the skip output as the decoder concat's two blocked copies
    const CatCopies* cat_in = nullptr;      // bf16: the concat input as two blocked copies
    const Site* act_out = nullptr;          // bf16: the output as ONE blocked tensor with this site's prologue applied
    const CatCopies* pool_copies = nullptr; // bf16: the pooled output as two blocked copies for the next encoder block
    const UpFuse* up = nullptr;             // bf16, decoder_block6: its transposed conv inside the block's fused kernel
    float* kpart = nullptr;                 // f32: the block's split-K partials, BlockRoute::kpart_floats of them (conv_route.h)
    float* vws = nullptr;                   // f32: the transformed input image of one conv at a time (the V-from-memory layers),
    size_t vws_floats = 0;                  // at least BlockRoute::v_floats
    float* mws = nullptr;                   // f32: the product image of one conv at a time on the gemm route (wino4_gemm.hip),
    size_t mws_floats = 0;                  // at least BlockRoute::m_floats
    const HeadScPlanes* planes = nullptr;   // f32, encoder_block1 / decoder_block6 of lass_separate: the head's shortcut logits as
                                            // planes (Plan::lg_skip / lg_up) - written by conv2's epilogue / read by the folded head
};

// What one block call's site adds to the block's shape (conv_route.h holds the rules that read it)
BlockIO block_io(const float* x, long x_bs, const BlockFusions& f) {
    BlockIO io;
    io.x0 = f.pre && f.pre->x0;
    io.head = f.head != nullptr;
    io.pool = f.pool_out != nullptr; io.pool_h = f.pool_h;
    io.x_aligned = x && ((uintptr_t)x & 15u) == 0 && x_bs % 4 == 0;
    io.sc_planes = f.planes != nullptr;
    io.cat_in = f.cat_in != nullptr; io.skip_out = f.skip_out != nullptr; io.pool_copies = f.pool_copies != nullptr;
    io.act_out = f.act_out != nullptr; io.up_cin = f.up ? f.up->cin : 0;
    return io;
}

// Do B clips of a_n floats, a_bs apart from a (a_bs = 0: one dense range), and the same of b share an element?
bool overlaps(int B, const float* a, long a_bs, size_t a_n, const float* b, long b_bs, size_t b_n) {
    return a && b && a_n && b_n && a < b + (size_t)(B - 1) * b_bs + b_n && b < a + (size_t)(B - 1) * a_bs + a_n;
}

// The bf16 modes, a block their kernels take, in its planned form (conv_route.h: plan_bf16_block): p / q = the filled conv1 /
// conv2 arguments.  As in launch_routed, the pointer-taking predicate of a fused kernel has the last word.
int run_resblock_bf16(lass_ctx* c, const ResBlock& rb, Bf16Form form, const ConvArgs& p, const ConvArgs& q, int B, hipStream_t st,
                      const BlockFusions& f) {
    if (form == BF16_TWO) {
        const bool x0 = f.pre && f.pre->x0;
        {
            ProfScope ps(c, st, P_CONV3X3);
            HIP_TRY(c, lass_launch_conv_bf16(x0 ? CONV1_ACT_PRE : CONV1_ACT, p, st));
        }
        ProfScope ps(c, st, P_CONV3X3);
        HIP_TRY(c, lass_launch_conv_bf16(rb.cin != rb.cout ? CONV2_SHORTCUT : x0 ? CONV2_IDENT_PRE : CONV2_IDENT, q, st));
        return 0;
    }
    // conv_bf16_fused.hip: encoder_block1 as ONE kernel, its 32-channel intermediate kept in LDS; decoder_block6 with the output
    // head behind it (conv1 from the activated cat copy, the 1x1 shortcut from the raw one), behind its transposed conv's launch
    // or - the caller has NOT run it - with that conv inside
    ConvArgs uq;
    if (const UpFuse* up = f.up) {
        uq.in_bf16 = up->xin; uq.Cin = up->cin; uq.H = up->h; uq.W = up->w; uq.B = B;
        uq.w_bf16 = up->w16; uq.w2_bf16 = up->wsc16;
    }
    if (!(form == BF16_ENC1 ? lass_enc1_fused_bf16_supported(p, q) : form == BF16_DEC6 ? lass_dec6_fused_bf16_supported(p, q)
                            : form == BF16_DEC6U && f.up && lass_dec6u_fused_bf16_supported(p, q, uq)))
        return fail(c, LASS_ERR_STATE, rb.prefix + ": the launch arguments contradict the planned route");
    ProfScope ps(c, st, P_CONV3X3);
    HIP_TRY(c, form == BF16_ENC1 ? lass_launch_enc1_fused_bf16(p, q, st) : form == BF16_DEC6 ? lass_launch_dec6_fused_bf16(p, q, st)
                                 : lass_launch_dec6u_fused_bf16(p, q, uq, st));
    return 0;
}

// One f32 conv launch of a block as its route says.  The pointer-taking predicate of the chosen family has the last word: where
// it contradicts the route (which saw the shape and the call-site facts of BlockIO only) nothing is launched.
int launch_routed(lass_ctx* c, const ResBlock& rb, const char* what, const ConvRoute& rt, const ConvArgs& a, const Wino4Split& sk,
                  float* vws, const Wino4Gemm& wg, hipStream_t st, const HeadScPlanes* planes = nullptr) {
    ProfScope ps(c, st, P_CONV3X3);
    bool ok = true;
    switch (rt.family) {
        case CONV_F4X4: {
            const Wino4Split s = rt.splits > 1 ? sk : Wino4Split();
            Wino4VPre vp;
            if (rt.v_from_memory) vp.v = vws;
            if (rt.head_sc_fold) {  // the folded head on the planes, or encoder_block1.conv2 that writes the skip's
                ok = planes && (rt.head_fold ? lass_wino4_headfold_planes_supported(a, *planes) : lass_wino4_sclogit_supported(a, *planes));
                if (ok) HIP_TRY(c, rt.head_fold ? lass_launch_wino4_headfold_planes(a, *planes, st) : lass_launch_wino4_sclogit(a, *planes, st));
                break;
            }
            if (rt.head_fold) {
                ok = lass_wino4_headfold_supported(a);
                if (ok) HIP_TRY(c, lass_launch_wino4_headfold(a, st));
                break;
            }
            if (rt.gemm) {  // scatter, 36 GEMMs, gather: three launches under this conv's scope, as the prep launch shares it
                ok = lass_wino4_gemm_supported(rt.kind, a, vp, wg);
                if (ok) HIP_TRY(c, lass_launch_wino4_gemm(rt.kind, a, vp, wg, st));
                break;
            }
            ok = rt.v_from_memory ? lass_wino4_vpre_supported(rt.kind, a, s) : lass_wino4_supported(rt.kind, a, s);
            if (ok) HIP_TRY(c, lass_launch_wino4(rt.kind, a, st, s, vp));
            break;
        }
        case CONV_F2X2:
            ok = lass_wino_supported(a);
            if (ok) HIP_TRY(c, lass_launch_wino(rt.kind, a, st));
            break;
        case CONV_DIRECT:
            HIP_TRY(c, lass_launch_conv(rt.kind, a, st));
            break;
        case CONV_NONE:
            ok = false;
            break;
    }
    return ok ? 0 : fail(c, LASS_ERR_STATE, rb.prefix + " " + what + ": the launch arguments contradict the planned route");
}

int run_resblock(lass_ctx* c, const ResBlock& rb, const float* x, long x_bs, int B, int H, int W, const float* shift,
                 float* a2, float* out, long out_bs, hipStream_t st, const BlockFusions& f = BlockFusions()) {
    const PreConv* pre = f.pre;
    const WeightImages& im = rb.img;
    const CatCopies *skip_out = f.skip_out, *cat_in = f.cat_in, *pool_copies = f.pool_copies;
    const float* x0 = pre ? pre->x0 : nullptr;
    const Site& s1 = c->sites[rb.s1];
    const Site& s2 = c->sites[rb.s2];
    const long HW = (long)H * W;
    ConvArgs p;
    p.in = x; p.in_bs = x_bs; p.Cin = rb.cin; p.w = im.f32(W1); p.Nw = rb.cout; p.N = rb.cout;
    p.pro_scale = c->bn_scale + s1.off; p.pro_shift = shift + s1.off; p.pro_shift_bs = c->n_shift;
    p.epi_scale = c->bn_scale + s2.off; p.epi_shift = shift + s2.off; p.epi_shift_bs = c->n_shift;
    p.out = a2; p.out_bs = rb.cout * HW; p.B = B; p.H = H; p.W = W;
    if (x0) {
        p.in = x0; p.in_bs = HW;
        p.pre_w = pre->w; p.pre_b = pre->b;
    }
    p.w_wino = im.f32(U1); p.w_wino4 = im.f32(U1F);
    p.w_bf16 = im.p[B1]; p.w_bf16_lo = im.p[B1L];
    // bf16 modes: the block's form, and which of the call site's hand-overs it admits (conv_route.h).  lass_separate planned
    // them for producer and consumer at once; one that the block does not admit would have a launch read f32 storage as bf16
    // units, or the reverse
    const BlockIO io = block_io(x, x_bs, f);
    const BlockShape shape{rb.cin, rb.cout, rb.width};
    const Bf16Block bb = plan_bf16_block(c->cfg, shape, H, W, io);
    if (bb.cat_in != io.cat_in || bb.skip_out != io.skip_out || bb.pool_copies != io.pool_copies || bb.act_out != io.act_out ||
        (bb.form == BF16_DEC6U) != (io.up_cin != 0))
        return fail(c, LASS_ERR_STATE, rb.prefix + ": the launch arguments contradict the planned route");
    const bool bf1 = bb.form != BF16_NONE;
    // ... the intermediate a2 is then kept as blocked bf16 (hi, and lo for the split mode) in the same scratch
    void* a2_hi = a2;
    void* a2_lo = c->cfg.mode == MODE_BF16X3 ? (void*)((char*)a2 + (size_t)B * rb.cout * HW * 2) : nullptr;
    if (bf1) { p.out_bf16 = a2_hi; p.out_bf16_lo = a2_lo; }
    if (cat_in) p.in_bf16 = cat_in->act;
    // f32: the route of both convs and of the shortcut, decided once (conv_route.h); its workspace is checked here, in front of the
    // block's first launch
    const BlockRoute rt = bf1 ? BlockRoute() : plan_block(c->cfg, shape, B, H, W, io);
    // ... and so are the images the route reads (weight_plan.h), once for the block
    if (const SlotSet miss = missing_images(c, &im, bb.form == BF16_DEC6U ? &c->up_img[5] : nullptr,  // (decoder_block6's own)
                                            bf1 ? route_images(bb, bf16_block_weights(c->cfg, rb.cin, rb.cout)) : route_images(rt)))
        return fail(c, LASS_ERR_STATE, rb.prefix + (miss == slots(WSC3) ? " shortcut: the split weights of the planned route are missing"
                                                                        : ": the launch arguments contradict the planned route"));
    const size_t xn = rb.cin * HW, on = rb.cout * HW;  // floats per clip of the input, and of the intermediate and the output
    if (rt.kpart_floats) {
        if (!f.kpart) return fail(c, LASS_ERR_STATE, "split-K needs its partial workspace");
        if (overlaps(B, f.kpart, 0, rt.kpart_floats, x, x_bs, xn) || overlaps(B, f.kpart, 0, rt.kpart_floats, a2, on, on) ||
            overlaps(B, f.kpart, 0, rt.kpart_floats, out, out_bs, on))
            return fail(c, LASS_ERR_STATE, "the split-K partials must not overlap the block's input, intermediate or output");
    }
    if (rt.v_floats) {  // the slot holds one conv's image at a time, in stream order
        if (!f.vws || f.vws_floats < rt.v_floats) return fail(c, LASS_ERR_STATE, "the V-from-memory route needs its image workspace");
        if (overlaps(B, f.vws, 0, rt.v_floats, x, x_bs, xn) || overlaps(B, f.vws, 0, rt.v_floats, a2, on, on) ||
            overlaps(B, f.vws, 0, rt.v_floats, out, out_bs, on) || overlaps(B, f.vws, 0, rt.v_floats, f.kpart, 0, rt.kpart_floats))
            return fail(c, LASS_ERR_STATE, "the V image must not overlap the block's input, intermediate, output or split-K partials");
    }
    if (rt.m_floats) {  // ... and so does the M slot of the gemm route
        if (!f.mws || f.mws_floats < rt.m_floats) return fail(c, LASS_ERR_STATE, "the gemm route needs its product-image workspace");
        if (overlaps(B, f.mws, 0, rt.m_floats, x, x_bs, xn) || overlaps(B, f.mws, 0, rt.m_floats, a2, on, on) ||
            overlaps(B, f.mws, 0, rt.m_floats, out, out_bs, on) || overlaps(B, f.mws, 0, rt.m_floats, f.kpart, 0, rt.kpart_floats) ||
            overlaps(B, f.mws, 0, rt.m_floats, f.vws, 0, rt.v_floats))
            return fail(c, LASS_ERR_STATE, "the product image must not overlap the block's input, intermediate, output or other workspaces");
        if (f.pool_out) {
            const size_t pn = on / ((size_t)f.pool_h * 2);
            if (overlaps(B, f.mws, 0, rt.m_floats, f.pool_out, f.pool_bs ? f.pool_bs : (long)pn, pn))
                return fail(c, LASS_ERR_STATE, "the product image must not overlap the block's pooled output");
        }
    }
    if (f.planes) {  // the plan decided the route for three launches at once: a block that cannot follow it would leave the head
                     // with planes nobody wrote
        if (!rt.conv2.head_sc_fold) return fail(c, LASS_ERR_STATE, rb.prefix + ": the head's shortcut planes contradict the block's route");
        const size_t pn = (size_t)3 * HW;
        for (const float* pl : {(const float*)f.planes->skip, (const float*)f.planes->up})
            if (overlaps(B, pl, pn, pn, x, x_bs, xn) || overlaps(B, pl, pn, pn, a2, on, on) || overlaps(B, pl, pn, pn, out, out_bs, on) ||
                overlaps(B, pl, pn, pn, f.kpart, 0, rt.kpart_floats) || overlaps(B, pl, pn, pn, f.vws, 0, rt.v_floats))
                return fail(c, LASS_ERR_STATE, "the head's shortcut planes must not overlap the block's tensors or workspaces");
        if (overlaps(B, f.planes->skip, pn, pn, f.planes->up, pn, pn)) return fail(c, LASS_ERR_STATE, "the two sets of shortcut planes overlap");
    }
    Wino4Split sk;  // both convs of the block
    if (rt.kpart_floats) { sk.n = std::max(rt.conv1.splits, rt.conv2.splits); sk.part = f.kpart; }
    ConvArgs q;
    q.in = a2; q.in_bs = rb.cout * HW; q.Cin = rb.cout; q.w = im.f32(W2); q.Nw = rb.cout; q.N = rb.cout;
    q.out = out; q.out_bs = out_bs; q.B = B; q.H = H; q.W = W;
    q.pool_out = f.pool_out; q.pool_h = f.pool_h; q.pool_bs = f.pool_bs;
    q.w_wino = im.f32(U2); q.w2_wino = im.f32(USC); q.w_wino4 = im.f32(U2F);
    if (const MaskHead* mh = f.head) {  // the block output is consumed by the fused head and never written
        q.out = nullptr;
        q.mask_w = rawp(c, "base.after_conv.weight"); q.mask_b = rawp(c, "base.after_conv.bias");
        q.mask_mag = mh->mag; q.mask_cos = mh->cosv; q.mask_sin = mh->sinv;
        q.mask_re = mh->oreal; q.mask_im = mh->oimag; q.mask_T = mh->T; q.mask_nbins = mh->nbins;
    }
    q.w_bf16 = im.p[B2]; q.w2_bf16 = im.p[BSC16]; q.w_bf16_lo = im.p[B2L]; q.w2_bf16_lo = im.p[BSCL];
    if (bf1) { q.in_bf16 = a2_hi; q.in_bf16_lo = a2_lo; }
    if (cat_in) q.in2_bf16 = cat_in->raw;
    if (pool_copies) {  // bf16 mode: the pooled output as blocked bf16 copies for the next encoder block
        q.pool_out = nullptr;
        q.pool_bf16 = pool_copies->raw; q.pool_bf16_act = pool_copies->act;
        q.pool_oct0 = f.cofs / 8; q.pool_noct = pool_copies->noct;
        q.pool_act_scale = pool_copies->scale + f.cofs; q.pool_act_shift = pool_copies->shift + f.cofs; q.act_shift_bs = c->n_shift;
    }
    if (const Site* act_out = f.act_out) {  // bf16 mode: the block output goes to the next transposed conv only - written as
                                            // ONE blocked bf16 tensor with that conv's BN+FiLM+leaky prologue already applied
                                            // (in `out`'s storage)
        q.out_bf16 = out; q.out = nullptr; q.out_oct0 = 0; q.out_noct = 0;
        q.epi_scale = c->bn_scale + act_out->off; q.epi_shift = shift + act_out->off; q.epi_shift_bs = c->n_shift;
    }
    if (skip_out) {  // the skip goes out as the two blocked copies (concat channels [C, 2C)) instead of f32
        q.out = nullptr;
        q.out_bf16 = skip_out->raw; q.out_bf16_act = skip_out->act;
        q.out_oct0 = (rb.cout + f.cofs) / 8; q.out_noct = skip_out->noct;
        q.act_scale = skip_out->scale + rb.cout + f.cofs; q.act_shift = skip_out->shift + rb.cout + f.cofs; q.act_shift_bs = c->n_shift;
    }
    if (rb.cin == rb.cout) {
        q.res = x; q.res_bs = x_bs;
        if (x0) {
            q.res = x0; q.res_bs = HW;
            q.pre_w = pre->w; q.pre_b = pre->b;
        }
    } else {
        q.in2 = x; q.in2_bs = x_bs; q.Cin2 = rb.cin; q.w2 = im.f32(WSC); q.bias = rawp(c, rb.prefix + ".shortcut.bias");
    }
    if (bf1) return run_resblock_bf16(c, rb, bb.form, p, q, B, st, f);
    if (rt.conv2.head_fold) {  // the composed images in place of conv2's, the shortcut's and after_conv's
        q.w_wino4 = im.f32(U2H); q.w2 = im.f32(WSCH); q.bias = im.f32(BH);
        q.mask_w = q.mask_b = nullptr;
    }
    if (rt.shortcut_gemm) {
        // the GEMM writes bias + Wsc x into the block's output slot; conv2 then adds its result to that slot in place
        if (overlaps(B, out, out_bs, on, x, x_bs, xn) || overlaps(B, out, out_bs, on, a2, on, on))
            return fail(c, LASS_ERR_STATE, "a block's output must not overlap its input or its intermediate");
        if (rt.conv2.family == CONV_NONE) return fail(c, LASS_ERR_STATE, "conv2 with the shortcut as residual");
        if (!lass_pw_gemm_supported(CONV2_SHORTCUT, q))
            return fail(c, LASS_ERR_STATE, rb.prefix + " shortcut: the launch arguments contradict the planned route");
        PwSplitW sw;
        if (rt.pw_split) sw.w = im.p[WSC3];
        {
            ProfScope ps(c, st, P_CONV3X3);
            HIP_TRY(c, lass_launch_pw_gemm(CONV2_SHORTCUT, q, st, sw));
        }
        q.in2 = nullptr; q.in2_bs = 0; q.Cin2 = 0; q.w2 = nullptr; q.bias = nullptr;
        q.res = out; q.res_bs = out_bs;
    }
    Wino4Gemm g1, g2;
    g1.w3 = im.p[U1G]; g2.w3 = im.p[U2G];
    g1.m = g2.m = f.mws;
    if (int r = launch_routed(c, rb, "conv1", rt.conv1, p, sk, f.vws, g1, st)) return r;
    return launch_routed(c, rb, "conv2", rt.conv2, q, sk, f.vws, g2, st, f.planes);
}

int run_upconv(lass_ctx* c, int di, const float* x, int B, int h, int w, const float* shift, float* out, long out_bs,
               hipStream_t st, const CatCopies* cb = nullptr, bool x_is_act_bf16 = false, const HeadScPlanes* planes = nullptr) {
    const DecSpec& d = c->m.D[di];
    const Site& s = c->sites[c->dec_site[di]];
    ConvArgs p;
    p.in = x; p.in_bs = (long)d.cin * h * w; p.Cin = d.cin;
    p.w = rawp(c, std::string("base.") + d.name + ".conv1.weight");  // (cin, cout, uh, uw) == [cin][n], n=(co,a,bb)
    p.N = p.Nw = d.cout * d.uh * d.uw;
    p.pro_scale = c->bn_scale + s.off; p.pro_shift = shift + s.off; p.pro_shift_bs = c->n_shift;
    p.out = out; p.out_bs = out_bs; p.B = B; p.H = h; p.W = w; p.up_h = d.uh;
    p.w_bf16 = c->up_img[di].p[UP16]; p.w_bf16_lo = c->up_img[di].p[UP16L];
    // the family, and which of the call site's hand-overs it admits (conv_route.h: plan_upconv)
    UpSite site;
    site.in_act = x_is_act_bf16; site.out_copies = cb != nullptr; site.logits = planes != nullptr;
    site.aligned = p.in_bs % 4 == 0 && p.out_bs % 2 == 0 && ((uintptr_t)p.in & 15u) == 0 && ((uintptr_t)p.w & 15u) == 0 && ((uintptr_t)p.out & 7u) == 0;
    const UpRoute rt = plan_upconv(c->cfg, d, h, w, site);
    bool ok = rt.in_act == site.in_act && rt.out_copies == site.out_copies && (rt.family == UP_LOGITS) == site.logits;
    if (rt.in_act) p.in_bf16 = x;  // the producer already applied this conv's prologue and wrote blocked bf16
    if (rt.out_copies) {           // concat channels [0, C) as the two blocked copies instead of f32
        p.out = nullptr;
        p.out_bf16 = cb->raw; p.out_bf16_act = cb->act; p.out_oct0 = 0; p.out_noct = cb->noct;
        p.act_scale = cb->scale; p.act_shift = cb->shift; p.act_shift_bs = c->n_shift;
    }
    ok = ok && !missing_images(c, nullptr, &c->up_img[di], route_images(rt, c->cfg));  // the images the route reads (weight_plan.h)
    if (ok && rt.family == UP_LOGITS) ok = lass_tconv_logits_supported(p, *planes);
    PwSplitW sw;
    if (rt.pw_split) sw.w = c->up_img[di].p[UP3];
    if (ok && rt.family == UP_GEMM) ok = lass_pw_gemm_supported(TCONV_ACT, p);
    if (!ok || rt.family == UP_INSIDE)
        return fail(c, LASS_ERR_STATE, std::string(d.name) + " transposed conv: the launch arguments contradict the planned route");
    ProfScope ps(c, st, P_TCONV);
    switch (rt.family) {
        case UP_LOGITS:  // decoder_block6 of the head_sc_fold route: the launch also writes the head's shortcut logits of its output
            HIP_TRY(c, lass_launch_tconv_logits(p, *planes, st));
            break;
        case UP_BF16:
            HIP_TRY(c, lass_launch_conv_bf16(TCONV_ACT, p, st));
            break;
        case UP_GEMM:
            HIP_TRY(c, lass_launch_pw_gemm(TCONV_ACT, p, st, sw));
            break;
        default:
            HIP_TRY(c, lass_launch_conv(TCONV_ACT, p, st));
            break;
    }
    return 0;
}

// ---- workspace plan ---------------------------------------------------------------------------------------------
// What workspace_plan.h's rules read of a context
// (head_sc_weights: the rule, and - a composition can decline - the images are really there)
PlanInputs plan_inputs(const lass_ctx* c) {
    const bool head_sc = head_sc_weights(c->cfg, c->m, c->head_rows) && !missing_images(c, nullptr, nullptr, slots(HS_WT, HS_WSKIP));
    return PlanInputs{c->g, c->m, c->cfg, c->n_shift, head_sc};
}
Plan make_plan(const lass_ctx* c, int B, int L) { return make_plan(plan_inputs(c), B, L); }
CallPlan plan_call(const lass_ctx* c, int B, int L, bool capturing, size_t workspace_bytes) {
    return plan_call(plan_inputs(c), B, L, c->split_batch, c->profiling, capturing, workspace_bytes);
}

// Every entry that launches or allocates runs on the context's device, whatever the caller's current device is.
int use_device(lass_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    return 0;
}

int check_ready(lass_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    if (!c->finalized) return fail(c, LASS_ERR_STATE, "lass_finalize has not been called (or a parameter changed since)");
    return use_device(c);
}

// Destroys every instantiated graph (live and retired).  Caller has synchronised the device.
void drop_graphs(lass_ctx* c) {
    for (hipGraphExec_t x : c->graphs.take_all()) (void)hipGraphExecDestroy(x);
}

// Stage calls have no workspace plan: their split-K partials and their V image live in two buffers of the context that grow on
// demand (the call must not be under stream capture when one does).  hipFree waits for the launches that still use the old buffer.
int stage_scratch(lass_ctx* c, const ResBlock& rb, int B, int H, int W, const float* x, BlockFusions* f) {
    const BlockRoute rt = plan_block(c->cfg, BlockShape{rb.cin, rb.cout, rb.width}, B, H, W, block_io(x, (long)rb.cin * H * W, *f));
    const auto grow = [&](float** buf, size_t* have, size_t need) -> int {
        if (need <= *have) return 0;
        if (*buf) HIP_TRY(c, hipFree(*buf));
        *buf = nullptr;
        *have = 0;
        HIP_TRY(c, hipMalloc((void**)buf, need * sizeof(float)));
        *have = need;
        return 0;
    };
    if (int r = grow(&c->stage_part, &c->stage_part_floats, rt.kpart_floats)) return r;
    if (rt.kpart_floats) f->kpart = c->stage_part;
    // ... and the V image of the V-from-memory layers: the caller's buffer if one is set (lass_set_wino4_vprep_buffer), as it is
    if (!c->stage_v_user)
        if (int r = grow(&c->stage_v, &c->stage_v_floats, rt.v_floats)) return r;
    if (rt.v_floats) {
        f->vws = c->stage_v_user ? c->stage_v_user : c->stage_v;
        f->vws_floats = c->stage_v_user ? c->stage_v_user_floats : c->stage_v_floats;
    }
    if (int r = grow(&c->stage_m, &c->stage_m_floats, rt.m_floats)) return r;
    if (rt.m_floats) { f->mws = c->stage_m; f->mws_floats = c->stage_m_floats; }
    return 0;
}

// The transform size of the weight-free stage calls (lass_stft_magphase, lass_istft): a ResUNet30 context's own; the multi-STFT
// model's context keeps the reference layout's 1024 there (its own transforms go through the *_nfft / *_components calls)
int stage_nfft(const lass_ctx* c) { return c->g.variant == 0 ? c->g.nfft : LASS_NFFT; }

// iSTFT transform sizes of a context: 1024 or 2048 at hop 160, 2048 alone at hop 320 (stft.hip instantiates no other pair)
bool istft_nfft_ok(const lass_ctx* c, int n_fft) { return n_fft == 2048 || (n_fft == 1024 && c->g.hop == LASS_HOP); }

const ResBlock* find_block(const lass_ctx* c, const std::string& prefix) {
    for (const auto& rb : c->enc) if (rb.prefix == prefix) return &rb;
    for (const auto& rb : c->dec) if (rb.prefix == prefix) return &rb;
    return nullptr;
}

// scale[c] = g / sqrt(var + eps), base[c] = beta - mean * scale of the BatchNorm `bn` of the checkpoint
hipError_t launch_bnfold(const lass_ctx* c, const std::string& bn, int C, float* scale, float* base, hipStream_t st) {
    return lass_launch_bnfold(rawp(c, bn + ".weight"), rawp(c, bn + ".bias"), rawp(c, bn + ".running_mean"), rawp(c, bn + ".running_var"), C,
                              kBnEps, scale, base, st);
}

int upload(lass_ctx* c, const std::vector<float>& v, void** slot) {
    float* d = nullptr;
    if (dev_alloc(c, &d, v.size())) return LASS_ERR_HIP;
    HIP_TRY(c, hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    *slot = d;
    return 0;
}

// The folded head's images (weight_plan.h: WF_HEAD_*): decoder_block6's conv2 and shortcut composed with after_conv, and (sc) the
// shortcut's two halves for the launches that produce its inputs - Wt' = Wsc'_up o Wt for the transposed conv, Wsc'_skip for
// encoder_block1.conv2's epilogue (head_fold.h).  A composition that declines leaves its vectors empty.
struct HeadHost {
    HeadFold hf;
    HeadScFold hsf;
    const std::vector<float>& of(WeightForm f) const {
        return f == WF_HEAD_U4 ? hf.u4 : f == WF_HEAD_WSC ? hf.wsc : f == WF_HEAD_BIAS ? hf.bias : f == WF_HEAD_SC_WT ? hsf.wt : hsf.wskip;
    }
};
int compose_head(lass_ctx* c, int Q, bool sc, HeadHost* h) {
    const ResBlock& rb = c->dec[5];
    const DecSpec& d6 = c->m.D[5];
    const int N = rb.cout, K = rb.cin;
    std::vector<float> w2, ws, bs, wa, ba, wt;
    const auto host = [&](std::vector<float>& v, const std::string& name, size_t n) -> int {
        v.resize(n);
        HIP_TRY(c, hipMemcpy(v.data(), rawp(c, name), n * sizeof(float), hipMemcpyDeviceToHost));
        return 0;
    };
    HIP_TRY(c, hipStreamSynchronize(nullptr));  // lass_finalize's stream: the one wait in front of the host reads
    if (host(w2, rb.prefix + ".conv2.weight", (size_t)N * N * 9) || host(ws, rb.prefix + ".shortcut.weight", (size_t)N * K) ||
        host(bs, rb.prefix + ".shortcut.bias", N) || host(wa, "base.after_conv.weight", (size_t)Q * N) ||
        host(ba, "base.after_conv.bias", Q) ||
        (sc && host(wt, std::string("base.") + d6.name + ".conv1.weight", (size_t)d6.cin * d6.cout * d6.uh * d6.uw)))
        return LASS_ERR_HIP;
    if (sc) compose_head_sc_fold(ws.data(), wa.data(), wt.data(), N, d6.cout, kPreCh, Q, d6.cin, d6.uh, d6.uw, &h->hsf);
    if (!compose_head_fold(w2.data(), ws.data(), bs.data(), wa.data(), ba.data(), N, N, K, Q, &h->hf) || h->hf.u4.empty()) h->hf = HeadFold();
    return 0;
}

}  // namespace

extern "C" {

int lass_version(void) { return 11000; }  // 1.10.0: linked channels (lass_separate_ragged_linked, lass_separate_windows_linked, lass_masked_stft, lass_masked_stft_windows); 1.9.0: EBU R 128 figures (lass_resample_true_peak, lass_loudness_stats); 1.8.0: levelled export (lass_loudness, lass_resample_peak, lass_loudness_gain, lass_resample_encode_gain); 1.7.0: cross-faded window seams (lass_separate_windows_faded, lass_istft_windows_faded); 1.6.0: ResUNet30 at the (2048, 320) STFT geometry (lass_create_stft, lass_stft_geometry); 1.5.0: windows of one long row (lass_separate_windows & co); 1.4.0: per-clip lengths (lass_separate_ragged & co); 1.3.0: CLAP text tower (lass_text_*, text.hip); 1.2.0: F(4x4,3x3) kernels, lass_set_graph_replay (1.1.0: multi-STFT model, fused iSTFT, graph replay)

const char* lass_last_error(const lass_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

static int create_impl(lass_ctx** out, int device_id, const Geometry& geom) {
    if (!out) return LASS_ERR_ARG;
    *out = nullptr;
    if (int rc = open_device(device_id, g_create_err)) return rc;
    lass_ctx* c = new lass_ctx();
    c->device = device_id;
    c->g = geom;
    if (const char* e = getenv("LASS_FUSE_CATB")) c->cfg.fuse_catb = atoi(e) != 0;
    if (const char* e = getenv("LASS_FUSE_BLOCK")) c->cfg.fuse_block = atoi(e) != 0;
    if (const char* e = getenv("LASS_FUSE_UP")) c->cfg.fuse_up = atoi(e) != 0;
    if (const char* e = getenv("LASS_WINO4")) c->cfg.wino4_mincin = atoi(e);
    if (const char* e = getenv("LASS_WINO4_VPREP")) c->cfg.vprep_mode = std::max(0, std::min(2, atoi(e)));  // A/B: lass_set_wino4_vprep
    if (const char* e = getenv("LASS_HEAD_FOLD")) c->cfg.head_fold = atoi(e) != 0;  // A/B: lass_set_head_fold
    if (const char* e = getenv("LASS_HEAD_SC_FOLD")) c->cfg.head_sc_fold = atoi(e) != 0;  // A/B: lass_set_head_sc_fold
    if (const char* e = getenv("LASS_PW_SPLIT")) c->cfg.pw_split = atoi(e) != 0;  // A/B: lass_set_pw_split
    if (const char* e = getenv("LASS_WINO4_GEMM")) c->cfg.wino4_gemm = atoi(e) != 0;  // A/B: lass_set_wino4_gemm
    if (const char* e = getenv("LASS_SPLIT")) c->split_batch = std::max(0, std::min(2, atoi(e)));
    if (const char* e = getenv("LASS_GRAPH")) c->use_graph = atoi(e) != 0;
    c->prof.resize(P_COUNT);
    for (int i = 0; i < P_COUNT; ++i) c->prof[i].name = kProfNames[i];
    build_arch(c);
    if (hipSetDevice(device_id) != hipSuccess) {
        g_create_err = "hipSetDevice failed";
        delete c;
        return LASS_ERR_HIP;
    }
    // FFT twiddles (the periodic Hann windows are read off the same table), evaluated in double on the host.
    std::vector<float2> tw2k(2048);
    for (int k = 0; k < 2048; ++k) {
        const double a = 2.0 * M_PI * k / 2048.0;
        tw2k[k] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    if (hipMalloc((void**)&c->tw2k, sizeof(float2) * 2048) != hipSuccess ||
        hipMemcpy(c->tw2k, tw2k.data(), sizeof(float2) * 2048, hipMemcpyHostToDevice) != hipSuccess) {
        g_create_err = "allocating FFT tables failed";
        delete c;
        return LASS_ERR_HIP;
    }
    *out = c;
    return 0;
}

int lass_create(lass_ctx** out, int device_id) { return create_impl(out, device_id, Geometry()); }

int lass_create_stft(lass_ctx** out, int device_id, int n_fft, int hop) {
    if (!out) return LASS_ERR_ARG;
    *out = nullptr;
    Geometry g;  // (1024, 160): exactly lass_create
    if (n_fft == 2048 && hop == 320) {
        g.nfft = 2048; g.nbins = 1025; g.fcrop = 1024; g.hop = 320; g.wins[0] = 2048;
    } else if (n_fft != LASS_NFFT || hop != LASS_HOP) {
        g_create_err = "lass_create_stft: (n_fft, hop) must be (1024, 160) or (2048, 320), got (" + std::to_string(n_fft) + ", " +
                       std::to_string(hop) + ")";
        return LASS_ERR_ARG;
    }
    return create_impl(out, device_id, g);
}

int lass_stft_geometry(const lass_ctx* c, int* n_fft, int* hop) {
    if (!c) return LASS_ERR_ARG;
    if (n_fft) *n_fft = c->g.nfft;
    if (hop) *hop = c->g.hop;
    return 0;
}

int lass_create_multistft(lass_ctx** out, int device_id, int n_fft, int n_windows, const int* win_lengths,
                          int mask_window) {
    if (!out) return LASS_ERR_ARG;
    *out = nullptr;
    Geometry g;
    g.variant = 1;
    g.magphase_sem = 1;
    if (n_fft != 2048 || n_windows < 1 || n_windows > kMaxBranches || !win_lengths) {
        g_create_err = "lass_create_multistft: n_fft must be 2048 and 1 <= n_windows <= 4";
        return LASS_ERR_ARG;
    }
    g.nfft = n_fft; g.nbins = n_fft / 2 + 1; g.fcrop = n_fft / 2; g.nbr = n_windows; g.mask_br = -1;
    for (int k = 0; k < n_windows; ++k) {
        const int w = win_lengths[k];
        if (w < 32 || w > n_fft || (2048 % w) != 0) {
            g_create_err = "lass_create_multistft: window lengths must be powers of two in [32, n_fft]";
            return LASS_ERR_ARG;
        }
        for (int j = 0; j < k; ++j)
            if (g.wins[j] == w) {
                g_create_err = "lass_create_multistft: duplicate window length";
                return LASS_ERR_ARG;
            }
        g.wins[k] = w;
        if (w == mask_window) g.mask_br = k;
    }
    if (g.mask_br < 0) {
        g_create_err = "lass_create_multistft: mask_window is not one of the analysis windows";
        return LASS_ERR_ARG;
    }
    return create_impl(out, device_id, g);
}

int lass_destroy(lass_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    (void)hipSetDevice(c->device);
    free_owned(c);
    c->raw.free_all();
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    (void)hipDeviceSynchronize();  // no replay of a graph below is in flight any more
    drop_graphs(c);
    if (c->g_stream) (void)hipStreamDestroy(c->g_stream);
    if (c->s2) (void)hipStreamDestroy(c->s2);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    (void)hipFree(c->tw2k);
    (void)hipFree(c->stage_part);
    (void)hipFree(c->stage_v);
    (void)hipFree(c->stage_m);
    delete c;
    return 0;
}

int lass_set_param(lass_ctx* c, const char* name_c, const void* data, const int64_t* shape, int ndim, int dtype) {
    if (!c || !name_c || !data || ndim < 0 || (ndim > 0 && !shape)) return fail(c, LASS_ERR_ARG, "bad argument");
    const std::string name(name_c);
    std::vector<int64_t> want = expected_shape(c, name);
    if (want.empty()) {
        if (ignorable(name)) return 1;
        return fail(c, LASS_ERR_ARG, "unknown parameter '" + name + "'");
    }
    if (dtype != LASS_F32) return fail(c, LASS_ERR_ARG, "parameter '" + name + "' must be float32");
    std::vector<int64_t> got(shape, shape + ndim);
    if (got != want) {
        std::string m = "shape mismatch for '" + name + "': got (";
        for (auto v : got) m += std::to_string(v) + ",";
        m += ") want (";
        for (auto v : want) m += std::to_string(v) + ",";
        return fail(c, LASS_ERR_ARG, m + ")");
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = c->raw.put(c, name, data, shape, ndim)) return rc;
    c->finalized = false;
    return 0;
}

int lass_finalize(lass_ctx* c, int compute_mode) {
    if (!c) return LASS_ERR_ARG;
    if (compute_mode != LASS_COMPUTE_F32 && compute_mode != LASS_COMPUTE_BF16 && compute_mode != LASS_COMPUTE_BF16X3)
        return fail(c, LASS_ERR_ARG, "unsupported compute mode");
    c->last_split.clear();
    c->cfg.mode = (ComputeMode)compute_mode;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipDeviceSynchronize());  // replays of graphs that hold the old derived buffers have drained
    drop_graphs(c);
    free_owned(c);  // ... and with the storage goes every pointer to it: a second finalize in another mode starts from no image
    for (auto* blocks : {&c->enc, &c->dec})
        for (ResBlock& rb : *blocks) rb.img = WeightImages();
    for (WeightImages& u : c->up_img) u = WeightImages();
    c->img = WeightImages();
    c->head_rows = 0;
    c->finalized = false;
    c->err.clear();
    hipStream_t st = nullptr;
    // -- every parameter is there: the first one missing, in this order, is the error
    const auto need = [&](const std::string& p, std::initializer_list<const char*> fields) {
        for (const char* f : fields)
            if (!rawp(c, p + f) && c->err.empty()) c->err = "missing parameter '" + p + f + "'";
    };
    const auto bn = {".weight", ".bias", ".running_mean", ".running_var"}, wb = {".weight", ".bias"};
    for (const Site& s : c->sites) { need(s.bn, bn); need("film." + s.film, wb); }
    need("base.bn0", bn);
    for (int k = 0; k < c->g.nbr; ++k) need(c->pre_name[k], wb);
    need("base.after_conv", wb);
    for (const auto* blocks : {&c->enc, &c->dec})
        for (const ResBlock& rb : *blocks) {
            need(rb.prefix, {".conv1.weight", ".conv2.weight"});
            if (rb.cin != rb.cout) need(rb.prefix, {".shortcut.weight", ".shortcut.bias"});
        }
    for (const DecSpec& d : c->m.D) need(std::string("base.") + d.name, {".conv1.weight"});
    if (!c->err.empty()) return LASS_ERR_STATE;
    // -- BN folding for the 32 live sites + bn0, FiLM concatenation
    if (dev_alloc(c, &c->bn_scale, c->n_shift) || dev_alloc(c, &c->bn_base, c->n_shift) ||
        dev_alloc(c, &c->film_W, (size_t)c->n_shift * LASS_COND) || dev_alloc(c, &c->film_b, c->n_shift) ||
        dev_alloc(c, &c->bn0_s, c->g.nbins) || dev_alloc(c, &c->bn0_h, c->g.nbins))
        return LASS_ERR_HIP;
    for (const Site& s : c->sites) {
        HIP_TRY(c, launch_bnfold(c, s.bn, s.C, c->bn_scale + s.off, c->bn_base + s.off, st));
        HIP_TRY(c, hipMemcpyAsync(c->film_W + (size_t)s.off * LASS_COND, rawp(c, "film." + s.film + ".weight"),
                                  (size_t)s.C * LASS_COND * sizeof(float), hipMemcpyDeviceToDevice, st));
        HIP_TRY(c, hipMemcpyAsync(c->film_b + s.off, rawp(c, "film." + s.film + ".bias"), s.C * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(c, launch_bnfold(c, "base.bn0", c->g.nbins, c->bn0_s, c->bn0_h, st));
    // -- the weight images: weight_plan.h says which, in which form and from what; every launcher below writes `count` elements
    const Param* ra = c->raw.find("base.after_conv.weight");
    if (!ra->shape.empty() && ra->n == (size_t)ra->shape[0] * c->dec[5].cout) c->head_rows = (int)ra->shape[0];
    const ResBlock& rb6 = c->dec[5];
    const DecSpec& d6 = c->m.D[5];
    HeadHost head;
    bool composed = false;
    for (const WeightItem& it : plan_weights(c->cfg, c->m, c->head_rows)) {
        ResBlock* rb = it.owner != OWN_BLOCK ? nullptr : it.index < (int)c->enc.size() ? &c->enc[it.index] : &c->dec[it.index - c->enc.size()];
        WeightImages& im = rb ? rb->img : it.owner == OWN_DECODER ? c->up_img[it.index] : c->img;
        // the owner's prefix of checkpoint names: the block's, or its decoder's (the context's images are decoder_block6's)
        const std::string prefix = rb ? rb->prefix + "." : std::string("base.") + c->m.D[it.owner == OWN_DECODER ? it.index : 5].name + ".";
        const float* src = it.param ? rawp(c, prefix + it.param) : it.from >= 0 ? im.f32((WeightSlot)it.from) : nullptr;
        if (weight_form_on_host(it.form)) {  // in double on the host, from the checkpoint alone
            if (!composed && compose_head(c, c->head_rows, head_sc_weights(c->cfg, c->m, c->head_rows), &head)) return LASS_ERR_HIP;
            composed = true;
            const std::vector<float>& v = head.of(it.form);
            if (v.empty()) continue;  // the composition declined: no image, and the route is off
            if (v.size() != it.count) return fail(c, LASS_ERR_STATE, "lass_finalize: a head composition contradicts the weight plan");
            if (int r = upload(c, v, &im.p[it.slot])) return r;
            continue;
        }
        char* dst = nullptr;
        if (dev_alloc(c, &dst, it.count * it.elem_bytes)) return LASS_ERR_HIP;
        float* dstf = (float*)dst;
        switch (it.form) {
            case WF_RELAYOUT: HIP_TRY(c, lass_launch_relayout_conv(src, it.rows, it.cols, it.taps, dstf, st)); break;
            case WF_F2X2: HIP_TRY(c, lass_launch_wino_weights(src, it.rows, it.cols, dstf, st)); break;
            case WF_F2X2_SC: HIP_TRY(c, lass_launch_wino_shortcut_weights(src, it.rows, it.cols, dstf, st)); break;
            case WF_F4X4: HIP_TRY(c, lass_launch_wino4_weights(src, it.rows, it.cols, dstf, st)); break;
            case WF_F4X4_SPLIT3: HIP_TRY(c, lass_launch_wino4_gemm_weights(src, it.rows, it.cols, dst, st)); break;
            case WF_PW_SPLIT3: HIP_TRY(c, lass_launch_pw_split_weights(src, it.rows, it.cols, dst, st)); break;
            case WF_UP_SC:
                HIP_TRY(c, lass_launch_compose_up_shortcut(rawp(c, rb6.prefix + ".shortcut.weight"), rawp(c, prefix + "conv1.weight"), d6.cin,
                                                           d6.cout, rb6.cin, rb6.cout, dstf, st));
                break;
            case WF_BF16: case WF_BF16_LO: case WF_BF16_T: case WF_BF16_T_LO:
                HIP_TRY(c, lass_launch_weights_bf16(src, it.rows, it.cols, it.taps, dst, it.form == WF_BF16_LO || it.form == WF_BF16_T_LO,
                                                    it.form >= WF_BF16_T, st));
                break;
            default: return fail(c, LASS_ERR_STATE, "lass_finalize: a weight form without a launcher");
        }
        im.p[it.slot] = dst;
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    c->finalized = true;
    ++c->gen;  // any captured graph refers to the previous derived buffers
    return 0;
}

int lass_workspace_bytes(const lass_ctx* c, int B, int L, size_t* bytes) {
    if (!c || !bytes) return LASS_ERR_ARG;
    // (the half-batch plans side by side differ from the whole plan by alignment padding only)
    const CallPlan cp = plan_call(c, B, L, false, kNoWorkspaceLimit);
    if (!cp.whole.valid) return LASS_ERR_ARG;  // B < 1, L <= n_fft / 2 or L beyond the 32-bit per-clip addressing limit
    *bytes = cp.need;
    return 0;
}

int lass_film_width(const lass_ctx* c) { return c ? c->n_shift : LASS_ERR_ARG; }

int lass_film_offset(const lass_ctx* c, const char* site) {
    if (!c || !site) return -1;
    auto it = c->site_idx.find(site);
    return it == c->site_idx.end() ? -1 : c->sites[it->second].off;
}

int lass_film(lass_ctx* c, const float* cond, int B, float* shift, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!cond || !shift || B <= 0) return fail(c, LASS_ERR_ARG, "lass_film: bad argument");
    HIP_TRY(c, lass_launch_film(cond, B, c->film_W, c->film_b, c->bn_base, c->n_shift, shift, (hipStream_t)stream));
    return 0;
}

int lass_film_raw(lass_ctx* c, const float* cond, int B, float* film, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!cond || !film || B <= 0) return fail(c, LASS_ERR_ARG, "lass_film_raw: bad argument");
    HIP_TRY(c, lass_launch_film(cond, B, c->film_W, c->film_b, nullptr, c->n_shift, film, (hipStream_t)stream));
    return 0;
}

int lass_stft_magphase(lass_ctx* c, const float* wav, int B, int L, float* mag, float* cos_out, float* sin_out,
                       float* real_out, float* imag_out, void* stream) {
    if (!c) return LASS_ERR_ARG;
    const int n_fft = stage_nfft(c), hop = c->g.hop;  // a ResUNet30 context analyses at its own geometry
    if (!wav || B <= 0 || L <= n_fft / 2) return fail(c, LASS_ERR_ARG, "lass_stft_magphase: bad argument");
    if (int r = use_device(c)) return r;
    const int T = 1 + L / hop;
    StftBranch br;
    br.wlen = n_fft; br.mag = mag; br.cosv = cos_out; br.sinv = sin_out; br.real = real_out; br.imag = imag_out;
    HIP_TRY(c, lass_launch_stft2(wav, ClipForm{B, L}, n_fft, hop, T, T, 1, &br, 0, nullptr, nullptr, c->tw2k,
                                 (hipStream_t)stream));
    return 0;
}

int lass_stft_components(lass_ctx* c, const float* wav, int B, int L, int n_fft, int hop, int n_windows,
                         const int* win_lengths, float* const* mag, float* const* cos_out, float* const* sin_out,
                         void* stream) {
    if (!c || !wav || !win_lengths || !mag || !cos_out || !sin_out || B <= 0 || hop <= 0 || n_windows <= 0 ||
        n_windows > LASS_MAX_STFT_WINDOWS || (n_fft != 1024 && n_fft != 2048) || L <= n_fft / 2)
        return fail(c, LASS_ERR_ARG, "lass_stft_components: bad argument (n_fft 1024 or 2048, at most 4 windows, L > n_fft/2)");
    StftBranch br[LASS_MAX_STFT_WINDOWS];
    for (int i = 0; i < n_windows; ++i) {
        const int w = win_lengths[i];
        if (w < 32 || w > n_fft || (2048 % w) != 0)
            return fail(c, LASS_ERR_ARG, "lass_stft_components: window lengths must be powers of two in [32, n_fft]");
        if (!mag[i] || !cos_out[i] || !sin_out[i]) return fail(c, LASS_ERR_ARG, "lass_stft_components: null output");
        br[i].wlen = w; br[i].mag = mag[i]; br[i].cosv = cos_out[i]; br[i].sinv = sin_out[i];
    }
    if (int r = use_device(c)) return r;
    const int T = 1 + L / hop;
    HIP_TRY(c, lass_launch_stft2(wav, ClipForm{B, L}, n_fft, hop, T, T, n_windows, br, 1, nullptr, nullptr, c->tw2k,
                                 (hipStream_t)stream));
    return 0;
}

int lass_multi_stft(lass_ctx* c, const float* wav, int B, int L, int hop, int n_windows, const int* win_lengths,
                    float* const* mag, float* const* cos_out, float* const* sin_out, void* stream) {
    if (!c || !wav || !win_lengths || !mag || !cos_out || !sin_out || B <= 0 || hop <= 0 || n_windows <= 0 ||
        n_windows > LASS_MAX_STFT_WINDOWS)
        return fail(c, LASS_ERR_ARG, "lass_multi_stft: bad argument");
    for (int i = 0; i < n_windows; ++i) {
        const int N = win_lengths[i];
        if (N != 256 && N != 512 && N != 1024 && N != 2048)
            return fail(c, LASS_ERR_ARG, "lass_multi_stft: window lengths must be 256, 512, 1024 or 2048");
        if (L <= N / 2) return fail(c, LASS_ERR_ARG, "lass_multi_stft: waveform shorter than the reflect padding");
        if (!mag[i] || !cos_out[i] || !sin_out[i]) return fail(c, LASS_ERR_ARG, "lass_multi_stft: null output");
    }
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_multi_stft(wav, B, L, hop, n_windows, win_lengths, c->tw2k, mag, cos_out, sin_out,
                                      (hipStream_t)stream));
    return 0;
}

int lass_istft(lass_ctx* c, const float* real, const float* imag, int B, int T, int L, float* wav, float* frames_ws,
               void* stream) {
    (void)frames_ws;  // the fused kernel needs no frame scratch (kept in the signature for ABI stability; may be NULL)
    if (!c) return LASS_ERR_ARG;
    return lass_istft_nfft(c, real, imag, B, T, L, stage_nfft(c), stage_nfft(c), wav, stream);
}

int lass_istft_nfft(lass_ctx* c, const float* real, const float* imag, int B, int T, int L, int n_fft, int win_length,
                    float* wav, void* stream) {
    if (!c || !real || !imag || !wav || B <= 0 || T <= 0 || L <= 0 || (n_fft != 1024 && n_fft != 2048) ||
        !istft_nfft_ok(c, n_fft) || win_length < 32 || win_length > n_fft || (2048 % win_length) != 0 ||
        (long)L + n_fft / 2 > (long)(T - 1) * c->g.hop + n_fft)
        return fail(c, LASS_ERR_ARG, "lass_istft: bad argument (n_fft 1024 or 2048 - 2048 alone at hop 320 -, the frames must cover L)");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_istft2(real, imag, ClipForm{B, L}, T, n_fft, win_length, c->g.hop, c->tw2k, wav, (hipStream_t)stream));
    return 0;
}

int lass_convblock(lass_ctx* c, const char* prefix, const float* x, int B, int H, int W, const float* shift, float* y,
                   float* scratch, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!prefix || !x || !shift || !y || !scratch) return fail(c, LASS_ERR_ARG, "lass_convblock: bad argument");
    const ResBlock* rb = find_block(c, prefix);
    if (!rb) return fail(c, LASS_ERR_ARG, std::string("lass_convblock: unknown block '") + prefix + "'");
    const long HW = (long)H * W;
    BlockFusions f;
    if ((r = stage_scratch(c, *rb, B, H, W, x, &f))) return r;
    return run_resblock(c, *rb, x, rb->cin * HW, B, H, W, shift, scratch, y, rb->cout * HW, (hipStream_t)stream, f);
}

int lass_encoder_block(lass_ctx* c, const char* name, const float* x, int B, int H, int W, const float* shift, float* y,
                       float* pool, float* scratch, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!name || !x || !shift || !y || !scratch || B <= 0 || H <= 0 || W <= 0)
        return fail(c, LASS_ERR_ARG, "lass_encoder_block: bad argument");
    for (size_t bi = 0; bi < c->enc.size(); ++bi) {
        const ResBlock& rb = c->enc[bi];
        if (rb.prefix != std::string(name) + ".conv_block1") continue;
        const EncSpec& e = c->m.E[bi < (size_t)c->g.nbr ? 0 : bi - c->g.nbr + 1];
        const long HW = (long)H * W;
        const bool pooled = e.dw == 2;
        if (pooled && (!pool || W % 2 != 0)) return fail(c, LASS_ERR_ARG, "lass_encoder_block: pool output needed, W even");
        // same rule as lass_separate: the pool rides in conv2's epilogue when the rows divide, else its own kernel
        const bool fuse = pooled && (H % e.dh) == 0;
        hipStream_t st = (hipStream_t)stream;
        BlockFusions f;
        if (fuse) { f.pool_out = pool; f.pool_h = e.dh; }
        if ((r = stage_scratch(c, rb, B, H, W, x, &f))) return r;
        r = run_resblock(c, rb, x, rb.cin * HW, B, H, W, shift, scratch, y, rb.cout * HW, st, f);
        if (r) return r;
        if (pooled && !fuse) HIP_TRY(c, lass_launch_pool(y, rb.cout * HW, B, rb.cout, H, W, e.dh, e.dw, pool, st));
        return 0;
    }
    return fail(c, LASS_ERR_ARG, std::string("lass_encoder_block: unknown encoder '") + name + "'");
}

// The front end of the network for the clips of cf, one launch for all analysis branches: x0[k] (B, Tp, fcrop) of branch k,
// mag / cos / sin of the mask branch alone.
static hipError_t launch_front_end(lass_ctx* c, const float* wav, const ClipForm& cf, float* const* x0, float* mag, float* cosv,
                                   float* sinv, hipStream_t st) {
    const Geometry& g = c->g;
    const int T = 1 + cf.L / g.hop, Tp = (T + 31) / 32 * 32;
    StftBranch br[kMaxBranches];
    for (int k = 0; k < g.nbr; ++k) {
        br[k].wlen = g.wins[k];
        br[k].x0 = x0[k];
        if (k == g.mask_br) { br[k].mag = mag; br[k].cosv = cosv; br[k].sinv = sinv; }
    }
    return lass_launch_stft2(wav, cf, g.nfft, g.hop, T, Tp, g.nbr, br, g.magphase_sem, c->bn0_s, c->bn0_h, c->tw2k, st);
}

// lass_front_end, lass_front_end_ragged and lass_front_end_windows behind their argument checks: x0 is (nbr, B, Tp, fcrop)
static int front_end(lass_ctx* c, const float* wav, const ClipForm& cf, float* mag, float* cos_out, float* sin_out, float* x0,
                     void* stream) {
    const int T = 1 + cf.L / c->g.hop, Tp = (T + 31) / 32 * 32;
    float* x0k[kMaxBranches];
    for (int k = 0; k < c->g.nbr; ++k) x0k[k] = x0 + (size_t)k * cf.B * Tp * c->g.fcrop;
    HIP_TRY(c, launch_front_end(c, wav, cf, x0k, mag, cos_out, sin_out, (hipStream_t)stream));
    return 0;
}

int lass_front_end(lass_ctx* c, const float* wav, int B, int L, float* mag, float* cos_out, float* sin_out, float* x0,
                   void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!wav || !x0 || B <= 0 || L <= c->g.nfft / 2) return fail(c, LASS_ERR_ARG, "lass_front_end: bad argument");
    return front_end(c, wav, ClipForm{B, L}, mag, cos_out, sin_out, x0, stream);
}

int lass_front_end_ragged(lass_ctx* c, const float* wav, const int* lengths, int B, int L, float* mag, float* cos_out,
                          float* sin_out, float* x0, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!wav || !lengths || !x0 || B <= 0 || L <= c->g.nfft / 2) return fail(c, LASS_ERR_ARG, "lass_front_end_ragged: bad argument");
    return front_end(c, wav, ClipForm{B, L, lengths}, mag, cos_out, sin_out, x0, stream);
}

int lass_istft_ragged(lass_ctx* c, const float* real, const float* imag, const int* lengths, int B, int T, int L, int n_fft,
                      int win_length, float* wav, void* stream) {
    if (!c || !real || !imag || !lengths || !wav || B <= 0 || !istft_nfft_ok(c, n_fft) || L <= n_fft / 2 ||
        T != 1 + L / c->g.hop || win_length < 32 || win_length > n_fft || (2048 % win_length) != 0)
        return fail(c, LASS_ERR_ARG, "lass_istft_ragged: bad argument (T = 1 + L/" + std::to_string(c ? c->g.hop : LASS_HOP) +
                                         " frames per clip, L > n_fft/2)");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_istft2(real, imag, ClipForm{B, L, lengths}, T, n_fft, win_length, c->g.hop, c->tw2k, wav,
                                  (hipStream_t)stream));
    return 0;
}

int lass_front_end_windows(lass_ctx* c, const float* recording, int64_t total, const int64_t* starts, int B, int W, float* mag,
                           float* cos_out, float* sin_out, float* x0, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!recording || !starts || !x0 || B <= 0 || W <= c->g.nfft / 2 || total < W)
        return fail(c, LASS_ERR_ARG, "lass_front_end_windows: bad argument (n_fft/2 < W <= total)");
    return front_end(c, recording, ClipForm{B, W, nullptr, starts, nullptr, total}, mag, cos_out, sin_out, x0, stream);
}

int lass_istft_windows(lass_ctx* c, const float* real, const float* imag, const int64_t* starts, const int* keep, int64_t total,
                       int B, int T, int W, int n_fft, int win_length, float* out, void* stream) {
    if (!c || !real || !imag || !starts || !keep || !out || B <= 0 || !istft_nfft_ok(c, n_fft) || W <= n_fft / 2 ||
        total < W || T != 1 + W / c->g.hop || win_length < 32 || win_length > n_fft || (2048 % win_length) != 0)
        return fail(c, LASS_ERR_ARG, "lass_istft_windows: bad argument (T = 1 + W/" + std::to_string(c ? c->g.hop : LASS_HOP) +
                                         " frames per window, n_fft/2 < W <= total)");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_istft2(real, imag, ClipForm{B, W, nullptr, starts, keep, total}, T, n_fft, win_length, c->g.hop,
                                  c->tw2k, out, (hipStream_t)stream));
    return 0;
}

int lass_istft_windows_faded(lass_ctx* c, const float* real, const float* imag, const int64_t* starts, const int* keep,
                             const int* fade, const float* ramp, int F, int64_t total, int B, int T, int W, int n_fft,
                             int win_length, float* out, void* stream) {
    if (!c || !real || !imag || !starts || !keep || !fade || !ramp || !out || B <= 0 || !istft_nfft_ok(c, n_fft) || W <= n_fft / 2 ||
        total < W || T != 1 + W / c->g.hop || win_length < 32 || win_length > n_fft || (2048 % win_length) != 0 || F < 1 || F > W)
        return fail(c, LASS_ERR_ARG, "lass_istft_windows_faded: bad argument (T = 1 + W/" + std::to_string(c ? c->g.hop : LASS_HOP) +
                                         " frames per window, n_fft/2 < W <= total, 1 <= F <= W)");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_istft2(real, imag, ClipForm{B, W, nullptr, starts, keep, total, fade, ramp, F}, T, n_fft, win_length,
                                  c->g.hop, c->tw2k, out, (hipStream_t)stream));
    return 0;
}

int lass_workspace_tensor(const lass_ctx* c, int B, int L, const char* name_c, size_t* offset, int64_t shape[4],
                          int64_t strides[4]) {
    if (!c || !name_c || !offset || !shape || !strides) return LASS_ERR_ARG;
    // a batch whose LAST separation ran as half-batches (B >= 8, LASS_SPLIT: the replayed graph by default) holds their layouts
    // in its workspace, not this one; after an eager, unsplit call - or before any call - the whole-batch layout is what is there
    if (auto it = c->last_split.find({B, L}); it != c->last_split.end() && it->second) return LASS_ERR_STATE;
    const Plan pl = make_plan(c, B, L);
    if (!pl.valid) return LASS_ERR_ARG;
    const std::string name(name_c);
    for (const PlanTensor& t : plan_tensors(plan_inputs(c), pl))
        if (t.name == name) {
            *offset = t.offset;
            std::copy(t.shape, t.shape + 4, shape);
            std::copy(t.strides, t.strides + 4, strides);
            return 0;
        }
    return LASS_ERR_ARG;
}

int lass_upconv(lass_ctx* c, const char* name, const float* x, int B, int h, int w, const float* shift, float* y,
                void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!name || !x || !shift || !y) return fail(c, LASS_ERR_ARG, "lass_upconv: bad argument");
    for (int i = 0; i < 6; ++i)
        if (std::string("base.") + c->m.D[i].name == name)
            return run_upconv(c, i, x, B, h, w, shift, y, (long)c->m.D[i].cout * h * c->m.D[i].uh * w * c->m.D[i].uw,
                              (hipStream_t)stream);
    return fail(c, LASS_ERR_ARG, std::string("lass_upconv: unknown decoder '") + name + "'");
}

int lass_mask_apply(lass_ctx* c, const float* x12, const float* mag, const float* cos_in, const float* sin_in, int B,
                    int T, int Tpad, float* out_real, float* out_imag, void* stream) {
    int r = check_ready(c);
    if (r) return r;
    if (!x12 || !mag || !cos_in || !sin_in || !out_real || !out_imag)
        return fail(c, LASS_ERR_ARG, "lass_mask_apply: bad argument");
    HIP_TRY(c, lass_launch_mask(x12, rawp(c, "base.after_conv.weight"), rawp(c, "base.after_conv.bias"), mag, cos_in,
                                sin_in, B, T, Tpad, c->g.fcrop, out_real, out_imag, (hipStream_t)stream));
    return 0;
}

int lass_sdr_stats(lass_ctx* c, const float* ref, const float* est, int B, int L, double* stats, void* stream) {
    if (!c || !ref || !est || !stats || B <= 0 || L <= 0) return fail(c, LASS_ERR_ARG, "lass_sdr_stats: bad argument");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_sdr(ref, est, B, L, stats, (hipStream_t)stream));
    return 0;
}

int lass_mix_at_snr(lass_ctx* c, float* source, const float* noise, const float* snr_db, float* mixture, int B, int L,
                    double* scratch, void* stream) {
    if (!c || !source || !noise || !snr_db || !mixture || !scratch || B <= 0 || L <= 0)
        return fail(c, LASS_ERR_ARG, "lass_mix_at_snr: bad argument");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_mix_at_snr(source, noise, snr_db, mixture, B, L, scratch, (hipStream_t)stream));
    return 0;
}

// ---- the audio file entry points ------------------------------------------------------------------------------------------------
// Each builds audio_args.h's operand structs from its positional arguments, runs its ordered list of checks there (plus, where it
// has one, the refusal that reads device-side constants, last as ever), selects the device and launches.
static int refuse(lass_ctx* c, const std::string& message) { return message.empty() ? 0 : fail(c, LASS_ERR_ARG, message); }

// The two decode entries (planar: one output plane per channel, no down-mix).
static int decode_resample(lass_ctx* c, const char* w, const PayloadRows& raw, int B, const RationalFilter& F, bool planar, float* out,
                           int L_out, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (int r = refuse(c, check_decode(w, raw, B, F, out, L_out))) return r;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_decode_resample(raw, B, F, planar, out, L_out, (hipStream_t)stream));
    return 0;
}

int lass_decode_resample(lass_ctx* c, const void* raw, int64_t row_stride_bytes, int B, int frames, int channels, int encoding,
                         int up, int down, const float* taps, int n_taps, float* out, int L_out, void* stream) {
    return decode_resample(c, "lass_decode_resample: ", {raw, row_stride_bytes, encoding, frames, channels}, B, {up, down, taps, n_taps},
                           false, out, L_out, stream);
}

int lass_decode_resample_planar(lass_ctx* c, const void* raw, int64_t row_stride_bytes, int B, int frames, int channels,
                                int encoding, int up, int down, const float* taps, int n_taps, float* out, int L_out, void* stream) {
    return decode_resample(c, "lass_decode_resample_planar: ", {raw, row_stride_bytes, encoding, frames, channels}, B,
                           {up, down, taps, n_taps}, true, out, L_out, stream);
}

// The three encode entries (dry NULL: no remix; gain_required: lass_resample_encode_gain).
static int encode(lass_ctx* c, const char* w, const PlaneRows& P, const RationalFilter& F, const DrySource* dry, const float* gain,
                  bool gain_required, const PayloadRows& out, unsigned* clipped, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (int r = refuse(c, check_encode(w, P, F, dry, gain, gain_required, out, clipped))) return r;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_encode(P, F, dry, gain, out, clipped, (hipStream_t)stream));
    return 0;
}

int lass_resample_encode(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                         int up, int down, const float* taps, int n_taps, int encoding, void* out_bytes,
                         int64_t out_row_stride_bytes, int frames_out, unsigned* clipped, void* stream) {
    return encode(c, "lass_resample_encode: ", {planes, row_stride, plane_stride, B, channels, L_in}, {up, down, taps, n_taps}, nullptr,
                  nullptr, false, {out_bytes, out_row_stride_bytes, encoding, frames_out, channels}, clipped, stream);
}

int lass_resample_encode_gain(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels,
                              int L_in, int up, int down, const float* taps, int n_taps, int encoding, const float* gain,
                              void* out_bytes, int64_t out_row_stride_bytes, int frames_out, unsigned* clipped, void* stream) {
    return encode(c, "lass_resample_encode_gain: ", {planes, row_stride, plane_stride, B, channels, L_in}, {up, down, taps, n_taps},
                  nullptr, gain, true, {out_bytes, out_row_stride_bytes, encoding, frames_out, channels}, clipped, stream);
}

int lass_remix_encode(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in, int up,
                      int down, const float* taps, int n_taps, const void* dry, int64_t dry_row_stride_bytes, int dry_encoding,
                      const float* amount, int encoding, const float* gain, void* out_bytes, int64_t out_row_stride_bytes,
                      int frames_out, unsigned* clipped, void* stream) {
    const DrySource d{{dry, dry_row_stride_bytes, dry_encoding, frames_out, channels}, amount};
    return encode(c, "lass_remix_encode: ", {planes, row_stride, plane_stride, B, channels, L_in}, {up, down, taps, n_taps}, &d, gain,
                  false, {out_bytes, out_row_stride_bytes, encoding, frames_out, channels}, clipped, stream);
}

// The two sample-peak entries (dry NULL: no remix).
static int sample_peak(lass_ctx* c, const char* w, const PlaneRows& P, const RationalFilter& F, const DrySource* dry, int frames_out,
                       float* peak, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (int r = refuse(c, check_peak(w, P, F, dry, frames_out, nullptr, peak))) return r;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_sample_peak(P, F, dry, frames_out, peak, (hipStream_t)stream));
    return 0;
}

int lass_resample_peak(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                       int up, int down, const float* taps, int n_taps, int frames_out, float* peak, void* stream) {
    return sample_peak(c, "lass_resample_peak: ", {planes, row_stride, plane_stride, B, channels, L_in}, {up, down, taps, n_taps}, nullptr,
                       frames_out, peak, stream);
}

int lass_remix_peak(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in, int up,
                    int down, const float* taps, int n_taps, const void* dry, int64_t dry_row_stride_bytes, int dry_encoding,
                    const float* amount, int frames_out, float* peak, void* stream) {
    const DrySource d{{dry, dry_row_stride_bytes, dry_encoding, frames_out, channels}, amount};
    return sample_peak(c, "lass_remix_peak: ", {planes, row_stride, plane_stride, B, channels, L_in}, {up, down, taps, n_taps}, &d,
                       frames_out, peak, stream);
}

int lass_resample_true_peak(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                            int up, int down, const float* taps, int n_taps, int frames_out, int os, const float* os_taps,
                            int n_os_taps, float* peak, void* stream) {
    const std::string w = "lass_resample_true_peak: ";
    if (!c) return LASS_ERR_ARG;
    const PlaneRows P{planes, row_stride, plane_stride, B, channels, L_in};
    const RationalFilter F{up, down, taps, n_taps};
    const Oversampler O{os, os_taps, n_os_taps};
    if (int r = refuse(c, check_peak(w, P, F, nullptr, frames_out, &O, peak))) return r;
    if (!lass_resample_true_peak_fits(up, down, (up == 1 && down == 1) ? 1 : n_taps, os))
        return fail(c, LASS_ERR_ARG, w + "at up = " + std::to_string(up) + ", down = " + std::to_string(down) +
                    " the 21 frames one interpolated value reaches do not fit the CU's LDS beside the filter table (take the "
                    "true peak on the host)");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_resample_true_peak(P, F, frames_out, O, peak, (hipStream_t)stream));
    return 0;
}

// The two meter entries up to the launch: the checks, then the filter formed (stats: lass_loudness_stats).
static int meter_ready(lass_ctx* c, const std::string& w, const PlaneRows& P, const int* lengths, int hop, const double* coef,
                       const float* weights, const double* out, const double* blocks, int nb_max, const double* short_term, int ns_max,
                       const void* scratch, size_t scratch_bytes, bool stats, LoudnessFilter* f) {
    if (!c) return LASS_ERR_ARG;
    if (int r = refuse(c, check_meter(w, P, lengths, hop, coef, weights, out, blocks, nb_max, short_term, ns_max, scratch, scratch_bytes,
                                      stats)))
        return r;
    if (!lass_loudness_filter(coef, hop, f))
        return fail(c, LASS_ERR_ARG, w + "coef must be finite, both biquads with their poles inside the unit circle");
    return use_device(c);
}

int lass_loudness_stats(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L,
                        const int* lengths, int hop, const double* coef, const float* weights, double* out, double* blocks,
                        int nb_max, double* short_term, int ns_max, void* scratch, size_t scratch_bytes, void* stream) {
    const PlaneRows P{planes, row_stride, plane_stride, B, channels, L};
    LoudnessFilter f;
    if (int r = meter_ready(c, "lass_loudness_stats: ", P, lengths, hop, coef, weights, out, blocks, nb_max, short_term, ns_max, scratch,
                            scratch_bytes, true, &f))
        return r;
    HIP_TRY(c, lass_launch_loudness_stats(P, lengths, hop, f, weights, out, blocks, nb_max, short_term, ns_max,
                                          static_cast<double*>(scratch), (hipStream_t)stream));
    return 0;
}

int lass_loudness(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L,
                  const int* lengths, int hop, const double* coef, const float* weights, double* out, double* blocks, int nb_max,
                  void* scratch, size_t scratch_bytes, void* stream) {
    const PlaneRows P{planes, row_stride, plane_stride, B, channels, L};
    LoudnessFilter f;
    if (int r = meter_ready(c, "lass_loudness: ", P, lengths, hop, coef, weights, out, blocks, nb_max, nullptr, 0, scratch, scratch_bytes,
                            false, &f))
        return r;
    HIP_TRY(c, lass_launch_loudness(P, lengths, hop, f, weights, out, blocks, nb_max, static_cast<double*>(scratch), (hipStream_t)stream));
    return 0;
}

int lass_loudness_gain(lass_ctx* c, const double* loudness, const float* peak, int B, double target_lufs, float ceiling, float* gain,
                       int* limited, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (int r = refuse(c, check_gain_rule("lass_loudness_gain: ", loudness, peak, B, target_lufs, ceiling, gain, limited))) return r;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_loudness_gain(loudness, peak, B, target_lufs, ceiling, gain, limited, (hipStream_t)stream));
    return 0;
}

int lass_limit(lass_ctx* c, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L, int os,
               const float* os_taps, int n_os_taps, const float* gain, float ceiling, int H, const float* window, float* out,
               int64_t out_row_stride, int64_t out_plane_stride, float* curve, float* envelope, int64_t curve_row_stride,
               float* min_gain, int* frames, void* stream) {
    if (!c) return LASS_ERR_ARG;
    const PlaneRows P{planes, row_stride, plane_stride, B, channels, L}, O{out, out_row_stride, out_plane_stride, B, channels, L};
    if (int r = refuse(c, check_limit("lass_limit: ", P, {os, os_taps, n_os_taps}, gain, ceiling, H, window, O, curve, envelope,
                                      curve_row_stride, min_gain, frames)))
        return r;
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_limit(P, {os, os > 1 ? os_taps : nullptr, os > 1 ? n_os_taps : 0}, gain, ceiling, H, window, O, curve, envelope,
                                 curve_row_stride, min_gain, frames, (hipStream_t)stream));
    return 0;
}

int lass_segment_mix(lass_ctx* c, const float* waveforms, int B, int L, const int* mix_num, const float* comp_db, int max_comp,
                     const float* noise_db, float* mixture, float* segment, double* scratch, void* stream) {
    if (!c || !waveforms || !mix_num || !comp_db || !noise_db || !mixture || !segment || !scratch || B <= 0 || L <= 0)
        return fail(c, LASS_ERR_ARG, "lass_segment_mix: bad argument");
    if (max_comp < 1 || max_comp > 7) return fail(c, LASS_ERR_ARG, "lass_segment_mix: max_comp (max_mix_num - 1) must be 1 ... 7");
    if (mixture == waveforms || segment == waveforms || mixture == segment)
        return fail(c, LASS_ERR_ARG, "lass_segment_mix: waveforms, mixture and segment must be three different buffers");
    if (int r = use_device(c)) return r;
    HIP_TRY(c, lass_launch_segment_mix(waveforms, B, L, mix_num, comp_db, max_comp, noise_db, mixture, segment, scratch,
                                       (hipStream_t)stream));
    return 0;
}

// Precomputed analysis of the mixtures (the reference's multi-STFT wrapper reads these from input_dict,
// resunet_with_multistft.py:233-241): magnitude per branch, cos / sin of the mask branch, each (B, T, nbins).
struct Components {
    const float* mag[kMaxBranches];
    const float* cosv;
    const float* sinv;
};

// cf: the clips of the call (kernels.h) - B rows of L samples, dense or with a length per clip, or B windows of L samples of ONE
// row of cf.total samples (`mixture`), their kept parts stored into one row of as many samples (`out`).  The two ends of the
// network run in cf's form; everything between them sees B images of (Tp, fcrop) whatever the form.  pl: the plan of (cf.B, cf.L) -
// the caller made it, once per call (an invalid one is refused here, behind the checks that come first).
static int separate_impl(lass_ctx* c, const float* mixture, const Components* comp, const float* condition, float* out,
                         const ClipForm& cf, const Plan& pl, void* workspace, size_t workspace_bytes, void* stream, const char* who) {
    const int B = cf.B;
    int r = check_ready(c);
    if (r) return r;
    const Geometry& g = c->g;
    if ((!mixture && !comp) || !condition || !out || !workspace) return fail(c, LASS_ERR_ARG, std::string(who) + ": null pointer");
    if (!pl.valid)
        return fail(c, LASS_ERR_ARG, std::string(who) + ": need B >= 1 and " + std::to_string(g.nfft / 2) +
                                         " < L, with decoder_block6's concat (" + std::to_string(c->m.dec_cat[5]) +
                                         " ch x frames x " + std::to_string(g.fcrop) +
                                         " bins, f32) below 4 GiB per clip (longer clips: ResUNet30.chunk_inference)");
    if (workspace_bytes < pl.total)
        return fail(c, LASS_ERR_WORKSPACE, "workspace too small: need " + std::to_string(pl.total) + " bytes");
    if (((uintptr_t)workspace & 255) != 0) return fail(c, LASS_ERR_ARG, "workspace must be 256-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    const int T = pl.T, Tp = pl.Tp, nbr = g.nbr;
    float* shift = F(pl.shift);
    // What each block is called with - its BlockIO, its bf16 form, each transposed conv's family - is decided once, in
    // conv_route.h's plan_separate; the fusions below follow it, and run_resblock / run_upconv refuse a contradiction
    const SeparatePlan& sp = pl.sp;
    const auto scratch = [&](BlockFusions& f) {  // the plan's split-K and V slots, for every block
        if (sp.kpart_floats) f.kpart = F(pl.kpart);
        if (sp.v_floats) { f.vws = F(pl.vprep); f.vws_floats = sp.v_floats; }
        if (sp.m_floats) { f.mws = F(pl.mgemm); f.mws_floats = sp.m_floats; }
    };
    // ---- front end: STFT + magnitude / phase + bn0 / T-pad / F-crop (base.py:83-113, resunet.py:533-552) ------------
    const float *mag_m = F(pl.mag), *cos_m = F(pl.cosv), *sin_m = F(pl.sinv);  // of the mask branch
    if (mixture) {
        ProfScope ps(c, st, P_STFT);
        float* x0k[kMaxBranches];
        for (int k = 0; k < nbr; ++k) x0k[k] = F(pl.x0[k]);
        if (cf.planes) {
            // linked channels: the network reads the guide's magnitude through x0 alone, and the head meets the unit spectrum
            // (mag = cos = 1, sin = 0, filled on every call, replays included) - out_real / out_imag are then the mask itself
            HIP_TRY(c, launch_front_end(c, mixture, cf, x0k, nullptr, nullptr, nullptr, st));
            HIP_TRY(c, lass_launch_unit_spectrum(F(pl.mag), F(pl.cosv), F(pl.sinv), (size_t)B * T * g.nbins, st));
        } else {
            HIP_TRY(c, launch_front_end(c, mixture, cf, x0k, F(pl.mag), F(pl.cosv), F(pl.sinv), st));
        }
    } else {
        ProfScope ps(c, st, P_STFT);
        for (int k = 0; k < nbr; ++k) {
            if (!comp->mag[k]) return fail(c, LASS_ERR_ARG, std::string(who) + ": null magnitude");
            HIP_TRY(c, lass_launch_x0_from_mag(comp->mag[k], B, T, Tp, g.fcrop, c->bn0_s, c->bn0_h, F(pl.x0[k]), st));
        }
        if (!comp->cosv || !comp->sinv) return fail(c, LASS_ERR_ARG, std::string(who) + ": null phase");
        mag_m = comp->mag[g.mask_br]; cos_m = comp->cosv; sin_m = comp->sinv;
    }
    {
        ProfScope ps(c, st, P_FILM);
        HIP_TRY(c, lass_launch_film(condition, B, c->film_W, c->film_b, c->bn_base, c->n_shift, shift, st));
    }
    // conv_route.h's head_sc_fold: one decision for encoder_block1.conv2, decoder_block6's transposed conv and the head
    HeadScPlanes hs_skip, hs_up, hs_head;
    if (sp.head_sc_fold) {
        hs_skip.skip = hs_head.skip = F(pl.lg_skip); hs_skip.w = c->img.f32(HS_WSKIP);
        hs_up.up = hs_head.up = F(pl.lg_up); hs_up.w = c->img.f32(HS_WT);
        hs_skip.up = hs_head.up;  // (for run_resblock's overlap checks; the encoder launch does not touch it)
    }
    // Routes.  pre_conv (resunet.py:555) is never materialised: encoder_block1 forms it from x0 while staging.  Tp is a
    // multiple of 32, so every pooled level has even rows and F.avg_pool2d (resunet.py:197) rides in conv2's epilogue.
    // decoder_block6 runs at W = fcrop with 32 channels: after_conv + mask ride in its conv2's epilogue.
    // bf16 mode: which tensors travel as blocked bf16 copies, and which blocks run fused, is sp.
    // Where decoders 2-6 take their concat that way the copies live in the concat's storage
    const auto copies = [&](float* store, const ResBlock& rb, int e) {  // the two copies of rb's input (level e) in `store`
        const Site& s = c->sites[rb.s1];
        return CatCopies{store, (char*)store + (size_t)B * rb.cin * pl.lv.eh[e] * pl.lv.ew[e] * 2, rb.cin / 8, c->bn_scale + s.off, shift + s.off};
    };
    CatCopies cb[6], pc[4];
    for (int d = 1; d < 6; ++d) cb[d] = copies(F(pl.cat[d]), c->dec[d], 5 - d);
    // ... and encoder blocks 2-5 their (pooled) input, from the previous block's fused pool, in the pooled tensor's
    for (int i = 0; i < 4; ++i) pc[i] = copies(F(pl.pool[i]), c->enc[nbr + i], i + 1);
    // ---- encoder (resunet.py:556-562; resunet_with_multistft.py:151-179) -----------------------------------------------
    const float* x = nullptr;
    for (int i = 0; i < 7; ++i) {
        const int H = pl.lv.eh[i], W = pl.lv.ew[i];
        const long HW = (long)H * W;
        const EncSpec& e = c->m.E[i];
        const int nb = i == 0 ? nbr : 1;  // encoder_block1 runs once per analysis branch
        float* o = nullptr;
        long o_bs = 0;
        for (int k = 0; k < nb; ++k) {
            const ResBlock& rb = c->enc[i == 0 ? k : nbr - 1 + i];
            const BlockIO& io = sp.enc_io[i];
            BlockFusions f;
            f.cofs = k * e.cout;  // channel offset of this branch inside the concatenated skip / pool
            if (i < 6) {  // skip output lives behind the transposed-conv half of decoder (5-i)'s concat buffer
                const int d = 5 - i;
                o = F(pl.cat[d]) + (size_t)(c->m.D[d].cout + f.cofs) * HW;
                o_bs = (long)c->m.dec_cat[d] * HW;
            } else {
                o = F(pl.center);
                o_bs = rb.cout * HW;
            }
            if (io.pool) {
                const long Ho = H / e.dh, Wo = W / e.dw;
                f.pool_out = F(pl.pool[i]) + (size_t)f.cofs * Ho * Wo;
                f.pool_h = e.dh;
                f.pool_bs = (long)e.cout * nb * Ho * Wo;
            }
            PreConv pre{};
            if (io.x0) {
                pre = PreConv{F(pl.x0[k]), rawp(c, c->pre_name[k] + ".weight"), rawp(c, c->pre_name[k] + ".bias")};
                f.pre = &pre;
            }
            if (io.sc_planes) f.planes = &hs_skip;
            if (io.skip_out) f.skip_out = &cb[5 - i];
            if (io.cat_in) f.cat_in = &pc[i - 1];
            if (io.pool_copies) f.pool_copies = &pc[i];
            scratch(f);
            r = run_resblock(c, rb, x, rb.cin * HW, B, H, W, shift, F(pl.a2), o, o_bs, st, f);
            if (r) return r;
        }
        x = i < 6 ? F(pl.pool[i]) : o;  // conv_block7a: downsample (1,1) is the identity (resunet.py:363-370)
    }
    // ---- decoder (resunet.py:563-568) -------------------------------------------------------------------------
    for (int d = 0; d < 6; ++d) {
        const int e = 5 - d;
        const int H = pl.lv.eh[e], W = pl.lv.ew[e];
        const long HW = (long)H * W;
        const int h = H / c->m.D[d].uh, w = W / c->m.D[d].uw;
        const ResBlock& rb = c->dec[d];
        const BlockIO& io = sp.dec_io[d];
        BlockFusions f;
        // decoder_block6 in the blocked bf16 pipeline: the transposed conv runs inside the block's fused kernel, its output
        // (half of the concat, at the full resolution) is never written
        const UpFuse upf{x, c->m.D[d].cin, h, w, c->up_img[d].p[UP16], c->img.p[UP_SC16]};
        if (io.up_cin) {
            f.up = &upf;
        } else {
            r = run_upconv(c, d, x, B, h, w, shift, F(pl.cat[d]), rb.cin * HW, st, sp.up[d].out_copies ? &cb[d] : nullptr, sp.up[d].in_act,
                           sp.up[d].family == UP_LOGITS ? &hs_up : nullptr);
            if (r) return r;
        }
        // a decoder output that feeds only the next transposed conv is handed over activated, as blocked bf16
        if (io.act_out) f.act_out = &c->sites[c->dec_site[d + 1]];
        if (io.cat_in) f.cat_in = &cb[d];
        const MaskHead head{mag_m, cos_m, sin_m, F(pl.oreal), F(pl.oimag), T, g.nbins};
        if (io.head) f.head = &head;
        if (io.sc_planes) f.planes = &hs_head;
        scratch(f);
        r = run_resblock(c, rb, F(pl.cat[d]), rb.cin * HW, B, H, W, shift, F(pl.a2), F(pl.decout[d]), rb.cout * HW, st, f);
        if (r) return r;
        x = F(pl.decout[d]);
    }
    if (cf.planes) {
        // The head has read the unit spectrum: its three planes now serve as the Y scratch of one channel at a time (two of them),
        // Y = STFT(plane) * M, which the iSTFT of the call's own form turns into that channel's output.  One launch pair per
        // channel, in stream order: the scratch holds one channel's spectrum.
        for (int ch = 0; ch < cf.channels; ++ch) {
            {
                ProfScope ps(c, st, P_STFT);
                HIP_TRY(c, lass_launch_masked_stft(cf.planes + (size_t)ch * cf.plane_stride, cf, g.nfft, g.hop, T, g.wins[g.mask_br],
                                                   F(pl.oreal), F(pl.oimag), F(pl.mag), F(pl.cosv), c->tw2k, st));
            }
            ProfScope ps(c, st, P_ISTFT);
            HIP_TRY(c, lass_launch_istft2(F(pl.mag), F(pl.cosv), cf, T, g.nfft, g.wins[g.mask_br], g.hop, c->tw2k,
                                          out + (size_t)ch * cf.out_plane_stride, st));
        }
        return 0;
    }
    {
        ProfScope ps(c, st, P_ISTFT);
        HIP_TRY(c, lass_launch_istft2(F(pl.oreal), F(pl.oimag), cf, T, g.nfft, g.wins[g.mask_br], g.hop, c->tw2k, out, st));
    }
    return 0;
}

// Clips [h, B) of cf as a call of their own.  *row: how far into the mixture and the output their rows begin - the window form's
// second half reads its own entries of the index arrays and the SAME two long rows.
static ClipForm upper_clips(const ClipForm& cf, int h, size_t* row) {
    ClipForm u = cf;
    u.B = cf.B - h;
    if (cf.lengths) u.lengths = cf.lengths + h;
    if (cf.starts) u.starts = cf.starts + h;
    if (cf.keep) u.keep = cf.keep + 2 * h;
    if (cf.fade) u.fade = cf.fade + 2 * h;
    *row = cf.starts ? 0 : (size_t)h * cf.L;
    if (cf.planes) u.planes = cf.planes + *row;  // (the linked planes are laid out as the guide)
    return u;
}

// lass_separate's launches, whole or as two overlapping half-batches, as cp (plan_call) says.  Capture-safe: under stream capture
// the event pair makes `s2` a parallel branch of the same graph.  The one place that records, for lass_workspace_tensor, which
// layout the workspace is left in.
static int separate_any(lass_ctx* c, const float* mixture, const float* condition, float* out, const ClipForm& cf, const CallPlan& cp,
                        void* workspace, size_t workspace_bytes, hipStream_t stream, const char* who) {
    // (a call that separate_impl is going to refuse - not finalized, a null pointer - reaches it whole, for its error text)
    const bool split = cp.split && c->finalized && mixture && condition && out && workspace;
    c->last_split[{cf.B, cf.L}] = split;
    if (!split) return separate_impl(c, mixture, nullptr, condition, out, cf, cp.whole, workspace, workspace_bytes, stream, who);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->ev_fork) HIP_TRY(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    if (!c->s2) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->s2, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    }
    const int h = cf.B / 2;
    const size_t half_ws = cp.half_bytes();
    HIP_TRY(c, hipEventRecord(c->ev_fork, stream));
    HIP_TRY(c, hipStreamWaitEvent(c->s2, c->ev_fork, 0));
    ClipForm lower = cf;
    lower.B = h;
    size_t row2;
    const ClipForm upper = upper_clips(cf, h, &row2);  // (split_halves: B is even)
    int r = separate_impl(c, mixture, nullptr, condition, out, lower, cp.half, workspace, half_ws, stream, who);
    const int r2 = separate_impl(c, mixture + row2, nullptr, condition + (size_t)h * LASS_COND, out + row2, upper, cp.half,
                                 (char*)workspace + half_ws, half_ws, c->s2, who);
    if (!r) r = r2;
    // the join is recorded even after a failure: a capturing stream must get its branch back
    HIP_TRY(c, hipEventRecord(c->ev_join, c->s2));
    HIP_TRY(c, hipStreamWaitEvent(stream, c->ev_join, 0));
    return r;
}

// lass_separate, lass_separate_ragged and lass_separate_windows (cf says which): one call, eager or through the graph cache
static int separate_call(lass_ctx* c, const float* mixture, const float* condition, float* out, const ClipForm& cf, void* workspace,
                         size_t workspace_bytes, void* stream, const char* who) {
    const int B = cf.B, L = cf.L;
    if (!mixture) return fail(c, LASS_ERR_ARG, std::string(who) + ": null pointer");
    // Graph replay: the third call that presents the same (pointers, shape) key is captured once (on an internal stream; the
    // caller's may be the legacy default stream, which cannot be captured) and replayed from then on.  Callers that hand
    // over fresh buffers every time simply stay on the eager path; so does a profiled context.
    if (c->use_graph && !c->profiling && c->finalized) {
        GraphKey key;
        key.mix = mixture; key.cond = condition; key.out = out; key.ws = workspace; key.lens = cf.lengths; key.B = B; key.L = L;
        key.gen = c->gen;
        key.starts = cf.starts; key.keep = cf.keep; key.total = cf.total;
        key.fade = cf.fade; key.ramp = cf.ramp; key.F = cf.F;
        key.planes = cf.planes; key.plane_stride = cf.plane_stride; key.out_plane_stride = cf.out_plane_stride; key.channels = cf.channels;
        auto& slot = c->graphs.touch(key);
        if (c->graphs.drain_due()) {  // a caller cycling through many recurring keys: bound the list of evicted execs here
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipDeviceSynchronize());
            for (hipGraphExec_t x : c->graphs.take_retired()) (void)hipGraphExecDestroy(x);
        }
        if (slot.exec()) {  // (no planning on a replay: the slot holds what the captured plan said)
            if (workspace_bytes < slot.need)
                return fail(c, LASS_ERR_WORKSPACE, "workspace too small: need " + std::to_string(slot.need) + " bytes");
            HIP_TRY(c, hipSetDevice(c->device));
            HIP_TRY(c, hipGraphLaunch(slot.exec(), (hipStream_t)stream));
            ++c->g_replays;
            c->last_split[{B, L}] = slot.split;
            return 0;
        }
        if (c->graphs.capture_due(slot)) {
            // argument errors are reported as such, before any capture starts, by the eager run below: only a failure of the
            // capture machinery itself (begin / end / instantiate, or a launch refused under capture) turns graph replay off
            int r0 = check_ready(c);
            if (r0) return r0;
            const CallPlan cp = plan_call(c, B, L, true, workspace_bytes);
            if (condition && out && workspace && cp.whole.valid && workspace_bytes >= cp.whole.total && ((uintptr_t)workspace & 255) == 0) {
                slot.need = cp.need;
                slot.split = cp.split;
                HIP_TRY(c, hipSetDevice(c->device));
                if (!c->g_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->g_stream, hipStreamNonBlocking));
                hipGraphExec_t exec = nullptr;
                if (hipStreamBeginCapture(c->g_stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
                    const int r = separate_any(c, mixture, condition, out, cf, cp, workspace, workspace_bytes, c->g_stream, who);
                    hipGraph_t graph = nullptr;
                    const hipError_t e = hipStreamEndCapture(c->g_stream, &graph);  // always ends the capture, also after a failure
                    if (!(r == 0 && e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess))
                        exec = nullptr;
                    if (graph) (void)hipGraphDestroy(graph);
                }
                if (exec) {
                    c->graphs.set_exec(slot, exec);
                    ++c->g_captures;
                    HIP_TRY(c, hipGraphLaunch(exec, (hipStream_t)stream));
                    return 0;
                }
                // A launch failed inside the capture, or the runtime refused it: nothing has run yet.  Stay eager from now on and
                // run this call eagerly below (an error is reported only if the eager run fails too).
                (void)hipGetLastError();
                c->use_graph = false;
                c->err.clear();
            }
        }
    }
    const CallPlan cp = plan_call(c, B, L, false, workspace_bytes);
    return separate_any(c, mixture, condition, out, cf, cp, workspace, workspace_bytes, (hipStream_t)stream, who);
}

int lass_separate(lass_ctx* c, const float* mixture, const float* condition, float* out, int B, int L, void* workspace,
                  size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    return separate_call(c, mixture, condition, out, ClipForm{B, L}, workspace, workspace_bytes, stream, "lass_separate");
}

int lass_ragged_bucket(const lass_ctx* c, int L, int* lo, int* hi) {
    if (!c || L <= c->g.nfft / 2) return LASS_ERR_ARG;
    const int T = 1 + L / c->g.hop, Tp = (T + 31) / 32 * 32;
    if (lo) *lo = std::max(c->g.hop * (Tp - 32), c->g.nfft / 2 + 1);
    if (hi) *hi = L;  // a row holds L samples
    return 0;
}

int lass_separate_ragged(lass_ctx* c, const float* mixture, const int* lengths, const float* condition, float* out, int B, int L,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (!lengths) return fail(c, LASS_ERR_ARG, "lass_separate_ragged: null lengths");
    return separate_call(c, mixture, condition, out, ClipForm{B, L, lengths}, workspace, workspace_bytes, stream, "lass_separate_ragged");
}

// lass_separate_windows and lass_separate_windows_faded behind the checks that only the latter has (fade == nullptr: the former)
// link: the planes of a linked call (ClipForm's four fields; none: an unlinked call), checked by the caller
static int separate_windows(lass_ctx* c, const std::string& who, const float* recording, int64_t total, const int64_t* starts,
                            const int* keep, const int* fade, const float* ramp, int F, const float* condition, float* out, int B,
                            int W, void* workspace, size_t workspace_bytes, void* stream, const ClipForm& link = ClipForm()) {
    if (!recording || !starts || !keep || !condition || !out || !workspace) return fail(c, LASS_ERR_ARG, who + ": null pointer");
    if (B <= 0) return fail(c, LASS_ERR_ARG, who + ": need B >= 1");
    if (W <= c->g.nfft / 2)
        return fail(c, LASS_ERR_ARG, who + ": a window must be longer than the reflect padding (W > " + std::to_string(c->g.nfft / 2) + ")");
    if (total < W) return fail(c, LASS_ERR_ARG, who + ": the recording is shorter than one window (total < W)");
    const uintptr_t r0 = (uintptr_t)recording, o0 = (uintptr_t)out, bytes = (uintptr_t)total * sizeof(float);
    if (r0 < o0 + bytes && o0 < r0 + bytes) return fail(c, LASS_ERR_ARG, who + ": recording and out overlap");
    ClipForm cf{B, W, nullptr, starts, keep, total, fade, ramp, F};
    cf.planes = link.planes; cf.plane_stride = link.plane_stride; cf.out_plane_stride = link.out_plane_stride; cf.channels = link.channels;
    return separate_call(c, recording, condition, out, cf, workspace, workspace_bytes, stream, who.c_str());
}

int lass_separate_windows(lass_ctx* c, const float* recording, int64_t total, const int64_t* starts, const int* keep,
                          const float* condition, float* out, int B, int W, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    return separate_windows(c, "lass_separate_windows", recording, total, starts, keep, nullptr, nullptr, 0, condition, out, B, W,
                            workspace, workspace_bytes, stream);
}

int lass_separate_windows_faded(lass_ctx* c, const float* recording, int64_t total, const int64_t* starts, const int* keep,
                                const int* fade, const float* ramp, int F, const float* condition, float* out, int B, int W,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    const std::string who = "lass_separate_windows_faded";
    if (!fade || !ramp) return fail(c, LASS_ERR_ARG, who + ": null pointer");
    if (F < 1 || F > W) return fail(c, LASS_ERR_ARG, who + ": the fade length must lie in [1, W]");
    return separate_windows(c, who, recording, total, starts, keep, fade, ramp, F, condition, out, B, W, workspace, workspace_bytes,
                            stream);
}

// ---- linked channels: one mask from the guide, applied to every plane ----------------------------------
// The checks that only the linked calls have: `n` floats per channel array (B * L, or total).  `link` receives the four fields.
static int check_linked(lass_ctx* c, const std::string& who, const float* guide, int64_t n, const float* planes, int64_t plane_stride,
                        int channels, const float* out, int64_t out_plane_stride, ClipForm* link) {
    if (c->g.variant != 0) return fail(c, LASS_ERR_ARG, who + ": linked channels are ResUNet30's (not a multi-STFT context)");
    if (!planes) return fail(c, LASS_ERR_ARG, who + ": null pointer");
    if (channels < 1 || channels > LASS_MAX_LINKED_CHANNELS)
        return fail(c, LASS_ERR_ARG, who + ": need 1 <= channels <= " + std::to_string(LASS_MAX_LINKED_CHANNELS));
    if (n > 0 && (plane_stride < n || out_plane_stride < n))
        return fail(c, LASS_ERR_ARG, who + ": a plane stride is shorter than one channel's array (" + std::to_string(n) + " floats)");
    if (guide && out && n > 0) {
        const uintptr_t bytes = (uintptr_t)n * sizeof(float);
        const auto meets = [&](const float* a, const float* b) {
            return (uintptr_t)a < (uintptr_t)b + bytes && (uintptr_t)b < (uintptr_t)a + bytes;
        };
        for (int o = 0; o < channels; ++o) {
            const float* oc = out + (size_t)o * out_plane_stride;
            if (meets(oc, guide)) return fail(c, LASS_ERR_ARG, who + ": out overlaps the guide");
            for (int i = 0; i < channels; ++i)
                if (meets(oc, planes + (size_t)i * plane_stride)) return fail(c, LASS_ERR_ARG, who + ": out overlaps an input plane");
        }
    }
    link->planes = planes; link->plane_stride = plane_stride; link->out_plane_stride = out_plane_stride; link->channels = channels;
    return 0;
}

int lass_separate_ragged_linked(lass_ctx* c, const float* guide, const int* lengths, const float* planes, int64_t plane_stride,
                                int channels, const float* condition, float* out, int64_t out_plane_stride, int B, int L,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    const std::string who = "lass_separate_ragged_linked";
    ClipForm cf{B, L, lengths};
    if (int r = check_linked(c, who, guide, B > 0 && L > 0 ? (int64_t)B * L : 0, planes, plane_stride, channels, out, out_plane_stride, &cf))
        return r;
    return separate_call(c, guide, condition, out, cf, workspace, workspace_bytes, stream, "lass_separate_ragged_linked");
}

int lass_separate_windows_linked(lass_ctx* c, const float* guide, int64_t total, const int64_t* starts, const int* keep, const int* fade,
                                 const float* ramp, int F, const float* planes, int64_t plane_stride, int channels,
                                 const float* condition, float* out, int64_t out_plane_stride, int B, int W, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!c) return LASS_ERR_ARG;
    const std::string who = "lass_separate_windows_linked";
    if ((fade == nullptr) != (ramp == nullptr)) return fail(c, LASS_ERR_ARG, who + ": fade and ramp go together");
    if (fade && (F < 1 || F > W)) return fail(c, LASS_ERR_ARG, who + ": the fade length must lie in [1, W]");
    ClipForm link;
    if (int r = check_linked(c, who, guide, total > 0 ? total : 0, planes, plane_stride, channels, out, out_plane_stride, &link)) return r;
    return separate_windows(c, who, guide, total, starts, keep, fade, ramp, fade ? F : 0, condition, out, B, W, workspace, workspace_bytes,
                            stream, link);
}

// lass_masked_stft and lass_masked_stft_windows behind their argument checks
static int masked_stft(lass_ctx* c, const char* who, const float* wav, const ClipForm& cf, const float* m_re, const float* m_im,
                       float* y_re, float* y_im, void* stream) {
    if (c->g.variant != 0) return fail(c, LASS_ERR_ARG, std::string(who) + ": linked channels are ResUNet30's (not a multi-STFT context)");
    int r = check_ready(c);
    if (r) return r;
    if (!wav || !m_re || !m_im || !y_re || !y_im || cf.B <= 0 || cf.L <= c->g.nfft / 2 || (cf.starts && cf.total < cf.L))
        return fail(c, LASS_ERR_ARG, std::string(who) + ": bad argument (n_fft/2 < L, W <= total)");
    HIP_TRY(c, lass_launch_masked_stft(wav, cf, c->g.nfft, c->g.hop, 1 + cf.L / c->g.hop, c->g.wins[c->g.mask_br], m_re, m_im, y_re, y_im,
                                       c->tw2k, (hipStream_t)stream));
    return 0;
}

int lass_masked_stft(lass_ctx* c, const float* plane, const int* lengths, int B, int L, const float* m_re, const float* m_im,
                     float* y_re, float* y_im, void* stream) {
    if (!c) return LASS_ERR_ARG;
    return masked_stft(c, "lass_masked_stft", plane, ClipForm{B, L, lengths}, m_re, m_im, y_re, y_im, stream);
}

int lass_masked_stft_windows(lass_ctx* c, const float* recording, int64_t total, const int64_t* starts, int B, int W,
                             const float* m_re, const float* m_im, float* y_re, float* y_im, void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (!starts) return fail(c, LASS_ERR_ARG, "lass_masked_stft_windows: null pointer");
    return masked_stft(c, "lass_masked_stft_windows", recording, ClipForm{B, W, nullptr, starts, nullptr, total}, m_re, m_im, y_re, y_im,
                       stream);
}

int lass_set_graph_replay(lass_ctx* c, int enabled) {
    if (!c) return LASS_ERR_ARG;
    c->use_graph = enabled != 0;  // captured graphs stay cached: switching back on replays them again
    return 0;
}

int lass_set_wino4_splits(lass_ctx* c, int splits) {
    if (!c || (splits != 0 && splits != 1 && splits != 2 && splits != 4)) return fail(c, LASS_ERR_ARG, "lass_set_wino4_splits: 0, 1, 2 or 4");
    c->cfg.ksplit_force = splits;
    ++c->gen;  // captured graphs hold the launches of the previous choice (and workspace sizes follow it)
    return 0;
}

int lass_set_wino4_vprep(lass_ctx* c, int mode) {
    if (!c || mode < 0 || mode > 2) return fail(c, LASS_ERR_ARG, "lass_set_wino4_vprep: 0, 1 or 2");
    c->cfg.vprep_mode = mode;
    ++c->gen;  // as lass_set_wino4_splits: other launches, another workspace size
    return 0;
}

int lass_set_head_fold(lass_ctx* c, int enabled) {
    if (!c || (enabled != 0 && enabled != 1)) return fail(c, LASS_ERR_ARG, "lass_set_head_fold: 0 or 1");
    c->cfg.head_fold = enabled != 0;
    ++c->gen;  // captured graphs hold the launch of the previous choice
    return 0;
}

int lass_set_head_sc_fold(lass_ctx* c, int enabled) {
    if (!c || (enabled != 0 && enabled != 1)) return fail(c, LASS_ERR_ARG, "lass_set_head_sc_fold: 0 or 1");
    c->cfg.head_sc_fold = enabled != 0;
    ++c->gen;  // as lass_set_wino4_splits: other launches, another workspace size
    return 0;
}

int lass_set_pw_split(lass_ctx* c, int enabled) {
    if (!c || (enabled != 0 && enabled != 1)) return fail(c, LASS_ERR_ARG, "lass_set_pw_split: 0 or 1");
    c->cfg.pw_split = enabled != 0;
    ++c->gen;  // captured graphs hold the launches of the previous choice
    return 0;
}

int lass_set_wino4_gemm(lass_ctx* c, int enabled) {
    if (!c || (enabled != 0 && enabled != 1)) return fail(c, LASS_ERR_ARG, "lass_set_wino4_gemm: 0 or 1");
    c->cfg.wino4_gemm = enabled != 0;
    ++c->gen;  // as lass_set_wino4_splits: other launches, another workspace size
    return 0;
}

int lass_set_wino4_vprep_buffer(lass_ctx* c, float* v, size_t floats) {
    if (!c || (v && !floats)) return fail(c, LASS_ERR_ARG, "lass_set_wino4_vprep_buffer: a buffer and its size, or NULL");
    c->stage_v_user = v;
    c->stage_v_user_floats = v ? floats : 0;
    return 0;
}

int lass_graph_stats(const lass_ctx* c, long* captures, long* replays) {
    if (!c) return LASS_ERR_ARG;
    if (captures) *captures = c->g_captures;
    if (replays) *replays = c->g_replays;
    return c->use_graph ? 1 : 0;
}

int lass_separate_components(lass_ctx* c, const float* const* mag, const float* cos_mask, const float* sin_mask,
                             const float* condition, float* out, int B, int L, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (!c) return LASS_ERR_ARG;
    if (!mag || !cos_mask || !sin_mask) return fail(c, LASS_ERR_ARG, "lass_separate_components: null pointer");
    Components comp;
    for (int k = 0; k < kMaxBranches; ++k) comp.mag[k] = k < c->g.nbr ? mag[k] : nullptr;
    comp.cosv = cos_mask; comp.sinv = sin_mask;
    return separate_impl(c, nullptr, &comp, condition, out, ClipForm{B, L}, make_plan(c, B, L), workspace, workspace_bytes, stream,
                         "lass_separate_components");
}

int lass_set_profiling(lass_ctx* c, int enabled) {
    if (!c) return LASS_ERR_ARG;
    if (enabled && c->ev_pool.size() < 2 * kProfPairs) {
        HIP_TRY(c, hipSetDevice(c->device));
        c->pending.reserve(kProfPairs);
        while (c->ev_pool.size() < 2 * kProfPairs) {
            hipEvent_t e;
            HIP_TRY(c, hipEventCreate(&e));
            c->ev_pool.push_back(e);
        }
    }
    c->profiling = enabled != 0;
    return 0;
}
int lass_profile_count(const lass_ctx* c) { return c ? P_COUNT : LASS_ERR_ARG; }
int lass_profile_get(lass_ctx* c, int i, const char** name, double* ms, int* launches) {
    if (!c || i < 0 || i >= P_COUNT) return LASS_ERR_ARG;
    prof_collect(c);
    if (name) *name = c->prof[i].name;
    if (ms) *ms = c->prof[i].ms;
    if (launches) *launches = c->prof[i].launches;
    return 0;
}
int lass_profile_reset(lass_ctx* c) {
    if (!c) return LASS_ERR_ARG;
    prof_collect(c);
    for (auto& p : c->prof) { p.ms = 0; p.launches = 0; }
    return 0;
}

}  // extern "C"
