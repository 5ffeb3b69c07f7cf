// workspace_plan.h - what one lass_separate call does, as a value computed once: the layout of its workspace (Plan), and whether
// the call runs whole or as two half-batches with the bytes either takes (CallPlan).  The ONE place behind lass_workspace_bytes,
// lass_workspace_tensor, the argument checks and the launches of lass_separate & co (api.hip).  Host only and free of HIP, as
// conv_route.h, whose walk over the call's blocks (plan_separate) it reads.  tools/workspace_table.cpp prints it;
// tests/test_workspace_plan_cpu.py holds the layout's invariants and tests/test_gpu_workspace_plan.py ties the C-ABI to that table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "conv_route.h"

// Model geometry.  variant 0 = ResUNet30 (models/resunet.py): one analysis branch, n_fft = win, at one of two STFT geometries -
// (1024, hop 160), the reference's 16 kHz layout (lass_create), or (2048, hop 320), the 32 kHz layout of the same network
// (lass_create_stft: 1025-bin bn0, 1024-bin images, the same durations of 64 ms / 10 ms).
// variant 1 = the multi-resolution-STFT separator (models/resunet_with_multistft.py under the authored spec of
// DESIGN.md / lass_amd/arch.py): nbr analysis windows at a common n_fft, one pre_conv + encoder_block1 per window,
// channel-concatenated pools / skips, shared trunk, mask and iSTFT on the branch `mask_br`; always hop 160.
struct Geometry {
    int variant = 0;
    int nbr = 1;
    int wins[LASS_MAX_STFT_WINDOWS] = {1024, 0, 0, 0};
    int nfft = 1024, nbins = 513, fcrop = 512;
    int hop = LASS_HOP;  // frames are 1 + L / hop; a ragged bucket is 32 * hop samples wide
    int mask_br = 0;
    int magphase_sem = 0;  // 0: base.py:83-88 clamp on |X|^2; 1: torchlibrosa magphase (precomputed-STFT wire format)
};

// Everything of a context that a plan depends on
struct PlanInputs {
    const Geometry& g;
    const ModelTable& m;
    const RouteCfg& cfg;
    int n_shift;           // FiLM width: the channels of all sites
    bool head_sc_weights;  // lass_finalize composed the head's shortcut weights for this checkpoint (plan_separate)
};

struct Plan {
    bool valid = false;  // make_plan accepted (B, L)
    int B = 0, L = 0, T = 0, Tp = 0;
    size_t total = 0;
    size_t mag = 0, cosv = 0, sinv = 0, x0[LASS_MAX_STFT_WINDOWS] = {0}, shift = 0, a2 = 0, cat[6] = {0}, pool[6] = {0}, center = 0,
           decout[6] = {0}, oreal = 0, oimag = 0;
    // One slot each, sized to the largest block (sp.kpart_floats / v_floats / m_floats; the launches of a plan run in stream order):
    // split-K partials of the 32 x 16 Winograd blocks, the V image of the V-from-memory layers, the product image of the gemm route
    size_t kpart = 0, vprep = 0, mgemm = 0;
    // conv_route.h's head_sc_fold (sp.head_sc_fold): the folded head's shortcut logits as two sets of planes [B][3][Tp][fcrop], one
    // written by encoder_block1.conv2 and one by decoder_block6's transposed conv (last in the plan: no other offset depends on the switch)
    size_t lg_skip = 0, lg_up = 0;
    // every slot bump handed out, in order: (offset, bytes) - what the layout's invariants are checked on (tools/workspace_table.cpp)
    static constexpr int kMaxSlots = 40;
    int nslots = 0;
    size_t slot_off[kMaxSlots] = {0}, slot_bytes[kMaxSlots] = {0};
    Levels lv;         // encoder block spatial sizes
    SeparatePlan sp;   // every block's BlockIO, route and bf16 form, the transposed convs' families (conv_route.h)
};

inline size_t round256(size_t bytes) { return (bytes + 255) / 256 * 256; }

inline size_t bump(Plan& pl, size_t floats) {
    const size_t off = pl.total;
    pl.total += round256(floats * sizeof(float));
    if (pl.nslots < Plan::kMaxSlots) {
        pl.slot_off[pl.nslots] = off;
        pl.slot_bytes[pl.nslots++] = pl.total - off;
    }
    return off;
}

// The conv kernels address one clip's tensors through 32-bit buffer descriptors and byte offsets, so the largest per-clip
// tensor (decoder_block6's concat at full resolution, f32) bounds the clip length: below 4 GiB (all offset arithmetic of
// the f32 Winograd and the bf16 kernels is unsigned; both exercised by the 3.15-GB concat of the 30 s @ 32 kHz multi-STFT
// clip).  ResUNet30 at 16 kHz: 131 072 B per frame -> 2^32 at 32 768 frames (327 s); ResUNet30 at the 32 kHz geometry (64 ch x 1024
// bins): 262 144 B per frame -> 2^32 at 16 384 frames (163 s at hop 320); the multi-STFT model (128 ch x 1024 bins): 524 288 B per
// frame -> 2^32 at 8 192 frames (40.9 s at 32 kHz).  Longer inputs go through chunk_inference / separate_long.
// Refused (valid stays false): B < 1, L <= n_fft / 2, or L beyond that limit.
inline Plan make_plan(const PlanInputs& in, int B, int L) {
    Plan pl;
    const Geometry& g = in.g;
    const ModelTable& m = in.m;
    if (B <= 0 || L <= g.nfft / 2) return pl;
    pl.B = B; pl.L = L;
    pl.T = 1 + L / g.hop;
    pl.Tp = (pl.T + 31) / 32 * 32;
    const size_t clip_max = (size_t)m.dec_cat[5] * pl.Tp * g.fcrop * sizeof(float);
    if (clip_max > 0xFFFF0000ull) return pl;
    const size_t spec = (size_t)B * pl.T * g.nbins;
    pl.mag = bump(pl, spec); pl.cosv = bump(pl, spec); pl.sinv = bump(pl, spec);
    for (int k = 0; k < g.nbr; ++k) pl.x0[k] = bump(pl, (size_t)B * pl.Tp * g.fcrop);
    pl.shift = bump(pl, (size_t)B * in.n_shift);
    pl.lv = model_levels(m, pl.Tp);
    size_t a2max = 0;
    for (int i = 0; i < 7; ++i) {
        const size_t o = (size_t)B * m.E[i].cout * pl.lv.eh[i] * pl.lv.ew[i];
        if (o > a2max) a2max = o;
        if (i < 6) pl.pool[i] = bump(pl, (size_t)B * m.E[i].cout * (i == 0 ? g.nbr : 1) * pl.lv.eh[i + 1] * pl.lv.ew[i + 1]);
    }
    pl.center = bump(pl, (size_t)B * m.E[6].cout * pl.lv.eh[6] * pl.lv.ew[6]);
    for (int d = 0; d < 6; ++d) {
        const int e = 5 - d;  // decoder d concatenates the skip of encoder e
        const size_t hw = (size_t)pl.lv.eh[e] * pl.lv.ew[e];
        pl.cat[d] = bump(pl, (size_t)B * m.dec_cat[d] * hw);
        pl.decout[d] = bump(pl, (size_t)B * m.D[d].cout * hw);
    }
    pl.a2 = bump(pl, a2max);
    pl.oreal = bump(pl, spec); pl.oimag = bump(pl, spec);
    // every block at its level's image size, with what lass_separate fuses into it.  (A half-batch plan has its own slots: the two
    // branches of the replayed graph never share partials.)
    pl.sp = plan_separate(in.cfg, m, pl.lv, B, in.head_sc_weights);
    if (pl.sp.kpart_floats) pl.kpart = bump(pl, pl.sp.kpart_floats);
    if (pl.sp.v_floats) pl.vprep = bump(pl, pl.sp.v_floats);
    if (pl.sp.m_floats) pl.mgemm = bump(pl, pl.sp.m_floats);
    if (pl.sp.head_sc_fold) {
        pl.lg_skip = bump(pl, (size_t)B * 3 * pl.lv.eh[0] * pl.lv.ew[0]);
        pl.lg_up = bump(pl, (size_t)B * 3 * pl.lv.eh[0] * pl.lv.ew[0]);
    }
    pl.valid = true;
    return pl;
}

// The tensors of a plan that lass_workspace_tensor names, in the order it matches them: (B, C, H, W) at `offset` bytes, strides in floats
struct PlanTensor {
    std::string name;
    size_t offset;
    int64_t shape[4], strides[4];
};
inline std::vector<PlanTensor> plan_tensors(const PlanInputs& in, const Plan& pl) {
    const Geometry& g = in.g;
    const ModelTable& m = in.m;
    std::vector<PlanTensor> v;
    const auto put = [&](const std::string& name, size_t off, int64_t C, int64_t H, int64_t W, int64_t bs) {
        v.push_back(PlanTensor{name, off, {pl.B, C, H, W}, {bs, H * W, W, 1}});
    };
    const int64_t spec = (int64_t)pl.T * g.nbins;
    put("mag", pl.mag, 1, pl.T, g.nbins, spec);
    put("cos", pl.cosv, 1, pl.T, g.nbins, spec);
    put("sin", pl.sinv, 1, pl.T, g.nbins, spec);
    put("out_real", pl.oreal, 1, pl.T, g.nbins, spec);
    put("out_imag", pl.oimag, 1, pl.T, g.nbins, spec);
    for (int k = 0; k < g.nbr; ++k)
        put(g.variant == 0 ? std::string("x0") : "x0." + std::to_string(g.wins[k]), pl.x0[k], 1, pl.Tp, g.fcrop, (int64_t)pl.Tp * g.fcrop);
    for (int i = 0; i < 7; ++i) {
        const EncSpec& e = m.E[i];
        const int64_t H = pl.lv.eh[i], W = pl.lv.ew[i];
        const int64_t C = (int64_t)e.cout * (i == 0 ? g.nbr : 1);  // encoder_block1: all branches, channel-concatenated
        if (i == 6) {
            put(e.name, pl.center, C, H, W, C * H * W);
        } else {
            const int d = 5 - i;  // the skip lives in place behind the transposed-conv half of decoder d's concat
            put(e.name, pl.cat[d] + (size_t)m.D[d].cout * H * W * sizeof(float), C, H, W, (int64_t)m.dec_cat[d] * H * W);
            put(std::string(e.name) + ".pool", pl.pool[i], C, H / e.dh, W / e.dw, C * (H / e.dh) * (W / e.dw));
        }
    }
    // the head's shortcut logits of the head_sc_fold route (only where the plan has them)
    if (pl.sp.head_sc_fold) {
        const int64_t H = pl.lv.eh[0], W = pl.lv.ew[0];
        put("head_sc.skip", pl.lg_skip, 3, H, W, 3 * H * W);
        put("head_sc.up", pl.lg_up, 3, H, W, 3 * H * W);
    }
    for (int d = 0; d < 6; ++d) {
        const int64_t H = pl.lv.eh[5 - d], W = pl.lv.ew[5 - d], C = m.D[d].cout;
        put(std::string(m.D[d].name) + ".up", pl.cat[d], C, H, W, (int64_t)m.dec_cat[d] * H * W);
        put(m.D[d].name, pl.decout[d], C, H, W, C * H * W);
    }
    return v;
}

// A batch is split into two overlapping half-batches when it is large enough for each half to fill the GPU on its own
// (split_batch: lass_ctx's LASS_SPLIT value - 0 never, 1 inside a captured graph only, 2 eager launches too)
inline bool split_halves(int split_batch, bool profiling, int B) { return split_batch > 0 && !profiling && B >= 8 && (B % 2) == 0; }

// One call of lass_separate & co: the whole-batch plan, the plan of one half, and whether the call runs as two half-batches -
// their plans then lie side by side in the workspace, each rounded to 256 bytes.
struct CallPlan {
    Plan whole, half;    // half: of B / 2 clips, planned only where split_halves holds
    bool split = false;  // the launches run as two half-batches
    size_t need = 0;     // bytes the call addresses: whole.total, or the two halves where they are more and fit workspace_bytes
    size_t half_bytes() const { return round256(half.total); }
};
constexpr size_t kNoWorkspaceLimit = ~(size_t)0;  // workspace_bytes of a call that only asks (lass_workspace_bytes)

// capturing: the launches go into a stream capture (the replayed graph), not onto the caller's stream
inline CallPlan plan_call(const PlanInputs& in, int B, int L, int split_batch, bool profiling, bool capturing, size_t workspace_bytes) {
    CallPlan cp;
    cp.whole = make_plan(in, B, L);
    cp.need = cp.whole.total;
    if (!cp.whole.valid || !split_halves(split_batch, profiling, B)) return cp;
    cp.half = make_plan(in, B / 2, L);
    const size_t both = 2 * cp.half_bytes();
    if (!cp.half.valid || both > workspace_bytes) return cp;  // a smaller workspace runs unsplit
    cp.split = capturing || split_batch >= 2;
    if (both > cp.need) cp.need = both;
    return cp;
}
