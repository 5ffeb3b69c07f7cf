// weight_plan.h - which weight images a model owns, in which layout, made from what (plan_weights: the ONE list lass_finalize
// allocates and fills, api.hip), and which of them a planned launch reads (route_images: the ONE check run_resblock and run_upconv
// make in front of a block's first launch).  The rules for which images exist are conv_route.h's predicates (wino4_images,
// lass_wino4_gemm_weights, lass_pw_split_*_weights, bf16_*_weights) and the two head rules below; the list reads only what is fixed
// when lass_finalize runs - the compute mode, wino4_mincin, the model table and the rows of after_conv - and no switch that a
// lass_set_* can throw afterwards: every image a later switch can route to is kept.  Host only and free of HIP, as conv_route.h.
// tools/weight_table.cpp prints both halves; tests/test_weight_plan_cpu.py holds route_images inside plan_weights over the grid of
// frame counts and switches, and the element counts against lass_amd/arch.py.
#pragma once
#include <stdint.h>

#include <vector>

#include "head_fold.h"

enum WeightSlot {
    // ---- per residual block (checkpoint layouts: conv (cout, cin, 3, 3), shortcut (cout, cin, 1, 1))
    W1, W2,            // conv.hip: conv1 / conv2 re-laid-out, [cin][tap][cout] f32
    WSC,               // conv.hip, wino4.hip, pw_gemm.hip: the 1x1 shortcut, [cin][cout] f32
    U1, U2,            // wino.hip: conv1 / conv2 in the F(2x2,3x3) domain, U[16][cin][cout] f32 (f32 mode)
    USC,               // wino.hip: the shortcut in that domain, [4][cin][cout] f32
    U1F, U2F,          // wino4.hip: conv1 / conv2 in the F(4x4,3x3) domain, LDS images of 36 cin cout f32 (wino4_images)
    U1G, U2G,          // wino4_gemm.hip: U1F / U2F as three bf16 pieces, [36][3][cin / 8][cout][8] (lass_wino4_gemm_weights)
    WSC3,              // pw_gemm.hip, split kernel: WSC as three bf16 pieces, [3][cin / 8][cout][8] (lass_pw_split_shortcut_weights)
    B1, B2, BSC16,     // conv_bf16.hip, conv_bf16_fused.hip: bf16 copies, [cin / 16][tap][2][cout][8] (the bf16 modes)
    B1L, B2L, BSCL,    // ... their lo halves bf16(w - float(bf16(w))), same layouts (bf16x3)
    U2H, WSCH, BH,     // wino4.hip, folded head (decoder_block6): conv2 and the shortcut composed with after_conv (head_fold.h) -
                       // compact U images per 8-channel chunk, Wsc' [cin][16], b' [16], f32
    // ---- per decoder's transposed conv (checkpoint layout (cin, cout, uh, uw) == [cin][n])
    UP16, UP16L,       // conv_bf16.hip, conv_bf16_fused.hip: bf16 hi / lo, transposed
    UP3,               // pw_gemm.hip, split kernel: three bf16 pieces, [3][cin / 8][n][8] (lass_pw_split_tconv_weights)
    // ---- per context
    UP_SC,             // decoder_block6's shortcut over the up-sampled half of its concat composed with its transposed conv, [4][32][64]
                       // f32: read by nothing but the launch that rounds it to ...
    UP_SC16,           // conv_bf16_fused.hip (dec6u_fused_bf16_kernel): ... its bf16 copy, [4][2][128] units
    HS_WT, HS_WSKIP,   // tconv_logits.hip: Wt' [cin][64]; wino4.hip (encoder_block1.conv2's epilogue): Wsc'_skip [3][32] (head_fold.h), f32
    kWeightSlots
};
constexpr int kBlockSlots = UP16, kDecoderSlotsEnd = UP_SC;  // [0, UP16) a block's, [UP16, UP_SC) a decoder's, the rest the context's

using SlotSet = uint32_t;  // bit s: WeightSlot s
constexpr SlotSet slots() { return 0; }
template <class... S>
constexpr SlotSet slots(WeightSlot s, S... rest) { return (SlotSet(1) << s) | slots(rest...); }

// One owner's images by slot; a value-initialised one has none
struct WeightImages {
    void* p[kWeightSlots] = {};
    const float* f32(WeightSlot s) const { return (const float*)p[s]; }
};

// How an image is made: one launcher of kernels.h each, or a host composition of head_fold.h.  (rows, cols, taps) are the launcher's
// matrix arguments; an image holds factor x rows x cols x taps elements.
enum WeightForm {
    WF_RELAYOUT,                                     // lass_launch_relayout_conv (Cout, Cin, taps): [cin][tap][cout] f32
    WF_BF16, WF_BF16_LO, WF_BF16_T, WF_BF16_T_LO,    // lass_launch_weights_bf16 (Cout, Cin, taps): hi / lo, plain / transposed
    WF_F2X2, WF_F2X2_SC,                             // lass_launch_wino_weights, lass_launch_wino_shortcut_weights (Cout, Cin): 16 / 4 points
    WF_F4X4,                                         // lass_launch_wino4_weights (Cout, Cin): 36 points
    WF_F4X4_SPLIT3,                                  // lass_launch_wino4_gemm_weights (Cout, Cin), from the F(4x4,3x3) image: 3 pieces of 36 points
    WF_PW_SPLIT3,                                    // lass_launch_pw_split_weights (K, N), from a [K][N] f32 matrix: 3 pieces
    WF_UP_SC,                                        // lass_launch_compose_up_shortcut: (4 Nsc, Cin) f32
    WF_HEAD_U4, WF_HEAD_WSC, WF_HEAD_BIAS,           // compose_head_fold: HeadFold::u4 (chunks, kHeadFoldU4Floats), wsc (K, 16), bias (1, 16)
    WF_HEAD_SC_WT, WF_HEAD_SC_WSKIP                  // compose_head_sc_fold: HeadScFold::wt (Kt, 64), wskip (Q, Cskip)
};
inline bool weight_form_on_host(WeightForm f) { return f >= WF_HEAD_U4; }
inline bool weight_form_bf16(WeightForm f) { return (f >= WF_BF16 && f <= WF_BF16_T_LO) || f == WF_F4X4_SPLIT3 || f == WF_PW_SPLIT3; }
inline int weight_form_factor(WeightForm f) {
    return f == WF_F2X2 ? 16 : f == WF_F2X2_SC ? 4 : f == WF_F4X4 ? kWino4NXI : f == WF_F4X4_SPLIT3 ? 3 * kWino4NXI : f == WF_PW_SPLIT3 ? 3 : 1;
}

enum WeightOwner { OWN_BLOCK, OWN_DECODER, OWN_CONTEXT };

// The residual blocks of a model in lass_finalize's order: the nbr branch blocks (encoder_block1[s]), the 6 trunk blocks, the 6 decoders'
inline int model_blocks(const ModelTable& m) { return m.nbr + 12; }
inline BlockShape block_shape(const ModelTable& m, int b) {
    return b < m.nbr ? m.enc_shape(0) : b < m.nbr + 6 ? m.enc_shape(b - m.nbr + 1) : m.dec_shape(b - m.nbr - 6);
}

struct WeightItem {
    WeightOwner owner;
    int index;          // OWN_BLOCK: block_shape's b; OWN_DECODER: the decoder; OWN_CONTEXT: 0
    WeightSlot slot;
    WeightForm form;
    const char* param;  // the source: a checkpoint parameter under the owner's prefix ("conv1.weight"), or null and then ...
    int from;           // ... the owner's own image in that slot (U1G from U1F, WSC3 from WSC), or -1: a composition names its inputs
    int rows, cols, taps;
    size_t count;       // elements of the image, written here and nowhere else; elem_bytes each
    int elem_bytes;
};

// ---- the folded head: the shape half of the two compositions of head_fold.h.  Q: rows of after_conv, the one input that comes from
// the checkpoint's shapes.  The compositions can still decline (compose_head_fold / compose_head_sc_fold): the images are then absent.
// decoder_block6's conv2 and shortcut composed with after_conv: where conv2 has its F(4x4,3x3) image and the shortcut exists; the
// compact image the kernels read has rows for at most 3 logits
inline bool head_fold_weights(const RouteCfg& cfg, const ModelTable& m, int Q) {
    const BlockShape b = m.dec_shape(5);
    return wino4_images(cfg, b.cin, b.cout, b.width).u2f && b.cin != b.cout && Q > 0 && Q < kHeadFoldRows4;
}
// ... and the shortcut's two halves for the launches that produce its inputs (ResUNet30: the skip is ONE encoder_block1's output).
// The rule behind PlanInputs::head_sc_weights (workspace_plan.h).
inline bool head_sc_weights(const RouteCfg& cfg, const ModelTable& m, int Q) {
    const DecSpec& d = m.D[5];
    return head_fold_weights(cfg, m, Q) && m.windows == 0 && m.nbr == 1 && Q == 3 && m.dec_cat[5] == d.cout + kPreCh &&
           Q * d.uh * d.uw <= kHeadScLive;
}

// Every image of a model, in the order lass_finalize makes them (its launches keep their order on the stream)
inline std::vector<WeightItem> plan_weights(const RouteCfg& cfg, const ModelTable& m, int Q) {
    std::vector<WeightItem> v;
    WeightOwner owner = OWN_BLOCK;  // ... and index: whose images the add() calls below list
    int index = 0;
    const auto add = [&](WeightSlot slot, WeightForm form, const char* param, int from, int rows, int cols, int taps = 1) {
        v.push_back(WeightItem{owner, index, slot, form, param, from, rows, cols, taps,
                               (size_t)weight_form_factor(form) * rows * cols * taps, weight_form_bf16(form) ? 2 : 4});
    };
    const bool f32 = cfg.f32(), lo = cfg.mode == MODE_BF16X3;
    const char *c1 = "conv1.weight", *c2 = "conv2.weight", *sc = "shortcut.weight";
    for (index = 0; index < model_blocks(m); ++index) {
        const BlockShape s = block_shape(m, index);
        const int ci = s.cin, co = s.cout;
        add(W1, WF_RELAYOUT, c1, -1, co, ci, 9);
        add(W2, WF_RELAYOUT, c2, -1, co, co, 9);
        const Bf16Weights wt = bf16_block_weights(cfg, ci, co);  // the copies the bf16 plan counts on
        if (wt.pair) { add(B1, WF_BF16, c1, -1, co, ci, 9); add(B2, WF_BF16, c2, -1, co, co, 9); }
        if (wt.pair_lo) { add(B1L, WF_BF16_LO, c1, -1, co, ci, 9); add(B2L, WF_BF16_LO, c2, -1, co, co, 9); }
        if (f32) {
            add(U1, WF_F2X2, c1, -1, co, ci);
            add(U2, WF_F2X2, c2, -1, co, co);
            const Wino4Images im = wino4_images(cfg, ci, co, s.width);  // the routes plan_block can give the block
            if (im.u1f) add(U1F, WF_F4X4, c1, -1, co, ci);
            if (im.u2f) add(U2F, WF_F4X4, c2, -1, co, co);
            // ... and, for the convs plan_block can route through wino4_gemm.hip, the split of exactly those f32 images
            if (im.u1f && lass_wino4_gemm_weights(true, ci, co)) add(U1G, WF_F4X4_SPLIT3, nullptr, U1F, co, ci);
            if (im.u2f && lass_wino4_gemm_weights(true, co, co)) add(U2G, WF_F4X4_SPLIT3, nullptr, U2F, co, co);
        }
        if (ci == co) continue;
        add(WSC, WF_RELAYOUT, sc, -1, co, ci);
        if (wt.shortcut) add(BSC16, WF_BF16, sc, -1, co, ci);
        if (wt.shortcut_lo) add(BSCL, WF_BF16_LO, sc, -1, co, ci);
        if (f32) add(USC, WF_F2X2_SC, sc, -1, co, ci);
        if (lass_pw_split_shortcut_weights(f32, ci, co)) add(WSC3, WF_PW_SPLIT3, nullptr, WSC, ci, co);  // from the f32 kernel's matrix
    }
    owner = OWN_DECODER;
    for (index = 0; index < 6; ++index) {
        const DecSpec& d = m.D[index];
        const int N = d.cout * d.uh * d.uw;
        if (lass_pw_split_tconv_weights(f32, d.cin, N, d.uh)) add(UP3, WF_PW_SPLIT3, c1, -1, d.cin, N);
        if (bf16_tconv_weights(cfg, d)) add(UP16, WF_BF16_T, c1, -1, N, d.cin);
        if (bf16_tconv_weights(cfg, d) && lo) add(UP16L, WF_BF16_T_LO, c1, -1, N, d.cin);
    }
    owner = OWN_CONTEXT;
    index = 0;
    const DecSpec& d6 = m.D[5];
    const BlockShape b6 = m.dec_shape(5);
    if (bf16_up_sc_weights(cfg, m)) {  // from decoder_block6's shortcut.weight and its transposed conv's conv1.weight
        add(UP_SC, WF_UP_SC, nullptr, -1, 4 * b6.cout, d6.cin);
        add(UP_SC16, WF_BF16, nullptr, UP_SC, 4 * b6.cout, d6.cin);
    }
    // the host compositions, from decoder_block6's conv2 / shortcut, after_conv and the transposed conv in front
    if (head_sc_weights(cfg, m, Q)) {
        add(HS_WT, WF_HEAD_SC_WT, nullptr, -1, d6.cin, kHeadScCols);
        add(HS_WSKIP, WF_HEAD_SC_WSKIP, nullptr, -1, Q, b6.cin - d6.cout);
    }
    if (head_fold_weights(cfg, m, Q)) {
        owner = OWN_BLOCK;
        index = m.nbr + 11;  // decoder_block6
        add(U2H, WF_HEAD_U4, nullptr, -1, b6.cout / kWino4KC, kHeadFoldU4Floats);
        add(WSCH, WF_HEAD_WSC, nullptr, -1, b6.cin, kHeadFoldRows);
        add(BH, WF_HEAD_BIAS, nullptr, -1, 1, kHeadFoldRows);
    }
    return v;
}

// ---- the consumer half: the slots a planned launch reads.  Block slots are the block's own, decoder slots its decoder's.
// f32 (and, in the bf16 modes, a block their kernels do not take: plan_block's direct route)
inline SlotSet route_images(const BlockRoute& r) {
    const auto conv = [](const ConvRoute& c, WeightSlot w, WeightSlot u, WeightSlot uf, WeightSlot ug) -> SlotSet {
        const bool sc = c.kind == CONV2_SHORTCUT;  // the fused shortcut phase
        switch (c.family) {
            case CONV_DIRECT: return slots(w) | (sc ? slots(WSC) : 0);
            case CONV_F2X2: return slots(u) | (sc ? slots(USC) : 0);
            case CONV_F4X4:
                if (c.head_fold) return slots(U2H, WSCH, BH);  // in place of conv2's, the shortcut's and after_conv's
                if (c.head_sc_fold) return slots(uf, HS_WSKIP);  // encoder_block1.conv2 writing the skip's logit planes
                return c.gemm ? slots(ug) : slots(uf) | (sc ? slots(WSC) : 0);
            default: return 0;
        }
    };
    SlotSet s = conv(r.conv1, W1, U1, U1F, U1G) | conv(r.conv2, W2, U2, U2F, U2G);
    if (r.shortcut_gemm) s |= slots(WSC) | (r.pw_split ? slots(WSC3) : 0);
    return s;
}
// the bf16 kernels, by the block's form and the copies bf16_block_weights gives it
inline SlotSet route_images(const Bf16Block& b, const Bf16Weights& wt) {
    if (b.form == BF16_NONE) return 0;
    return slots(B1, B2) | (wt.pair_lo ? slots(B1L, B2L) : 0) | (wt.shortcut ? slots(BSC16) : 0) | (wt.shortcut_lo ? slots(BSCL) : 0) |
           (b.form == BF16_DEC6U ? slots(UP16, UP_SC16) : 0);
}
// a transposed conv (the direct kernel reads the checkpoint's own matrix)
inline SlotSet route_images(const UpRoute& r, const RouteCfg& cfg) {
    switch (r.family) {
        case UP_GEMM: return r.pw_split ? slots(UP3) : 0;
        case UP_BF16: return slots(UP16) | (cfg.mode == MODE_BF16X3 ? slots(UP16L) : 0);
        case UP_LOGITS: return slots(HS_WT);
        default: return 0;
    }
}
