// conv_route.h - which kernel family runs the 3x3 convs of a residual block in f32, and the workspace that takes; in the bf16
// modes which blocks run the bf16 kernels, in which form (two launches or one fused kernel), and which tensors travel between
// launches as blocked bf16 copies; in every mode the family of each transposed conv; and the model table with its level walk.
// The ONE rule behind the launches of run_resblock and run_upconv (api.hip), the predicates that weight_plan.h lists the weight
// images and bf16 copies of lass_finalize by (wino4_images, lass_wino4_gemm_weights, lass_pw_split_*_weights, bf16_*_weights),
// and the shape halves of the lass_*_supported predicates of wino.hip, wino4.hip, wino4_gemm.hip, pw_gemm.hip, conv_bf16.hip and
// conv_bf16_fused.hip; and, as plan_separate, the ONE walk over the blocks of a lass_separate: what each block is called with, its
// route and hand-overs, the head_sc_fold decision and the workspace the routes take.  workspace_plan.h sizes the workspace from that
// walk (make_plan) and lass_separate sets each block's fusions from it (api.hip: separate_impl); run_resblock and run_upconv derive
// the route again from the pointers they are handed and refuse a contradiction (the stage calls come the same way, on a default
// site).  Host only and free of HIP: any C++17 compiler builds it.
// tools/route_table.cpp prints the rule as a table; tests/test_wino4_routing_cpu.py holds lass_amd.arch.wino4_routed (the Python
// mirror that bench.py's executed-FLOP accounting reads) against that table, tests/test_wino4_gemm_routing_cpu.py pins the gemm
// route (ConvRoute::gemm), tests/test_bf16_routing_cpu.py pins the bf16 plan
// and tests/test_gpu_bf16_routes.py ties the printed launch counts to what a lass_separate runs.
#pragma once
#include <stddef.h>

enum ConvKind { CONV1_ACT = 0, CONV2_IDENT = 1, CONV2_SHORTCUT = 2, TCONV_ACT = 3, CONV1_ACT_PRE = 4, CONV2_IDENT_PRE = 5 };

constexpr int kPreCh = 32;  // channels of pre_conv and of encoder_block1

// ---- chunk and tile constants of the kernel files (each file names its own from these) ---------------------------------------
constexpr int kWinoKC = 8;                              // wino.hip: input channels of a chunk
constexpr int kWino4KC = 8;                             // wino4.hip: input channels of a chunk
constexpr int kWino4NXI = 36;                           // wino4.hip: points of the 6 x 6 transform domain
constexpr int kWino4VFloats = kWino4NXI * 4 * 32 * 2;   // wino4.hip: floats of one (block, chunk) of the transformed input
constexpr int kHeadFoldRows = 16;                       // wino4.hip, folded output head: rows of the one MFMA tile the 3 logits are padded to
constexpr int kPwGemmNB = 128;                          // pw_gemm.hip: couts of a workgroup
constexpr int kPwGemmKC = 16;                           // pw_gemm.hip: k rows of a chunk
constexpr int kBf16FusedTileW = 32;                     // conv_bf16_fused.hip: columns of an output tile

// wino4.hip: images that tile only into 32-row x 16-column blocks (the 16-bin level of a clip whose frame count at that level
// is a multiple of 32); the 8 x 64 / 16 x 32 blocks take every geometry they fit
inline bool lass_wino4_narrow(int H, int W) { return W % 32 == 16 && H % 32 == 0; }
// The block geometry of an H x W image, as tile columns per block (TC; a block is 32 tiles of 4 x 4 outputs): 16 = 8 rows x 64
// columns, 8 = 16 rows x 32 columns, 4 = 32 rows x 16 columns (narrow), 0 = none fits.  The one rule behind lass_wino4_shape,
// the launchers and the sizing of the V image.
inline int lass_wino4_block_tc(int H, int W) {
    if (W % 64 == 0 && H % 8 == 0) return 16;
    if (W % 32 == 0 && H % 16 == 0) return 8;
    return lass_wino4_narrow(H, W) ? 4 : 0;
}

// ---- shape halves of the support predicates ------------------------------------------------------------------------------------
// One conv launch as the predicates see it: ConvArgs without its pointers (kernels.h: lass_conv_shape).  The kernel files'
// lass_*_supported are "shape function && the pointers are there".
struct ConvShape {
    int Cin = 0, N = 0, Nw = 0, H = 0, W = 0;
    int Cin2 = 0;       // CONV2_SHORTCUT: channels of the 1x1 shortcut's input
    bool pool = false;  // fused avg-pool of the output, pool_h x 2
    int pool_h = 2;
    bool head = false;  // fused output head (after_conv + mask) instead of the output
};

// wino.hip, F(2x2,3x3): W a multiple of 32 (or 16 / 8 bins with 64-cout groups), H even
inline bool lass_wino_shape(const ConvShape& s) {
    const bool w_ok = (s.W >= 32 && (s.W % 32) == 0) || ((s.W == 16 || s.W == 8) && s.N % 64 == 0);
    return w_ok && (s.H % 2) == 0 && s.Cin % (2 * kWinoKC) == 0 && s.N % 32 == 0 && (s.Nw % 32) == 0;
}

// wino4.hip, F(4x4,3x3), whole or split-K (splits workgroups per block, cout group and clip).  One clip's input is addressed
// through a 32-bit buffer descriptor.
inline bool lass_wino4_shape(ConvKind kind, const ConvShape& s, int splits = 1) {
    const int tc = lass_wino4_block_tc(s.H, s.W);
    if (!(tc != 0 && s.Cin % kWino4KC == 0 && s.N % 32 == 0 && s.Nw % 32 == 0 &&
          (unsigned long long)s.Cin * s.H * s.W * 4ull < 0xFFFF0000ull))
        return false;
    const bool pool2 = !s.pool || s.pool_h == 2;
    if (tc == 4) {  // narrow: conv1 and the identity conv2 (fused 2 x 2 or 1 x 2 pool), whole or split-K with the combine behind it
        if (splits != 1 && !(splits >= 2 && splits <= s.Cin / kWino4KC && s.N == s.Nw)) return false;
        return kind == CONV1_ACT || (kind == CONV2_IDENT && !s.head && (pool2 || s.pool_h == 1));
    }
    if (splits != 1) return false;
    switch (kind) {
        case CONV1_ACT:
            return true;
        case CONV1_ACT_PRE:  // encoder_block1.conv1: the 32 input channels are formed from x0
            return s.Cin == kPreCh;
        case CONV2_IDENT_PRE:  // encoder_block1.conv2: residual = pre_conv(x0), fused 2x2 avg-pool
            return s.N == kPreCh && s.Nw == kPreCh && pool2;
        case CONV2_IDENT:  // conv2 + residual from memory (the shortcut layers whose 1x1 conv runs in pw_gemm.hip), fused 2x2 avg-pool
            return !s.head && pool2;
        case CONV2_SHORTCUT:  // conv2 + 1x1 shortcut (+ fused 2x2 avg-pool, or decoder_block6's fused output head)
            return s.Cin2 % 16 == 0 && pool2 && (!s.head || (s.N == 32 && s.Nw == 32 && !s.pool));
        default:
            return false;
    }
}

// wino4.hip, decoder_block6's conv2 with after_conv folded into its weights and its shortcut's (head_fold.h): the shape of the
// unfolded launch - s.N = s.Nw = 32 names the conv that is folded, the images hold kHeadFoldRows rows - on the 8 x 64 blocks (the
// head's rows are 512 or 1 024 bins wide and a plan's frame count is a multiple of 32: no other geometry reaches it); the two
// k-step waves of the kernel take half of the shortcut's channels each, in groups of four k-steps
inline bool lass_wino4_headfold_shape(const ConvShape& s) {
    return s.head && lass_wino4_block_tc(s.H, s.W) == 16 && lass_wino4_shape(CONV2_SHORTCUT, s) && s.Cin2 % 32 == 0;
}

// ... with V from memory: conv1 and the identity conv2 (whole or split-K), the kinds without a fused shortcut phase or output
// head; the V image of one (clip, block) is addressed through a 32-bit buffer descriptor
inline bool lass_wino4_vpre_shape(ConvKind kind, const ConvShape& s, int splits = 1) {
    return (kind == CONV1_ACT || kind == CONV2_IDENT) && lass_wino4_shape(kind, s, splits) && !s.head &&
           (unsigned long long)(s.Cin / kWino4KC) * kWino4VFloats * 4ull < 0xFFFF0000ull;
}
// floats of that image: v[clip][block][chunk = cin / 8][36][256]
inline size_t lass_wino4_vpre_floats(int B, int Cin, int H, int W) { return (size_t)B * Cin * (size_t)(H * W / 16) * kWino4NXI; }

// wino4_gemm.hip, F(4x4,3x3) as scatter - 36 batched GEMMs - gather: the V-from-memory kinds, unsplit, with the split-bf16 GEMM's
// tile (128 couts; K = Cin in pairs of 16-row chunks).  The tiles of all clips of a launch are the GEMM's one column index p.
inline bool lass_wino4_gemm_shape(ConvKind kind, const ConvShape& s) {
    return lass_wino4_vpre_shape(kind, s, 1) && s.N == s.Nw && s.N % kPwGemmNB == 0 && s.Cin % (2 * kPwGemmKC) == 0;
}
// floats of its product image m[36][cout][p]: 2.25 x the output
inline size_t lass_wino4_gemm_m_floats(int B, int N, int H, int W) { return (size_t)B * N * (size_t)(H * W / 16) * kWino4NXI; }

// pw_gemm.hip: the 128-cout x 128-pixel tile of both kinds, and the 1x1 shortcut (K = Cin2 in pairs of chunks)
inline bool lass_pw_gemm_tile_shape(const ConvShape& s) {
    const long P = (long)s.H * s.W;
    return P > 0 && P % 4 == 0 && s.N > 0 && s.N % kPwGemmNB == 0 && s.N <= s.Nw && s.Nw % 4 == 0;
}
inline bool lass_pw_gemm_shortcut_shape(const ConvShape& s) {
    return lass_pw_gemm_tile_shape(s) && s.Cin2 > 0 && s.Cin2 % (2 * kPwGemmKC) == 0;
}
// ... and the kernel == stride transposed conv (up_h x 2; K = Cin in pairs of chunks)
inline bool lass_pw_gemm_tconv_shape(const ConvShape& s, int up_h) {
    return lass_pw_gemm_tile_shape(s) && s.Cin > 0 && s.Cin % (2 * kPwGemmKC) == 0 && (up_h == 1 || up_h == 2) && s.N % (2 * up_h) == 0;
}

// conv_bf16.hip: 8 or 16 bins, or a multiple of 32; K in 16-channel chunks, 32-cout wave tiles
inline bool lass_bf16_shape(int Cin, int N, int W) { return (W == 8 || W == 16 || (W % 32) == 0) && Cin % 16 == 0 && N % 32 == 0; }

// conv_bf16_fused.hip addresses one clip's blocked tensors (8-channel octets of bf16) through byte offsets below 2^28
inline bool lass_bf16_fused_addressable(int H, int W) { return (unsigned long long)H * W * 8ull < 0x10000000ull; }
// ... encoder_block1 as one kernel: p = conv1 (CONV1_ACT_PRE), q = conv2 (CONV2_IDENT_PRE; q.pool: an f32 pooled output, which
// the kernel does not write); pool_copies: the pooled output as the two blocked copies instead
inline bool lass_enc1_fused_bf16_shape(const ConvShape& p, const ConvShape& q, bool pool_copies) {
    return p.Cin == 32 && p.N == 32 && p.Nw == 32 && q.Cin == 32 && q.N == 32 && q.Nw == 32 && p.W % kBf16FusedTileW == 0 &&
           p.W >= kBf16FusedTileW && !q.pool && (!pool_copies || (q.pool_h == 2 && q.H % 2 == 0)) && q.H == p.H && q.W == p.W;
}
// ... decoder_block6 with the output head: conv1 64 -> 32, conv2 + the 1x1 shortcut over 64 channels
inline bool lass_dec6_fused_bf16_shape(const ConvShape& p, const ConvShape& q) {
    return p.Cin == 64 && p.N == 32 && p.Nw == 32 && q.Cin == 32 && q.N == 32 && q.Nw == 32 && q.Cin2 == 64 &&
           p.W % kBf16FusedTileW == 0 && p.W >= kBf16FusedTileW && q.head && !q.pool && q.H == p.H && q.W == p.W &&
           lass_bf16_fused_addressable(p.H, p.W);
}
// ... with its 2 x 2 transposed conv inside: u_cin channels at u_h x u_w
inline bool lass_dec6u_fused_bf16_shape(const ConvShape& p, const ConvShape& q, int u_cin, int u_h, int u_w) {
    return lass_dec6_fused_bf16_shape(p, q) && u_cin == 64 && u_h * 2 == p.H && u_w * 2 == p.W && p.H % 2 == 0 &&
           lass_bf16_fused_addressable(u_h, u_w);
}

// ---- the route of a block ----------------------------------------------------------------------------------------------------
// f32, the 3x3 convs of a block whose images tile only into 32-row x 16-column F(4x4,3x3) blocks (lass_wino4_narrow: the 16-bin
// level under a 32-multiple of frames): a clip plane is ONE block, so a launch has B * cout / 32 workgroups for the 512 slots
// (256 CUs x 2) - 96 per half-batch branch of the replayed B = 16 graph.  The input-channel loop is dealt to 4 workgroups each
// (48-96 chunks -> 12-24).  The factor is a constant of the route and NOT a function of B: the summation order of a clip must not
// depend on the batch it arrives in (half-batches, ragged tails and single clips are bit-identical - the suite pins that).
constexpr int kWino4Splits = 4;

// f32: the shortcut layers with at least this many input channels run their 1x1 conv in pw_gemm.hip.  Shallower ones (K = 32 ...
// 128: encoder_block2-4, decoder_block5-6) are byte-bound there - writing bias + Wsc x and reading it back costs more than
// the re-fetches it saves (measured, profiles/r06)
constexpr int kShortcutGemmMinCin = 256;

// f32, F(4x4,3x3): the Cout / 32 workgroups of a 32-tile block each form the same transformed input V per chunk (prologue, zero
// padding, 6x6 transform: 252 of a wave's ~460 non-MFMA instructions per chunk, on the datapath the f32 MFMA shares).  Layers with
// at least this many cout groups have one prep launch write V to memory (2.25 x the input) and their conv kernels copy it in by
// LDS-DMA like the weight slab.  Shape only, never a function of B.  The constant is the per-launch table of
// profiles/r09/README.md (B = 16, prep + conv against the launch that transforms its own input): the 12-group layers (Cout 384,
// the 64 x 32 and 32 x 16 levels) are 11-24 % below it; the 8-group layers (Cout 256, 128 x 64) only 1.5-5 % for a 0.6-GB image
// and stay off; with 4 groups or fewer the prep launch costs more than it saves (+ 20-44 %).
constexpr int kVprepMinCoutGroups = 12;

// f32: transposed convs with at least this many input channels run in pw_gemm.hip; decoder_block6's (K = 64, 1 GB of output
// per batch) is byte-bound and measured 7 % faster in the direct kernel
constexpr int kTconvGemmMinCin = 128;

// Which weight matrices lass_finalize also keeps as the three bf16 pieces of pw_gemm.hip's split kernel (6 K N bytes each): every
// one that plan_block / plan_upconv can send there at some image size (the channel half of their rules).  Kept whatever
// RouteCfg::pw_split says at that moment: the switch can be thrown afterwards (weight_plan.h reads no such switch, and
// tests/test_weight_plan_cpu.py holds every route of every switch setting inside the list it makes).
inline bool lass_pw_split_shortcut_weights(bool f32, int cin, int cout) {
    return f32 && cin != cout && cin >= kShortcutGemmMinCin && cin % (2 * kPwGemmKC) == 0 && cout % kPwGemmNB == 0;
}
inline bool lass_pw_split_tconv_weights(bool f32, int cin, int N, int up_h) {
    return f32 && cin >= kTconvGemmMinCin && cin % (2 * kPwGemmKC) == 0 && N % kPwGemmNB == 0 && (up_h == 1 || up_h == 2) && N % (2 * up_h) == 0;
}

enum ComputeMode { MODE_F32 = 0, MODE_BF16 = 1, MODE_BF16X3 = 2 };  // the values of LASS_COMPUTE_* (include/lass_hip.h)

struct RouteCfg {
    ComputeMode mode = MODE_F32;  // the bf16 modes prepare no Winograd weights: a block their kernels refuse runs the direct f32 kernels
    bool f32() const { return mode == MODE_F32; }
    int wino4_mincin = 32; // 3x3 convs with at least that many input channels run as F(4x4,3x3); 0 = off (F(2x2,3x3) everywhere)
    int ksplit_force = 0;  // 0 = kWino4Splits on the 32 x 16 blocks, else 1 / 2 / 4
    int vprep_mode = 1;    // V from memory: 0 = off, 1 = the layers of kVprepMinCoutGroups, 2 = every layer whose kind admits it
    bool head_fold = true; // the fused output head runs on weights composed with after_conv (3 logits instead of 32 channels)
    bool head_sc_fold = true;  // ... and takes its shortcut's logits as planes from the launches that produce its inputs
    bool wino4_gemm = true;  // the 384-cout F(4x4,3x3) convs with V from memory contract as 36 batched split-bf16 GEMMs (wino4_gemm.hip)
    bool pw_split = true;  // the pw_gemm.hip launches contract on the bf16 MFMA over three exact bf16 pieces per operand (f32 accuracy)
    // bf16 mode (MODE_BF16 only: the hi+lo split of bf16x3 has no blocked hand-overs and no fused kernels)
    bool fuse_catb = true;   // tensors between launches travel as blocked bf16 copies (LASS_FUSE_CATB)
    bool fuse_block = true;  // encoder_block1 and decoder_block6 as one kernel each (LASS_FUSE_BLOCK)
    bool fuse_up = true;     // decoder_block6's transposed conv inside that kernel (LASS_FUSE_UP; needs fuse_block)
    bool blocked() const { return mode == MODE_BF16 && fuse_catb; }
};

struct BlockShape {
    int cin, cout;
    int width;  // bins of the level the block runs at: known at finalize, the frame count is not
};

// What a call site adds to the shape
struct BlockIO {
    bool x0 = false;         // encoder_block1: the input is pre_conv(x0), formed on the fly (the *_PRE kinds)
    bool head = false;       // decoder_block6: the output head in conv2's epilogue
    bool pool = false;       // fused avg-pool in conv2's epilogue, pool_h x 2
    int pool_h = 2;
    bool x_aligned = true;   // the block input meets pw_gemm.hip's 16-byte alignment (pointer, and batch stride % 4 floats)
    bool sc_planes = false;  // encoder_block1 / decoder_block6 of one lass_separate: the call site hands over (takes) the head's
                             // shortcut logits as planes - plan_head_sc_fold below has decided that for both ends at once
    // bf16 mode, lass_separate only (plan_separate below decides them for producer and consumer at once): tensors the call site
    // hands over as blocked bf16 copies instead of f32
    bool cat_in = false;       // the input: two copies, one with conv1's prologue applied, one raw for the 1x1 shortcut
    bool skip_out = false;     // an encoder's skip output: the same two copies inside the decoder's concat
    bool pool_copies = false;  // the pooled output: the two copies that are the next encoder's cat_in
    bool act_out = false;      // a decoder's output: ONE copy with the next transposed conv's prologue applied
    int up_cin = 0;            // decoder_block6: the call site has NOT run the 2 x 2 transposed conv in front (up_cin channels at
                               // H/2 x W/2) - only the kernel that contains it will do; 0: it has
};

// Which of a block's F(4x4,3x3) weight images lass_finalize prepares: u1f (conv1) / u2f (conv2).  conv1 at every level that can
// tile; conv2 of the blocks with a 1x1 shortcut and of encoder_block1 (32 -> 32, residual = pre_conv(x0)); at the 16-bin level
// both convs of every block (the 32 x 16 blocks run them identity residual or not: + 106 MB of images for encoder_block6 and
// decoder_block1).  The 8-bin level tiles into no F(4x4,3x3) block and gets none.
struct Wino4Images {
    bool u1f = false, u2f = false;
};
inline Wino4Images wino4_images(const RouteCfg& cfg, int cin, int cout, int width) {
    Wino4Images im;
    const int m = cfg.wino4_mincin;
    if (!cfg.f32() || m <= 0 || cin % 8 != 0 || cout % 32 != 0) return im;
    const bool level = width % 32 == 0, narrow = width % 32 == 16;
    im.u1f = (level || narrow) && cin >= m;
    im.u2f = cout >= m && (level ? cin != cout || cout == kPreCh : narrow && cin >= m);
    return im;
}

enum ConvFamily {
    CONV_DIRECT = 0,  // conv.hip
    CONV_F2X2 = 1,    // wino.hip
    CONV_F4X4 = 2,    // wino4.hip
    CONV_NONE = 3     // conv2 behind a shortcut GEMM that no F(4x4,3x3) kernel takes: a state error, nothing is launched
};

struct ConvRoute {
    ConvFamily family = CONV_DIRECT;
    ConvKind kind = CONV1_ACT;
    int splits = 1;               // F(4x4,3x3) split-K factor
    bool v_from_memory = false;   // F(4x4,3x3): a prep launch writes the transformed input, the conv kernel reads it
    bool gemm = false;            // F(4x4,3x3) with V from memory: scatter, 36 batched split-bf16 GEMMs, gather (wino4_gemm.hip) in
                                  // place of the prep, conv (and combine) launches that the fields above describe
    bool head_fold = false;       // F(4x4,3x3), CONV2_SHORTCUT with the output head: the folded kernel and its composed images
    bool head_sc_fold = false;    // F(4x4,3x3) on 8 x 64 blocks: the folded head without its shortcut phase (it reads two sets of
                                  // logit planes), or CONV2_IDENT_PRE that writes the skip's set from its epilogue
};

struct BlockRoute {
    ConvRoute conv1, conv2;
    bool shortcut_gemm = false;  // the 1x1 shortcut is a pw_gemm.hip launch in front, into the block's output slot; conv2 is then
                                 // CONV2_IDENT with that slot as its residual, in place
    bool pw_split = false;       // ... by pw_gemm.hip's split-bf16 kernel (RouteCfg::pw_split: the switch picks the kernel, never the route)
    size_t kpart_floats = 0;     // split-K partials both convs share: [splits][B][cout][H][W]
    size_t v_floats = 0;         // the V slot: the larger of the two convs' images (one at a time, in stream order)
    size_t m_floats = 0;         // the M slot of the gemm route: the product image [36][cout][tiles of the batch], one conv at a time
};

// f32, F(4x4,3x3) with V from memory and at least kVprepMinCoutGroups cout groups (Cout 384: both convs of encoder_block5-6 and
// decoder_block1-2): the conv kernel there is 36 independent contractions M_xi = U_xi V_xi and an output transform, on the f32
// MFMA with a 16 x 16 wave tile that re-reads both operands from LDS per 16 MACs.  As GEMMs of their own they take pw_gemm.hip's
// split-bf16 body (128 x 128 tile, three exact bf16 pieces per operand, f32 accuracy).  Shape and switches only, never a
// function of B: a column's sum over K does not depend on the tile or the batch it sits in.
inline bool lass_wino4_gemm_routed(const RouteCfg& cfg, const ConvRoute& c, const ConvShape& s) {
    return cfg.f32() && cfg.wino4_gemm && cfg.ksplit_force == 0 && c.family == CONV_F4X4 && c.v_from_memory &&
           (c.kind == CONV1_ACT || c.kind == CONV2_IDENT) && s.N / 32 >= kVprepMinCoutGroups && s.Cin % 32 == 0 &&
           lass_wino4_gemm_shape(c.kind, s);
}
// ... and which convs lass_finalize keeps the split images of: the channel half of that rule, whatever the switch says then
inline bool lass_wino4_gemm_weights(bool f32, int cin, int cout) {
    return f32 && cout % kPwGemmNB == 0 && cout / 32 >= kVprepMinCoutGroups && cin % 32 == 0;
}

inline BlockRoute plan_block(const RouteCfg& cfg, const BlockShape& b, int B, int H, int W, const BlockIO& io) {
    BlockRoute r;
    const bool ident = b.cin == b.cout;
    r.conv1.kind = io.x0 ? CONV1_ACT_PRE : CONV1_ACT;  // (the direct kernels have no *_PRE kinds: they refuse them)
    r.conv2.kind = !ident ? CONV2_SHORTCUT : io.x0 ? CONV2_IDENT_PRE : CONV2_IDENT;
    if (!cfg.f32()) return r;
    ConvShape s1, s2;
    s1.Cin = b.cin; s1.N = s1.Nw = b.cout; s1.H = H; s1.W = W;
    s2.Cin = s2.N = s2.Nw = b.cout; s2.H = H; s2.W = W;
    s2.Cin2 = ident ? 0 : b.cin; s2.pool = io.pool; s2.pool_h = io.pool_h; s2.head = io.head;
    const Wino4Images im = wino4_images(cfg, b.cin, b.cout, b.width);
    const int m = cfg.wino4_mincin;
    // split-K: both convs of a 16-bin block on 32 x 16 images; 0 = the block does not take that route (never the x0 block)
    int ksplit = 0;
    if (!io.x0 && m > 0 && lass_wino4_narrow(H, W) && b.width % 32 == 16 && b.cin >= m && b.cout >= m && b.cin % 8 == 0 && b.cout % 32 == 0)
        ksplit = cfg.ksplit_force ? cfg.ksplit_force : kWino4Splits;
    const int n = ksplit > 1 ? ksplit : 1;
    // the weight images of a 16-bin level serve the 32 x 16 blocks only, those of the wider levels the wider blocks only
    const bool geom = b.width % 32 == 0 ? !lass_wino4_narrow(H, W) : ksplit > 0;
    const bool vprep = !io.x0 && geom && m > 0 && (cfg.vprep_mode == 2 || (cfg.vprep_mode == 1 && b.cout / 32 >= kVprepMinCoutGroups));
    // the F(4x4,3x3) routes are taken from the F(2x2,3x3) one: only where that shape test holds too
    const bool wino1 = lass_wino_shape(s1), wino2 = lass_wino_shape(s2);
    const auto f4 = [&](ConvRoute& c, ConvKind kind, const ConvShape& s, int splits) {
        c.family = CONV_F4X4; c.kind = kind; c.splits = splits;
        c.v_from_memory = vprep && lass_wino4_vpre_shape(kind, s, splits);
    };
    if (wino1 && im.u1f && geom && lass_wino4_shape(r.conv1.kind, s1, n))
        f4(r.conv1, r.conv1.kind, s1, n);
    else
        r.conv1.family = wino1 ? CONV_F2X2 : CONV_DIRECT;
    // The deep shortcut layers (encoder_block5, decoder_block2-4): the 1x1 shortcut as a GEMM of its own with a 128-cout tile.
    // Fused into conv2's 32-cout workgroups instead, every one of the Cout / 32 workgroups of a tile fetches the whole block input
    // again.  The other shortcut layers (and decoder_block6's output head) keep the fused phase.  The 32 x 16 blocks have no fused
    // shortcut phase at all - it would be serial work behind a split-K sum (decoder_block1) - and without the GEMM fall to F(2x2,3x3).
    const bool u2f = im.u2f && geom;
    r.shortcut_gemm = !ident && !io.head && b.cin >= kShortcutGemmMinCin && wino2 && u2f &&
                      (ksplit > 0 || lass_wino4_shape(CONV2_SHORTCUT, s2)) && lass_pw_gemm_shortcut_shape(s2) && io.x_aligned;
    r.pw_split = r.shortcut_gemm && cfg.pw_split;
    if (r.shortcut_gemm) {
        s2.Cin2 = 0;
        if (lass_wino4_shape(CONV2_IDENT, s2, n))
            f4(r.conv2, CONV2_IDENT, s2, n);
        else
            r.conv2 = ConvRoute{CONV_NONE, CONV2_IDENT};
    } else if (wino2 && u2f && (ident ? (io.x0 || ksplit > 0) && lass_wino4_shape(r.conv2.kind, s2, n)
                                      : lass_wino4_shape(CONV2_SHORTCUT, s2))) {
        // (identity: encoder_block1, and encoder_block6 with its 1 x 2 pool; the fused shortcut phase is never split)
        f4(r.conv2, r.conv2.kind, s2, ident ? n : 1);
        r.conv2.head_fold = cfg.head_fold && !ident && io.head && lass_wino4_headfold_shape(s2);
        r.conv2.head_sc_fold = io.sc_planes && cfg.head_fold && cfg.head_sc_fold && lass_wino4_block_tc(H, W) == 16 &&
                               (r.conv2.head_fold || (io.x0 && r.conv2.kind == CONV2_IDENT_PRE));
    } else {
        r.conv2.family = wino2 ? CONV_F2X2 : CONV_DIRECT;
    }
    if (r.conv1.splits > 1 || r.conv2.splits > 1) r.kpart_floats = (size_t)n * B * b.cout * H * W;
    if (r.conv1.v_from_memory) r.v_floats = lass_wino4_vpre_floats(B, b.cin, H, W);
    if (r.conv2.v_from_memory && lass_wino4_vpre_floats(B, b.cout, H, W) > r.v_floats) r.v_floats = lass_wino4_vpre_floats(B, b.cout, H, W);
    // The gemm route replaces the launches of a V-from-memory conv; every field above stays what the switch falls back to.  A
    // forced split factor asks for the split-K kernels and keeps them.
    r.conv1.gemm = lass_wino4_gemm_routed(cfg, r.conv1, s1);
    r.conv2.gemm = lass_wino4_gemm_routed(cfg, r.conv2, s2);
    if (r.conv1.gemm || r.conv2.gemm) r.m_floats = lass_wino4_gemm_m_floats(B, b.cout, H, W);
    return r;
}

// ---- the head's shortcut logits at their producers ------------------------------------------------------------------------------
// The folded head reads decoder_block6's concat only to apply the composed 1x1 shortcut Wsc' (head_fold.h).  Both halves of that
// concat are in registers, or in a staged tile, in the launch that produces them: the skip x1 in encoder_block1.conv2's epilogue,
// and up = Wt act(x11) as 12 more columns (3 logits x 4 sub-pixels) of the transposed conv's GEMM.  With both formed there the head
// reads conv1's output and two sets of logit planes, and runs no shortcut phase.  One decision for three launches of one
// lass_separate; the stage calls never take it.

// conv.hip's transposed conv with the extra cout block: 2 x 2, K = cin in 16-channel chunks, 64-cout x 32-pixel wave tiles, below
// the input-channel count from which transposed convs run in pw_gemm.hip
inline bool lass_tconv_logits_shape(int cin, int cout, int up_h, int up_w, int h, int w) {
    return up_h == 2 && up_w == 2 && cin > 0 && cin % 32 == 0 && cin < kTconvGemmMinCin && cout > 0 && (4 * cout) % 64 == 0 && h > 0 &&
           w > 0 && w % 32 == 0;
}

struct HeadScSite {
    int windows = 0;     // 0: ResUNet30; n: the multi-STFT model with n analysis windows - its skip is the concat of n branches, each
                         // from a launch of its own, and it keeps its launches as they are for every n (n = 1 included)
    int tconv_cin = 0;   // decoder_block6's transposed conv
    int up_h = 0, up_w = 0;
};

// enc1 / dec6: encoder_block1 and decoder_block6 with what lass_separate fuses into them, B, H, W: decoder_block6's image
inline bool plan_head_sc_fold(const RouteCfg& cfg, const BlockShape& enc1, BlockIO enc1_io, const BlockShape& dec6, BlockIO dec6_io,
                              const HeadScSite& site, int B, int H, int W) {
    if (!cfg.f32() || !cfg.head_fold || !cfg.head_sc_fold || site.windows != 0) return false;
    if (enc1.cout != kPreCh || dec6.cin != dec6.cout + enc1.cout) return false;  // cat = (up, skip): api.hip's concat order
    if (!lass_tconv_logits_shape(site.tconv_cin, dec6.cout, site.up_h, site.up_w, H / 2, W / 2)) return false;
    enc1_io.sc_planes = dec6_io.sc_planes = true;
    return plan_block(cfg, enc1, B, H, W, enc1_io).conv2.head_sc_fold && plan_block(cfg, dec6, B, H, W, dec6_io).conv2.head_sc_fold;
}

// ---- the model table ------------------------------------------------------------------------------------------------------------
// The default STFT geometry (lass_create).  A context carries its own (workspace_plan.h: Geometry - n_fft, hop, bins), and every
// launch interface of kernels.h takes them as arguments: these four name the default's values, nothing reads them as "the" geometry.
constexpr int LASS_NFFT = 1024;
constexpr int LASS_HOP = 160;
constexpr int LASS_NBINS = 513;
constexpr int LASS_FCROP = 512;
constexpr int LASS_COND = 512;
constexpr int LASS_MAX_STFT_WINDOWS = 4;

struct EncSpec { const char* name; int cin, cout, dh, dw; };  // a ConvBlockRes and the (dh, dw) avg-pool behind it
struct DecSpec { const char* name; int cin, cout, uh, uw; };  // the (uh, uw) transposed conv of a decoder; its ConvBlockRes reads the concat
// ResUNet30 (resunet.py:315-418)
constexpr EncSpec kEnc[7] = {{"encoder_block1", 32, 32, 2, 2},   {"encoder_block2", 32, 64, 2, 2},   {"encoder_block3", 64, 128, 2, 2},
                             {"encoder_block4", 128, 256, 2, 2}, {"encoder_block5", 256, 384, 2, 2}, {"encoder_block6", 384, 384, 1, 2},
                             {"conv_block7a", 384, 384, 1, 1}};
constexpr DecSpec kDec[6] = {{"decoder_block1", 384, 384, 1, 2}, {"decoder_block2", 384, 384, 2, 2}, {"decoder_block3", 384, 256, 2, 2},
                             {"decoder_block4", 256, 128, 2, 2}, {"decoder_block5", 128, 64, 2, 2},  {"decoder_block6", 64, 32, 2, 2}};

struct ModelTable {
    EncSpec E[7];  // E[0] is ONE analysis branch's block (there are nbr of them); E[1].cin = 32 * nbr
    DecSpec D[6];
    int windows = 0;  // 0: ResUNet30; n: the multi-STFT model with n analysis windows
    int nbr = 1;      // analysis branches
    int fcrop = 512;  // bins of the full-resolution level
    int dec_cat[6];   // concat channels of decoder d = D[d].cout + its skip's channels: torch.cat((x, skip), 1)
    BlockShape enc_shape(int i) const { return BlockShape{E[i].cin, E[i].cout, fcrop >> i}; }  // behind i frequency halvings
    BlockShape dec_shape(int d) const { return BlockShape{dec_cat[d], D[d].cout, fcrop >> (5 - d)}; }  // at its skip's level
};
// fcrop: n_fft / 2 of the context's STFT geometry - 512 (n_fft 1024) or 1024 (n_fft 2048: ResUNet30 at 32 kHz, and every multi-STFT model)
inline ModelTable model_table(int windows, int fcrop) {
    ModelTable m;
    for (int i = 0; i < 7; ++i) m.E[i] = kEnc[i];
    for (int d = 0; d < 6; ++d) m.D[d] = kDec[d];
    m.windows = windows;
    m.nbr = windows ? windows : 1;
    m.fcrop = fcrop;
    m.E[1].cin = kPreCh * m.nbr;  // the branches' pools, channel-concatenated
    for (int d = 0; d < 6; ++d) m.dec_cat[d] = m.D[d].cout + m.E[5 - d].cout * (d == 5 ? m.nbr : 1);
    return m;
}

// The image of encoder level i at t_pad padded frames; decoder d runs at level 5 - d, its transposed conv reads (eh / uh, ew / uw)
struct Levels {
    int eh[7], ew[7];
};
inline Levels model_levels(const ModelTable& m, int t_pad) {
    Levels lv;
    int h = t_pad, w = m.fcrop;
    for (int i = 0; i < 7; ++i) {
        lv.eh[i] = h; lv.ew[i] = w;
        h /= m.E[i].dh; w /= m.E[i].dw;
    }
    return lv;
}

// ---- the bf16 modes: weights, transposed convs, blocks --------------------------------------------------------------------------
// Which bf16 copies lass_finalize prepares (weight_plan.h: plan_weights).  The plans below ask these functions, not the pointers:
// finalize allocates by exactly this rule or fails.
struct Bf16Weights {
    bool pair = false, pair_lo = false;          // conv1 and conv2 (hi), and their lo halves (bf16x3)
    bool shortcut = false, shortcut_lo = false;  // the 1x1 shortcut of a block that has one
};
inline Bf16Weights bf16_block_weights(const RouteCfg& cfg, int cin, int cout) {
    Bf16Weights wt;
    wt.pair = !cfg.f32() && cin % 16 == 0 && cout % 16 == 0;
    wt.pair_lo = wt.pair && cfg.mode == MODE_BF16X3;
    wt.shortcut = cin != cout && wt.pair;
    wt.shortcut_lo = wt.shortcut && cfg.mode == MODE_BF16X3;
    return wt;
}
// a decoder's transposed conv (hi; the lo half in bf16x3)
inline bool bf16_tconv_weights(const RouteCfg& cfg, const DecSpec& d) { return !cfg.f32() && d.cin % 16 == 0; }
// decoder_block6's 1x1 shortcut over the up-sampled half of its concat, composed with its transposed conv (dec6u_fused_bf16_kernel)
inline bool bf16_up_sc_weights(const RouteCfg& cfg, const ModelTable& m) {
    const DecSpec& d = m.D[5];
    const BlockShape rb = m.dec_shape(5);
    return cfg.mode == MODE_BF16 && m.windows == 0 && d.cin == 64 && d.cout == 32 && d.uh == 2 && d.uw == 2 && rb.cin == 64 &&
           rb.cout == 32 && bf16_tconv_weights(cfg, d);
}

// The transposed conv of a decoder, every mode: h x w is its input image
enum UpFamily {
    UP_DIRECT = 0,  // conv.hip
    UP_GEMM = 1,    // pw_gemm.hip (f32)
    UP_BF16 = 2,    // conv_bf16.hip
    UP_LOGITS = 3,  // tconv_logits.hip: f32, with the head's shortcut logits as one more cout block (plan_head_sc_fold)
    UP_INSIDE = 4   // no launch: decoder_block6's fused bf16 kernel contains it (BF16_DEC6U)
};
struct UpSite {
    bool in_act = false;      // bf16: the input arrives as ONE blocked copy with this conv's prologue applied (the producer's act_out)
    bool out_copies = false;  // bf16: the output goes out as the concat's two blocked copies (the block's cat_in)
    bool logits = false;      // f32: the call site takes the head's shortcut logits from this launch
    bool aligned = true;      // input, weights and output meet pw_gemm.hip's alignment
};
struct UpRoute {
    UpFamily family = UP_DIRECT;
    bool in_act = false, out_copies = false;  // the site's, where the family admits them
    bool pw_split = false;                    // UP_GEMM: pw_gemm.hip's split-bf16 kernel (RouteCfg::pw_split)
};
inline UpRoute plan_upconv(const RouteCfg& cfg, const DecSpec& d, int h, int w, const UpSite& site = UpSite()) {
    UpRoute r;
    ConvShape s;
    s.Cin = d.cin; s.N = s.Nw = d.cout * d.uh * d.uw; s.H = h; s.W = w;
    if (site.logits && cfg.f32() && lass_tconv_logits_shape(d.cin, d.cout, d.uh, d.uw, h, w)) {
        r.family = UP_LOGITS;
    } else if (!cfg.f32() && bf16_tconv_weights(cfg, d) && lass_bf16_shape(s.Cin, s.N, w)) {
        r.family = UP_BF16;
        // (the blocked copies are written by the 2 x 2 kernels only)
        r.in_act = site.in_act && cfg.blocked();
        r.out_copies = site.out_copies && cfg.blocked() && d.uh == 2 && d.uw == 2;
    } else if (cfg.f32() && d.cin >= kTconvGemmMinCin && site.aligned && lass_pw_gemm_tconv_shape(s, d.uh)) {
        r.family = UP_GEMM;  // K = cin, N = 4 cout: one GEMM, the prologue applied once per element
        r.pw_split = cfg.pw_split;
    }
    return r;
}

// One block in the bf16 modes
enum Bf16Form {
    BF16_NONE = 0,  // the bf16 kernels do not take the block (or the mode is f32): plan_block's route, f32 hand-overs
    BF16_TWO = 1,   // conv1 and conv2 as two launches of conv_bf16.hip, the intermediate as blocked bf16
    BF16_ENC1 = 2,  // conv_bf16_fused.hip: encoder_block1 as one kernel, the intermediate in LDS
    BF16_DEC6 = 3,  // ... decoder_block6 with the output head
    BF16_DEC6U = 4  // ... and with its transposed conv inside
};
struct Bf16Block {
    Bf16Form form = BF16_NONE;
    bool cat_in = false, skip_out = false, pool_copies = false, act_out = false;  // BlockIO's, where the block admits them
    int launches() const { return form == BF16_NONE || form == BF16_TWO ? 2 : 1; }
};
// both convs of a block run the bf16 kernels (they share shape and mode), or neither
inline bool bf16_block_runs(const RouteCfg& cfg, const BlockShape& b, int W, bool x0) {
    const Bf16Weights wt = bf16_block_weights(cfg, b.cin, b.cout);
    return wt.pair && lass_bf16_shape(b.cin, b.cout, W) && (!x0 || W % 32 == 0) && (b.cin == b.cout || wt.shortcut);
}
inline Bf16Block plan_bf16_block(const RouteCfg& cfg, const BlockShape& b, int H, int W, const BlockIO& io) {
    Bf16Block r;
    if (!bf16_block_runs(cfg, b, W, io.x0)) return r;
    r.form = BF16_TWO;
    if (cfg.blocked()) {
        r.cat_in = io.cat_in; r.skip_out = io.skip_out; r.act_out = io.act_out;
        r.pool_copies = io.pool_copies && io.pool && io.pool_h == 2;  // written by the fused 2 x 2 pool only
    }
    if (cfg.mode != MODE_BF16 || !cfg.fuse_block) return r;
    const bool ident = b.cin == b.cout;
    ConvShape p, q;
    p.Cin = b.cin; p.N = p.Nw = b.cout; p.H = H; p.W = W;
    q.Cin = q.N = q.Nw = b.cout; q.H = H; q.W = W;
    q.Cin2 = ident ? 0 : b.cin; q.pool = io.pool && !r.pool_copies; q.pool_h = io.pool_h; q.head = io.head;
    if (io.x0) {  // in the blocked-copy pipeline only: the kernel writes its output as the skip's two copies
        if (r.skip_out && ident && lass_enc1_fused_bf16_shape(p, q, r.pool_copies)) r.form = BF16_ENC1;
    } else if (r.cat_in && io.head && !ident && W == b.width) {  // conv1 from the activated copy, the shortcut from the raw one
        if (io.up_cin) {
            if (lass_dec6u_fused_bf16_shape(p, q, io.up_cin, H / 2, W / 2)) r.form = BF16_DEC6U;
        } else if (lass_dec6_fused_bf16_shape(p, q)) {
            r.form = BF16_DEC6;
        }
    }
    return r;
}

// One lass_separate, the ONE walk over its blocks: the BlockIO every block is called with, every block's form and every hand-over
// between two launches, decided for producer and consumer at once - a consumer that read f32 storage as bf16 units, or the reverse,
// would read garbage - the head_sc_fold decision for its three launches, and in f32 every block's route with the workspace the
// routes take.  enc[0] stands for all nbr branch blocks.  The stage calls (lass_convblock, lass_encoder_block, lass_upconv) have no
// hand-overs: plan_block, plan_bf16_block and plan_upconv on a default-constructed site.
struct SeparatePlan {
    BlockIO enc_io[7], dec_io[6];  // complete: the bf16 hand-overs are the ones the block admits; inputs are workspace tensors (x_aligned)
    Bf16Block enc[7], dec[6];
    UpRoute up[6];
    bool head_sc_fold = false;     // plan_head_sc_fold's decision: enc_io[0].sc_planes, dec_io[5].sc_planes and up[5] = UP_LOGITS
    BlockRoute enc_rt[7], dec_rt[6];  // f32: plan_block at the call's B (the bf16 modes: the kinds alone)
    size_t kpart_floats = 0, v_floats = 0, m_floats = 0;  // ... and their largest slots over the trunk and decoder blocks
    // P_CONV3X3 / P_TCONV profiler scopes of the run: one per launch (f32: the prep launch of a V image shares its conv's)
    int conv_scopes = 0, tconv_scopes = 0;
};
// B sizes the workspace slots of the routes and nothing else: forms, hand-overs, families and scope counts do not depend on it.
// head_sc_weights: lass_finalize composed the head's shortcut with its two producers (head_fold.h) for this checkpoint
// (weight_plan.h: head_sc_weights is the rule, and the images are there).
inline SeparatePlan plan_separate(const RouteCfg& cfg, const ModelTable& m, const Levels& lv, int B, bool head_sc_weights) {
    SeparatePlan sp;
    // encoder_block1 forms pre_conv(x0), the encoders pool in conv2's epilogue, decoder_block6 carries the output head
    for (int i = 0; i < 7; ++i) {
        sp.enc_io[i].x0 = i == 0;
        sp.enc_io[i].pool = i < 6; sp.enc_io[i].pool_h = m.E[i].dh;
    }
    sp.dec_io[5].head = true;
    HeadScSite hs;
    hs.windows = m.windows; hs.tconv_cin = m.D[5].cin; hs.up_h = m.D[5].uh; hs.up_w = m.D[5].uw;
    sp.head_sc_fold = head_sc_weights && m.E[0].dh == 2 && m.E[0].dw == 2 &&
                      plan_head_sc_fold(cfg, m.enc_shape(0), sp.enc_io[0], m.dec_shape(5), sp.dec_io[5], hs, B, lv.eh[0], lv.ew[0]);
    sp.enc_io[0].sc_planes = sp.dec_io[5].sc_planes = sp.head_sc_fold;
    const auto enc_runs = [&](int i) { return bf16_block_runs(cfg, m.enc_shape(i), lv.ew[i], i == 0); };
    const auto dec_runs = [&](int d) { return bf16_block_runs(cfg, m.dec_shape(d), lv.ew[5 - d], false); };
    const auto has_sc = [&](const BlockShape& b) { return b.cin != b.cout; };
    const auto up = [&](int d, bool in_act, bool out_copies) {
        UpSite site;
        site.in_act = in_act; site.out_copies = out_copies; site.logits = d == 5 && sp.head_sc_fold;
        return plan_upconv(cfg, m.D[d], lv.eh[5 - d] / m.D[d].uh, lv.ew[5 - d] / m.D[d].uw, site);
    };
    // the hand-overs a block admits, back into the BlockIO it is called with
    const auto admit = [](BlockIO& io, const Bf16Block& b, int up_cin) {
        io.cat_in = b.cat_in; io.skip_out = b.skip_out; io.pool_copies = b.pool_copies; io.act_out = b.act_out;
        io.up_cin = b.form == BF16_DEC6U ? up_cin : 0;
    };
    for (int d = 0; d < 6; ++d) sp.up[d] = up(d, false, false);  // the family does not depend on the hand-overs
    // decoders 2-6 (2 x 2 up-sampling) take their concat as the two blocked copies: half from the transposed conv, half from the
    // encoder whose skip it is
    bool cb[6] = {false, false, false, false, false, false};
    for (int d = 1; d < 6; ++d)
        cb[d] = cfg.blocked() && m.D[d].uh == 2 && m.D[d].uw == 2 && dec_runs(d) && has_sc(m.dec_shape(d)) &&
                sp.up[d].family == UP_BF16 && enc_runs(5 - d);
    // ... and encoder blocks 2-5 their input, from the previous block's fused 2 x 2 pool - both blocks are then in the pipeline
    bool pc[4] = {false, false, false, false};
    for (int i = 0; i < 4; ++i)
        pc[i] = cfg.blocked() && m.E[i].dh == 2 && lv.ew[i] % 32 == 0 && cb[5 - i] && cb[4 - i] && has_sc(m.enc_shape(i + 1)) && enc_runs(i + 1);
    for (int i = 0; i < 7; ++i) {
        BlockIO io = sp.enc_io[i];
        io.skip_out = i < 5 && cb[5 - i];
        io.cat_in = i >= 1 && i <= 4 && pc[i - 1];
        io.pool_copies = i < 4 && pc[i];
        sp.enc[i] = plan_bf16_block(cfg, m.enc_shape(i), lv.eh[i], lv.ew[i], io);
        admit(sp.enc_io[i], sp.enc[i], 0);
    }
    for (int d = 0; d < 6; ++d) {
        const int e = 5 - d;
        BlockIO io = sp.dec_io[d];
        io.cat_in = cb[d];
        // the output feeds only the next transposed conv: handed over activated
        io.act_out = d < 5 && cfg.blocked() && dec_runs(d) && has_sc(m.dec_shape(d)) && sp.up[d + 1].family == UP_BF16;
        sp.dec[d] = plan_bf16_block(cfg, m.dec_shape(d), lv.eh[e], lv.ew[e], io);
        // decoder_block6: its transposed conv inside the fused kernel, if the kernel takes the block that way
        if (d == 5 && cfg.fuse_up && cb[d] && sp.dec[4].act_out && bf16_up_sc_weights(cfg, m)) {
            io.up_cin = m.D[d].cin;
            const Bf16Block in = plan_bf16_block(cfg, m.dec_shape(d), lv.eh[e], lv.ew[e], io);
            if (in.form == BF16_DEC6U) {
                sp.dec[d] = in;
                sp.up[d] = UpRoute{UP_INSIDE, true, false};
            }
        }
        admit(sp.dec_io[d], sp.dec[d], m.D[d].cin);
        if (sp.up[d].family != UP_INSIDE) sp.up[d] = up(d, d > 0 && sp.dec[d - 1].act_out, sp.dec[d].cat_in);
    }
    // the routes and the launches they make (f32: the GEMM shortcut is a launch of its own)
    const auto route = [&](BlockRoute& rt, const BlockShape& b, int e, const BlockIO& io, const Bf16Block& bf, int times, bool slots) {
        rt = plan_block(cfg, b, B, lv.eh[e], lv.ew[e], io);
        sp.conv_scopes += (cfg.f32() ? 2 + rt.shortcut_gemm : bf.launches()) * times;
        if (!slots) return;
        if (rt.kpart_floats > sp.kpart_floats) sp.kpart_floats = rt.kpart_floats;
        if (rt.v_floats > sp.v_floats) sp.v_floats = rt.v_floats;
        if (rt.m_floats > sp.m_floats) sp.m_floats = rt.m_floats;
    };
    for (int i = 0; i < 7; ++i) route(sp.enc_rt[i], m.enc_shape(i), i, sp.enc_io[i], sp.enc[i], i == 0 ? m.nbr : 1, i > 0);
    for (int d = 0; d < 6; ++d) {
        route(sp.dec_rt[d], m.dec_shape(d), 5 - d, sp.dec_io[d], sp.dec[d], 1, true);
        sp.tconv_scopes += sp.up[d].family != UP_INSIDE;
    }
    return sp;
}
