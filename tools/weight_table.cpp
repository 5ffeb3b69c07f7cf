// weight_table.cpp - the weight images of a model as lass_amd/csrc/weight_plan.h lists them (plan_weights: what lass_finalize
// allocates and fills), and the images the planned launches read (route_images: what run_resblock and run_upconv check).
// Host only: g++ -std=c++17 -I lass_amd/csrc tools/weight_table.cpp -o tools/bin/weight_table
// usage: weight_table MODE WINO4 WINDOWS FCROP Q [T_PAD [switch=value ...]]
//   MODE 0: f32, 1: bf16, 2: bf16x3;  WINO4: the LASS_WINO4 value (32; 0 = no F(4x4,3x3));  Q: rows of after_conv (3)
//   WINDOWS 0: ResUNet30 at FCROP 512 or 1024; 1 ... 4: the multi-STFT model with that many analysis windows (FCROP 1024)
//   T_PAD: padded frames of a lass_separate, or a comma list of them (a `frames <T_PAD>` line precedes each one's images lines)
//   switches: the ones a lass_set_* can throw after lass_finalize (defaults as a context's) -
//   vprep=1 splits=0 head_fold=1 head_sc_fold=1 wino4_gemm=1 pw_split=1 fuse_catb=1 fuse_block=1 fuse_up=1
// item <owner> <slot> <form> <source> <rows>x<cols>x<taps> <elements> <bytes>      one per image, in lass_finalize's order
//   owner: a block (encoder_block1, encoder_block1s.<k>, ..., decoder_block6), up:<decoder> (its transposed conv) or context
//   source: a checkpoint parameter under the owner's prefix, slot:<SLOT> of the same owner, or composed (several parameters)
// images <separate|stage> <block | up:<decoder>> <SLOT,SLOT,...|->      with T_PAD: every block and transposed conv of the plan_separate
//   walk, and the same on the default site of the stage calls (lass_convblock, lass_upconv)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "weight_plan.h"

namespace {

const char* kSlot[kWeightSlots] = {"W1", "W2", "WSC", "U1", "U2", "USC", "U1F", "U2F", "U1G", "U2G", "WSC3", "B1", "B2", "BSC16", "B1L", "B2L",
                                   "BSCL", "U2H", "WSCH", "BH", "UP16", "UP16L", "UP3", "UP_SC", "UP_SC16", "HS_WT", "HS_WSKIP"};
const char* kForm[] = {"relayout", "bf16", "bf16_lo", "bf16_t", "bf16_t_lo", "f2x2", "f2x2_sc", "f4x4", "f4x4_split3", "pw_split3", "up_sc",
                       "head_u4", "head_wsc", "head_bias", "head_sc_wt", "head_sc_wskip"};

std::string block_name(const ModelTable& m, int b) {
    if (b < m.nbr) return m.windows ? "encoder_block1s." + std::to_string(b) : std::string(m.E[0].name);
    return b < m.nbr + 6 ? m.E[b - m.nbr + 1].name : m.D[b - m.nbr - 6].name;
}

void print_images(const char* site, const std::string& name, SlotSet set) {
    std::string s;
    for (int i = 0; i < kWeightSlots; ++i)
        if (set >> i & 1) s += (s.empty() ? "" : ",") + std::string(kSlot[i]);
    printf("images %s %s %s\n", site, name.c_str(), s.empty() ? "-" : s.c_str());
}

// as run_resblock: the bf16 kernels' images where they take the block, else the route's
SlotSet block_images(const RouteCfg& cfg, const BlockShape& b, const Bf16Block& bf, const BlockRoute& rt) {
    return bf.form != BF16_NONE ? route_images(bf, bf16_block_weights(cfg, b.cin, b.cout)) : route_images(rt);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 6) {
        fprintf(stderr, "usage: %s MODE WINO4 WINDOWS FCROP Q [T_PAD [switch=value ...]]\n", argv[0]);
        return 2;
    }
    const int mode = atoi(argv[1]), windows = atoi(argv[3]), fcrop = atoi(argv[4]), Q = atoi(argv[5]);
    if (mode < 0 || mode > 2 || windows < 0 || windows > LASS_MAX_STFT_WINDOWS || (fcrop != 1024 && (fcrop != 512 || windows))) return 2;
    RouteCfg cfg;  // as lass_finalize sees it: the later switches at their defaults
    cfg.mode = (ComputeMode)mode;
    cfg.wino4_mincin = atoi(argv[2]);
    const ModelTable m = model_table(windows, fcrop);
    for (const WeightItem& it : plan_weights(cfg, m, Q)) {
        const std::string owner = it.owner == OWN_BLOCK ? block_name(m, it.index) : it.owner == OWN_DECODER ? std::string("up:") + m.D[it.index].name : "context";
        const std::string source = it.param ? it.param : it.from >= 0 ? std::string("slot:") + kSlot[it.from] : "composed";
        printf("item %s %s %s %s %dx%dx%d %zu %zu\n", owner.c_str(), kSlot[it.slot], kForm[it.form], source.c_str(), it.rows, it.cols, it.taps,
               it.count, it.count * it.elem_bytes);
    }
    if (argc < 7) return 0;
    for (int i = 7; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string k(argv[i], (size_t)(eq - argv[i]));
        const int v = atoi(eq + 1);
        if (k == "vprep") cfg.vprep_mode = v;
        else if (k == "splits") cfg.ksplit_force = v;
        else if (k == "head_fold") cfg.head_fold = v != 0;
        else if (k == "head_sc_fold") cfg.head_sc_fold = v != 0;
        else if (k == "wino4_gemm") cfg.wino4_gemm = v != 0;
        else if (k == "pw_split") cfg.pw_split = v != 0;
        else if (k == "fuse_catb") cfg.fuse_catb = v != 0;
        else if (k == "fuse_block") cfg.fuse_block = v != 0;
        else if (k == "fuse_up") cfg.fuse_up = v != 0;
        else return 2;
    }
    for (char* p = argv[6]; *p; p += *p == ',') {
        const int t_pad = (int)strtol(p, &p, 10);
        if (t_pad <= 0 || t_pad % 32 != 0) return 2;
        printf("frames %d\n", t_pad);
        const Levels lv = model_levels(m, t_pad);
        const SeparatePlan sp = plan_separate(cfg, m, lv, 1, head_sc_weights(cfg, m, Q));
        for (int b = 0; b < model_blocks(m); ++b) {
            const int i = b < m.nbr ? 0 : b - m.nbr + 1;  // encoder index; the decoders follow
            const bool enc = i < 7;
            const int d = i - 7, e = enc ? i : 5 - d;
            const BlockShape s = block_shape(m, b);
            print_images("separate", block_name(m, b), block_images(cfg, s, enc ? sp.enc[i] : sp.dec[d], enc ? sp.enc_rt[i] : sp.dec_rt[d]));
            print_images("stage", block_name(m, b), block_images(cfg, s, plan_bf16_block(cfg, s, lv.eh[e], lv.ew[e], BlockIO()),
                                                                   plan_block(cfg, s, 1, lv.eh[e], lv.ew[e], BlockIO())));
        }
        for (int d = 0; d < 6; ++d) {
            const std::string name = std::string("up:") + m.D[d].name;
            if (sp.up[d].family != UP_INSIDE) print_images("separate", name, route_images(sp.up[d], cfg));  // (inside: no launch, the block's images)
            print_images("stage", name, route_images(plan_upconv(cfg, m.D[d], lv.eh[5 - d] / m.D[d].uh, lv.ew[5 - d] / m.D[d].uw), cfg));
        }
    }
    return 0;
}
