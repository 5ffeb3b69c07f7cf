// route_table.cpp - the f32 conv routes of the model as lass_amd/csrc/conv_route.h decides them, one line per 3x3 conv and one per
// block.  Host only: g++ -std=c++17 -I lass_amd/csrc tools/route_table.cpp -o tools/bin/route_table
// usage: route_table T_PAD [MIN_CIN=32] [VPREP_MODE=1] [FORCED_SPLITS=0] [X_ALIGNED=1] [STFT_WINDOWS=0] [B=1] [HEAD_FOLD=1] [HEAD=1]
//                    [HEAD_SC_FOLD=1]
//   HEAD 1: decoder_block6 as lass_separate runs it, the output head in conv2's epilogue; 0: as the stage call runs it, without
//   HEAD_SC_FOLD: the switch of the head_sc_fold route (plan_head_sc_fold); the route itself needs HEAD = 1 as well
//   STFT_WINDOWS 0: ResUNet30 (512 bins); n > 0: the multi-STFT model with n analysis windows (1024 bins), rows named as
//   lass_amd.arch.ms_conv_layer_table names them (encoder_block1s.<k> for window k).
// conv <name> <direct|f2x2|f4x4|none> <kind> <splits> <v> fold=<0|1> scfold=<0|1>     block <name> shortcut=<gemm|fused|-> kpart=<floats> v=<floats>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "conv_route.h"

namespace {

struct Enc { const char* name; int cin, cout, dh, dw; };
struct Dec { const char* name; int cout, uh, uw; };
const Enc kEnc[7] = {{"encoder_block1", 32, 32, 2, 2},   {"encoder_block2", 32, 64, 2, 2},   {"encoder_block3", 64, 128, 2, 2},
                     {"encoder_block4", 128, 256, 2, 2}, {"encoder_block5", 256, 384, 2, 2}, {"encoder_block6", 384, 384, 1, 2},
                     {"conv_block7a", 384, 384, 1, 1}};
const Dec kDec[6] = {{"decoder_block1", 384, 1, 2}, {"decoder_block2", 384, 2, 2}, {"decoder_block3", 256, 2, 2},
                     {"decoder_block4", 128, 2, 2}, {"decoder_block5", 64, 2, 2},  {"decoder_block6", 32, 2, 2}};
const char* kFamily[] = {"direct", "f2x2", "f4x4", "none"};
const char* kKind[] = {"CONV1_ACT", "CONV2_IDENT", "CONV2_SHORTCUT", "TCONV_ACT", "CONV1_ACT_PRE", "CONV2_IDENT_PRE"};

void print_block(const RouteCfg& cfg, const std::string& name, const BlockShape& b, int B, int H, int W, const BlockIO& io) {
    const BlockRoute r = plan_block(cfg, b, B, H, W, io);
    const ConvRoute* cv[2] = {&r.conv1, &r.conv2};
    for (int k = 0; k < 2; ++k)
        printf("conv %s.conv%d %s %s %d %d fold=%d scfold=%d\n", name.c_str(), k + 1, kFamily[cv[k]->family], kKind[cv[k]->kind],
               cv[k]->splits, (int)cv[k]->v_from_memory, (int)cv[k]->head_fold, (int)cv[k]->head_sc_fold);
    printf("block %s shortcut=%s kpart=%zu v=%zu\n", name.c_str(), b.cin == b.cout ? "-" : r.shortcut_gemm ? "gemm" : "fused",
           r.kpart_floats, r.v_floats);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s T_PAD [MIN_CIN=32] [VPREP_MODE=1] [FORCED_SPLITS=0] [X_ALIGNED=1] [STFT_WINDOWS=0] [B=1] [HEAD_FOLD=1] [HEAD=1] "
                        "[HEAD_SC_FOLD=1]\n", argv[0]);
        return 2;
    }
    const auto arg = [&](int i, int dflt) { return argc > i ? atoi(argv[i]) : dflt; };
    const int t_pad = arg(1, 0), nwin = arg(6, 0), B = arg(7, 1);
    RouteCfg cfg;
    cfg.wino4_mincin = arg(2, 32);
    cfg.vprep_mode = arg(3, 1);
    cfg.ksplit_force = arg(4, 0);
    cfg.head_fold = arg(8, 1) != 0;
    cfg.head_sc_fold = arg(10, 1) != 0;
    const bool head = arg(9, 1) != 0;
    const bool aligned = arg(5, 1) != 0;
    if (t_pad <= 0 || nwin < 0 || nwin > 4 || B <= 0) return 2;
    const int nbr = nwin ? nwin : 1, fcrop = nwin ? 1024 : 512;
    // the image of encoder level i, as the workspace plan walks it
    int eh[7], ew[7], h = t_pad, w = fcrop;
    for (int i = 0; i < 7; ++i) {
        eh[i] = h; ew[i] = w;
        h /= kEnc[i].dh; w /= kEnc[i].dw;
    }
    // the head's shortcut logits at their producers: one decision for encoder_block1 and decoder_block6 of a lass_separate (HEAD = 1)
    bool sc_planes = false;
    if (head) {
        BlockIO eio, dio;
        eio.x0 = true; eio.pool = true; eio.pool_h = kEnc[0].dh; eio.x_aligned = aligned;
        dio.head = true; dio.x_aligned = aligned;
        HeadScSite site;
        site.windows = nwin; site.tconv_cin = kDec[4].cout; site.up_h = kDec[5].uh; site.up_w = kDec[5].uw;
        sc_planes = plan_head_sc_fold(cfg, BlockShape{kEnc[0].cin, kEnc[0].cout, fcrop}, eio,
                                      BlockShape{kDec[5].cout + kEnc[0].cout * nbr, kDec[5].cout, fcrop}, dio, site, B, t_pad, fcrop);
    }
    for (int i = 0; i < 7; ++i)
        for (int k = 0; k < (i == 0 ? nbr : 1); ++k) {
            BlockIO io;
            io.x0 = i == 0;
            io.pool = i < 6; io.pool_h = kEnc[i].dh;
            io.x_aligned = aligned;
            io.sc_planes = i == 0 && sc_planes;
            const int cin = i == 1 ? kPreCh * nbr : kEnc[i].cin;
            const std::string name = i == 0 && nwin ? "encoder_block1s." + std::to_string(k) : kEnc[i].name;
            print_block(cfg, name, BlockShape{cin, kEnc[i].cout, fcrop >> i}, B, eh[i], ew[i], io);
        }
    for (int d = 0; d < 6; ++d) {
        const int e = 5 - d;
        BlockIO io;
        io.head = head && d == 5;
        io.x_aligned = aligned;
        io.sc_planes = d == 5 && sc_planes;
        const int cat = kDec[d].cout + kEnc[e].cout * (e == 0 ? nbr : 1);  // torch.cat((x, skip), 1)
        print_block(cfg, kDec[d].name, BlockShape{cat, kDec[d].cout, fcrop >> e}, B, eh[e], ew[e], io);
    }
    return 0;
}
