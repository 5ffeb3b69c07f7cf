// route_table.cpp - the routes of one lass_separate as lass_amd/csrc/conv_route.h decides them: one line per 3x3 conv and one per
// block (the f32 rule), one per transposed conv, in the bf16 modes one per block (form and hand-overs), and the profiler scopes.
// Host only: g++ -std=c++17 -I lass_amd/csrc tools/route_table.cpp -o tools/bin/route_table
// usage: route_table T_PAD [MIN_CIN=32] [VPREP_MODE=1] [FORCED_SPLITS=0] [X_ALIGNED=1] [STFT_WINDOWS=0] [B=1] [HEAD_FOLD=1] [HEAD=1]
//                    [HEAD_SC_FOLD=1] [MODE=0] [FUSE_CATB=1] [FUSE_BLOCK=1] [FUSE_UP=1] [N_FFT=0] [WINO4_GEMM=1]
//   MODE 0: f32, 1: bf16, 2: bf16x3; FUSE_*: the LASS_FUSE_* switches of the bf16 mode.  With MODE given (any value) the up,
//   bf16 and scopes lines follow the conv and block lines; without it the output is the conv and block lines alone.
//   HEAD 1: decoder_block6 as lass_separate runs it, the output head in conv2's epilogue; 0: as the stage call runs it, without
//   HEAD_SC_FOLD: the switch of the head_sc_fold route (plan_head_sc_fold); the route itself needs HEAD = 1 as well
//   STFT_WINDOWS 0: ResUNet30 (512 bins); n > 0: the multi-STFT model with n analysis windows (1024 bins), rows named as
//   lass_amd.arch.ms_conv_layer_table names them (encoder_block1s.<k> for window k).
//   N_FFT 0: the model's own (1024 for ResUNet30, 2048 for the multi-STFT model); 2048 with STFT_WINDOWS 0: ResUNet30 at the
//   32 kHz geometry (1024 bins).
//   WINO4_GEMM: the switch of the gemm route (wino4_gemm.hip).  With it given (any value) the conv and block lines end in gemm= / m=;
//   the fields in front describe the launches the switch falls back to.  Without it the lines are what they always were.
// conv <name> <direct|f2x2|f4x4|none> <kind> <splits> <v> fold=<0|1> scfold=<0|1> [gemm=<0|1>]     block <name> shortcut=<gemm|fused|-> kpart=<floats> v=<floats> [m=<floats>]
// up <decoder> <direct|gemm|bf16|tconv_logits|inside> in_act=<0|1> out_copies=<0|1>
// bf16 <block> form=<f32|two|enc1|dec6|dec6u> cat_in=<0|1> skip_out=<0|1> pool_copies=<0|1> act_out=<0|1>      (MODE 1, 2)
// scopes conv3x3=<n> tconv=<n>      the P_CONV3X3 / P_TCONV profiler scopes of the run (HEAD = 1: a lass_separate)
#include <cstdio>
#include <cstdlib>
#include <string>

#include "conv_route.h"

namespace {

const char* kFamily[] = {"direct", "f2x2", "f4x4", "none"};
const char* kUpFamily[] = {"direct", "gemm", "bf16", "tconv_logits", "inside"};
const char* kForm[] = {"f32", "two", "enc1", "dec6", "dec6u"};
const char* kKind[] = {"CONV1_ACT", "CONV2_IDENT", "CONV2_SHORTCUT", "TCONV_ACT", "CONV1_ACT_PRE", "CONV2_IDENT_PRE"};

bool g_gemm_cols = false;  // the WINO4_GEMM argument was given: gemm= and m= trail the conv and block lines

void print_block(const std::string& name, const BlockShape& b, const BlockRoute& r) {
    const ConvRoute* cv[2] = {&r.conv1, &r.conv2};
    for (int k = 0; k < 2; ++k) {
        printf("conv %s.conv%d %s %s %d %d fold=%d scfold=%d", name.c_str(), k + 1, kFamily[cv[k]->family], kKind[cv[k]->kind],
               cv[k]->splits, (int)cv[k]->v_from_memory, (int)cv[k]->head_fold, (int)cv[k]->head_sc_fold);
        if (g_gemm_cols) printf(" gemm=%d", (int)cv[k]->gemm);
        printf("\n");
    }
    printf("block %s shortcut=%s kpart=%zu v=%zu", name.c_str(), b.cin == b.cout ? "-" : r.shortcut_gemm ? "gemm" : "fused",
           r.kpart_floats, r.v_floats);
    if (g_gemm_cols) printf(" m=%zu", r.m_floats);
    printf("\n");
}

void print_bf16(const std::string& name, const Bf16Block& b) {
    printf("bf16 %s form=%s cat_in=%d skip_out=%d pool_copies=%d act_out=%d\n", name.c_str(), kForm[b.form], (int)b.cat_in, (int)b.skip_out,
           (int)b.pool_copies, (int)b.act_out);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s T_PAD [MIN_CIN=32] [VPREP_MODE=1] [FORCED_SPLITS=0] [X_ALIGNED=1] [STFT_WINDOWS=0] [B=1] [HEAD_FOLD=1] [HEAD=1] "
                        "[HEAD_SC_FOLD=1] [MODE=0] [FUSE_CATB=1] [FUSE_BLOCK=1] [FUSE_UP=1] [N_FFT=0] [WINO4_GEMM=1]\n", argv[0]);
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
    const int mode = arg(11, 0);
    cfg.fuse_catb = arg(12, 1) != 0;
    cfg.fuse_block = arg(13, 1) != 0;
    cfg.fuse_up = arg(14, 1) != 0;
    cfg.wino4_gemm = arg(16, 1) != 0;
    g_gemm_cols = argc > 16;
    const bool head = arg(9, 1) != 0;
    const bool aligned = arg(5, 1) != 0;
    if (t_pad <= 0 || nwin < 0 || nwin > 4 || B <= 0 || mode < 0 || mode > 2) return 2;
    cfg.mode = (ComputeMode)mode;
    const int n_fft = arg(15, 0) ? arg(15, 0) : nwin ? 2048 : 1024;
    if ((n_fft != 1024 && n_fft != 2048) || (nwin && n_fft != 2048)) return 2;
    const ModelTable m = model_table(nwin, n_fft / 2);
    const int nbr = m.nbr;
    const Levels lv = model_levels(m, t_pad);
    // One lass_separate as the library plans it (HEAD = 1; the composed head-shortcut weights exist).  HEAD = 0 takes the head
    // off: no head_sc_fold, and decoder_block6 on a default site, as the stage call runs it.
    const SeparatePlan sp = plan_separate(cfg, m, lv, B, head);
    // The planned route of each block; computed here only for X_ALIGNED = 0 (the same site with an input that misses pw_gemm.hip's
    // alignment, as a stage call can be handed one) and for HEAD = 0's decoder_block6
    const auto route = [&](const BlockShape& b, int e, BlockIO io, const BlockRoute* planned) {
        if (planned && aligned) return *planned;
        io.x_aligned = aligned;
        return plan_block(cfg, b, B, lv.eh[e], lv.ew[e], io);
    };
    for (int i = 0; i < 7; ++i)
        for (int k = 0; k < (i == 0 ? nbr : 1); ++k) {
            const std::string name = i == 0 && nwin ? "encoder_block1s." + std::to_string(k) : m.E[i].name;
            print_block(name, m.enc_shape(i), route(m.enc_shape(i), i, sp.enc_io[i], &sp.enc_rt[i]));
        }
    for (int d = 0; d < 6; ++d) {
        const bool stage = d == 5 && !head;
        print_block(m.D[d].name, m.dec_shape(d), route(m.dec_shape(d), 5 - d, stage ? BlockIO() : sp.dec_io[d], stage ? nullptr : &sp.dec_rt[d]));
    }
    // The lines below come with the MODE argument only: a command line of up to ten arguments prints what it always printed.
    if (argc <= 11) return 0;
    // (the stage calls have no hand-overs and no fused forms)
    for (int d = 0; d < 6; ++d)
        printf("up %s %s in_act=%d out_copies=%d\n", m.D[d].name, kUpFamily[sp.up[d].family], (int)sp.up[d].in_act, (int)sp.up[d].out_copies);
    if (!cfg.f32()) {
        for (int i = 0; i < 7; ++i)
            for (int k = 0; k < (i == 0 ? nbr : 1); ++k)
                print_bf16(i == 0 && nwin ? "encoder_block1s." + std::to_string(k) : m.E[i].name, sp.enc[i]);
        for (int d = 0; d < 6; ++d) print_bf16(m.D[d].name, sp.dec[d]);
    }
    printf("scopes conv3x3=%d tconv=%d\n", sp.conv_scopes, sp.tconv_scopes);
    return 0;
}
