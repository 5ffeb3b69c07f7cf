// workspace_table.cpp - one call of lass_separate as lass_amd/csrc/workspace_plan.h plans it: the workspace layout, whether the call
// runs as two half-batches, and the bytes it needs - what lass_workspace_bytes and lass_workspace_tensor answer from.
// Host only: g++ -std=c++17 -I lass_amd/csrc tools/workspace_table.cpp -o tools/bin/workspace_table
// usage: workspace_table WINDOWS N_FFT HOP MODE B L SPLIT_BATCH CAPTURING WORKSPACE_BYTES [switch=value ...]
//   WINDOWS 0: ResUNet30 at (N_FFT, HOP) = (1024, 160) or (2048, 320); a comma list (256,512,2048): the multi-STFT model with
//   these analysis windows (N_FFT 2048, HOP 160)
//   MODE 0: f32, 1: bf16, 2: bf16x3;  SPLIT_BATCH: the LASS_SPLIT value (0, 1, 2);  CAPTURING 1: the launches go into a graph capture
//   WORKSPACE_BYTES: the caller's, or -1 for none (lass_workspace_bytes)
//   switches (defaults as a context's): wino4=32 vprep=1 splits=0 head_fold=1 head_sc_fold=1 wino4_gemm=1 pw_split=1 fuse_catb=1
//   fuse_block=1 fuse_up=1 profiling=0, and head_sc_weights (default: what lass_finalize composes for a complete checkpoint)
// plan B=<n> L=<n> T=<n> Tp=<n> total=<bytes>         exit status 1 and no output: (B, L) is refused
// half B=<n> total=<bytes>                            where the batch can split (split_halves)
// call split=<0|1> need=<bytes> accepted=<0|1>        accepted: the workspace holds the layout the call runs with
// slot <index> <offset> <bytes>                       every slot of the whole-batch plan, in plan order
// tensor <name> <offset> <B,C,H,W> <strides, floats>  every name lass_workspace_tensor knows, whole-batch plan
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "weight_plan.h"
#include "workspace_plan.h"

// The FiLM width of a model (lass_film_width): two sites per ConvBlockRes (cin, cout) and one per transposed conv (its cin)
static int film_width(const ModelTable& m) {
    int n = m.nbr * (m.E[0].cin + m.E[0].cout);
    for (int i = 1; i < 7; ++i) n += m.E[i].cin + m.E[i].cout;
    for (int d = 0; d < 6; ++d) n += m.D[d].cin + m.dec_cat[d] + m.D[d].cout;
    return n;
}

int main(int argc, char** argv) {
    if (argc < 10) {
        fprintf(stderr, "usage: %s WINDOWS N_FFT HOP MODE B L SPLIT_BATCH CAPTURING WORKSPACE_BYTES [switch=value ...]\n", argv[0]);
        return 2;
    }
    Geometry g;
    const int n_fft = atoi(argv[2]), hop = atoi(argv[3]), mode = atoi(argv[4]);
    if (strcmp(argv[1], "0") != 0) {  // lass_create_multistft
        g.variant = 1; g.magphase_sem = 1; g.nbr = 0;
        for (char* p = argv[1]; *p && g.nbr < LASS_MAX_STFT_WINDOWS; p += *p == ',') g.wins[g.nbr++] = (int)strtol(p, &p, 10);
        if (n_fft != 2048 || hop != LASS_HOP || g.nbr < 1) return 2;
    } else if (n_fft == 2048 && hop == 320) {  // lass_create_stft
        g.wins[0] = 2048;
    } else if (n_fft != LASS_NFFT || hop != LASS_HOP) {
        return 2;
    }
    g.nfft = n_fft; g.nbins = n_fft / 2 + 1; g.fcrop = n_fft / 2; g.hop = hop;
    if (mode < 0 || mode > 2) return 2;
    RouteCfg cfg;
    cfg.mode = (ComputeMode)mode;
    int profiling = 0, weights = -1;
    for (int i = 10; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        const std::string k(argv[i], (size_t)(eq - argv[i]));
        const int v = atoi(eq + 1);
        if (k == "wino4") cfg.wino4_mincin = v;
        else if (k == "vprep") cfg.vprep_mode = v;
        else if (k == "splits") cfg.ksplit_force = v;
        else if (k == "head_fold") cfg.head_fold = v != 0;
        else if (k == "head_sc_fold") cfg.head_sc_fold = v != 0;
        else if (k == "wino4_gemm") cfg.wino4_gemm = v != 0;
        else if (k == "pw_split") cfg.pw_split = v != 0;
        else if (k == "fuse_catb") cfg.fuse_catb = v != 0;
        else if (k == "fuse_block") cfg.fuse_block = v != 0;
        else if (k == "fuse_up") cfg.fuse_up = v != 0;
        else if (k == "profiling") profiling = v;
        else if (k == "head_sc_weights") weights = v;
        else return 2;
    }
    const ModelTable m = model_table(g.variant == 0 ? 0 : g.nbr, g.fcrop);
    if (weights < 0) weights = head_sc_weights(cfg, m, 3);  // weight_plan.h: what lass_finalize composes (after_conv has 3 rows)
    const PlanInputs in{g, m, cfg, film_width(m), weights != 0};
    const int B = atoi(argv[5]), L = atoi(argv[6]);
    const long long ws = atoll(argv[9]);
    const size_t workspace_bytes = ws < 0 ? kNoWorkspaceLimit : (size_t)ws;
    const CallPlan cp = plan_call(in, B, L, atoi(argv[7]), profiling != 0, atoi(argv[8]) != 0, workspace_bytes);
    const Plan& pl = cp.whole;
    if (!pl.valid) return 1;
    printf("plan B=%d L=%d T=%d Tp=%d total=%zu\n", pl.B, pl.L, pl.T, pl.Tp, pl.total);
    if (cp.half.valid) printf("half B=%d total=%zu\n", cp.half.B, cp.half.total);
    printf("call split=%d need=%zu accepted=%d\n", (int)cp.split, cp.need, (int)(cp.split || workspace_bytes >= pl.total));
    for (int i = 0; i < pl.nslots; ++i) printf("slot %d %zu %zu\n", i, pl.slot_off[i], pl.slot_bytes[i]);
    for (const PlanTensor& t : plan_tensors(in, pl))
        printf("tensor %s %zu %lld,%lld,%lld,%lld %lld,%lld,%lld,%lld\n", t.name.c_str(), t.offset, (long long)t.shape[0],
               (long long)t.shape[1], (long long)t.shape[2], (long long)t.shape[3], (long long)t.strides[0], (long long)t.strides[1],
               (long long)t.strides[2], (long long)t.strides[3]);
    return 0;
}
