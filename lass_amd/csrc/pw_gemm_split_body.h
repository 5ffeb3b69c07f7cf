// pw_gemm_split_body.h - the body of the split-bf16 GEMM kernels, included ONCE PER KERNEL inside the function braces (text and
// not a device function, for wino4_body.h's reason): pw_gemm_split_kernel (pw_gemm.hip) and wino4_gemm_kernel (wino4_gemm.hip).
// In scope: TCONV, XI, ACC2, `p`, `sw`.  XI: the batch index is the Winograd point xi - every "clip" has a weight matrix of its own
// (sw.w holds them one behind the other, [xi][3 pieces][K / 8][Nw][8]) and the accumulators start at zero instead of the bias.
// ACC2: the five small piece products of every chunk go to an accumulator set of their own (64 more registers), which is added to
// the hh sums once, behind the last chunk: the large accumulator is rounded once per chunk instead of six times.
    __shared__ __attribute__((aligned(16))) bf16x8 lds[2][2][3][SPLANE];  // [buffer][0 = W, 1 = X][piece][k octet][column]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave >> 1, wp = wave & 1;  // this wave's 64 couts / 64 pixels of the workgroup tile
    int bx, by, b;
    block_coords(p, bx, by, b);
    const int n0 = by * NB;
    const unsigned P = (unsigned)p.H * (unsigned)p.W;  // pixels per channel
    const unsigned p0 = (unsigned)bx * PB;
    const int K = TCONV ? p.Cin : p.Cin2;
    const unsigned Nw = (unsigned)p.Nw;

    // staging: thread = (k octet so of the chunk, column sc) of both operands; so is the same for a whole wave, so the prologue's
    // per-channel scale and shift are scalar loads.  Past the last pixel the column is clamped to the last one (loaded, never
    // stored to memory)
    const int sc = tid & (NB - 1), so = __builtin_amdgcn_readfirstlane(tid >> 7);
    const float* xs = (TCONV ? p.in + (size_t)b * p.in_bs : p.in2 + (size_t)b * p.in2_bs) + min(p0 + (unsigned)sc, P - 1u) +
                      (size_t)(so * 8) * P;
    const size_t wplane = (size_t)(K / 8) * Nw;  // 16-byte units of one piece of W
    const bf16x8* ws = reinterpret_cast<const bf16x8*>(sw.w) + (XI ? (size_t)b * 3 * wplane : (size_t)0) + (size_t)so * Nw + n0 + sc;
    const float* psc = TCONV ? p.pro_scale + so * 8 : nullptr;
    const float* psh = TCONV ? p.pro_shift + (size_t)b * p.pro_shift_bs + so * 8 : nullptr;
    // Two register stages, as in the f32 kernel (indexed only statically: the chunk loop is unrolled by two).  One chunk is 768
    // MFMA cycles per wave: shorter still against a memory round trip
    struct Act {  // scale and shift of a stage's 8 channels: wave-uniform, in scalar registers
        float s[8], h[8];
    };
    struct Stage {
        float x[8];
        bf16x8 w[3];
        Act a;
    };
    Stage S0, S1;
    const auto aload = [&](Act& a, int ch) {
        if (TCONV) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                a.s[j] = psc[(size_t)ch * KC + j];
                a.h[j] = psh[(size_t)ch * KC + j];
            }
        }
    };
    const auto gload = [&](Stage& st, int ch) {
        const size_t k = (size_t)ch * KC;
#pragma unroll
        for (int j = 0; j < 8; ++j) st.x[j] = xs[(k + j) * P];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) st.w[pc] = ws[pc * wplane + (size_t)ch * (KC / 8) * Nw];
    };
    // Staging in two halves, so that each can sit under its own part of a chunk's MFMAs: the prologue and the split, applied once
    // per staged element (vector arithmetic alone), and the six LDS writes
    const auto sprep = [&](const Stage& st, bf16x8 (&xp)[3]) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = TCONV ? leaky(fmaf(st.x[j], st.a.s[j], st.a.h[j])) : st.x[j];  // (resunet.py:247)
        split3(x, xp[0], xp[1], xp[2]);
    };
    const auto swrite = [&](const Stage& st, const bf16x8 (&xp)[3], int buf) {
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
            lds[buf][0][pc][so * NB + sc] = st.w[pc];
            lds[buf][1][pc][so * PB + sc] = xp[pc];
        }
    };

    f32x16 acc[2][2];
    if constexpr (XI)
        acc_zero(acc);
    else
        acc_init<TCONV>(p, acc, n0, wn, lane);
    f32x16 accs[2][2];  // (ACC2 only)
    if constexpr (ACC2) acc_zero(accs);

    // fragments: A[i = lane & 31][k = 8 (lane >> 5) ... + 7] = W[k][n], B[k = 8 (lane >> 5) ... + 7][j = lane & 31] = X[k][pixel]
    const int fo = (lane >> 5) * NB + (lane & 31);
    // the six products in ONE fixed order, smallest first; every accumulator sees the same order whatever the batch
    constexpr int WP[6] = {2, 0, 1, 1, 0, 0}, XP[6] = {0, 2, 1, 0, 1, 0};  // (lh, hl, mm, mh, hm, hh): 0 = h, 1 = m, 2 = l
    const auto prod = [&](const bf16x8 (&fa)[3][2], const bf16x8 (&fb)[3][2], int t) {
        f32x16(&d)[2][2] = (ACC2 && t < 5) ? accs : acc;  // (the small products: their own accumulators)
        d[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][0], d[0][0], 0, 0, 0);
        d[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][1], d[0][1], 0, 0, 0);
        d[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][0], d[1][0], 0, 0, 0);
        d[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][1], d[1][1], 0, 0, 0);
    };
    // One chunk of one wave: the 24 MFMAs of LDS buffer `buf`, and between them the staging of the other buffer from stage `st`,
    // whose registers then take chunk `chn`.  Nothing in a chunk waits for anything else in it, so nothing is fenced off (round 21):
    //   - the twelve fragment reads leave in the order the products take them - (W l, X h) for lh, (W h, X l) for hl, both m
    //     pieces for mm - and LDS returns them in order: hipcc's counted lgkmcnt lets lh start behind the first three reads, the
    //     others land under the MFMAs (lgkmcnt 9, 8, 5, 4, 1, 0);
    //   - lh, hl and mm carry the prologue and the split of the staged X, a few vector instructions behind each MFMA;
    //   - mh, hm and hh carry the six LDS writes and the global loads.  The scalar loads of the next scale and shift are issued
    //     HERE and not earlier: scalar memory shares lgkmcnt with LDS and returns out of order, so with one of them in flight every
    //     wait for a fragment is lgkmcnt(0).  Here the fragments have all landed; the barrier's own lgkmcnt(0) takes the loads.
    // The MFMAs, their operands and their order per accumulator are those of the plain sequence: every sum keeps its bits.
    constexpr int NV = TCONV ? 9 : 7;  // vector instructions behind each of the first twelve MFMAs: all of sprep's, spread
    const auto phase = [&](int buf, Stage& st, int chn) {
        bf16x8 fa[3][2], fb[3][2];  // [piece][tile]
        bf16x8 xp[3];
        constexpr int RW[3] = {2, 0, 1}, RX[3] = {0, 2, 1};
#pragma unroll
        for (int g = 0; g < 3; ++g) {
#pragma unroll
            for (int t = 0; t < 2; ++t) fa[RW[g]][t] = lds[buf][0][RW[g]][fo + wn * 64 + t * 32];
#pragma unroll
            for (int t = 0; t < 2; ++t) fb[RX[g]][t] = lds[buf][1][RX[g]][fo + wp * 64 + t * 32];
            __builtin_amdgcn_sched_barrier(0);  // (pinned: the counted waits count on this order)
        }
        prod(fa, fb, 0);
        prod(fa, fb, 1);
        prod(fa, fb, 2);
        sprep(st, xp);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // one MFMA
            __builtin_amdgcn_sched_group_barrier(0x002, NV, 0);  // vector instructions
        }
        __builtin_amdgcn_sched_barrier(0);
        aload(st.a, chn);
        __builtin_amdgcn_sched_barrier(0);  // (issued here: hipcc sinks them to the barrier otherwise, their latency exposed)
        prod(fa, fb, 3);
        prod(fa, fb, 4);
        prod(fa, fb, 5);
        swrite(st, xp, buf ^ 1);
        gload(st, chn);
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
            if (i < 6) __builtin_amdgcn_sched_group_barrier(0x200, 1, 1);   // one LDS write
            if (i >= 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 1);  // one global load
        }
        __builtin_amdgcn_sched_barrier(0);
    };
    // The f32 kernel's pipeline: chunk c in stage c % 2 and LDS buffer c % 2, nch even, one barrier per chunk, unconditional
    // loads (past the end: the last chunk again, never used)
    const int nch = K / KC;
    aload(S0.a, 0);
    aload(S1.a, 1);
    gload(S0, 0);
    gload(S1, 1);
    {
        bf16x8 xp[3];
        sprep(S0, xp);
        swrite(S0, xp, 0);
    }
    aload(S0.a, min(2, nch - 1));
    gload(S0, min(2, nch - 1));
    __syncthreads();
    // Entered without a guard (nch >= 2, host-checked): behind a guard hipcc sinks the scalar loads above into the loop's
    // preheader, past the barrier, and the first fragment wait of every other chunk becomes lgkmcnt(0)
    int ch = 0;
    do {
        phase(0, S1, min(ch + 3, nch - 1));  // chunk ch
        __syncthreads();
        phase(1, S0, min(ch + 4, nch - 1));  // chunk ch + 1 (behind the last chunk its staging is unused)
        __syncthreads();
        ch += 2;
    } while (ch < nch);
    if constexpr (ACC2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += accs[i][j][r];  // (element by element: a vector add is v_pk_add_f32)
    }
    store_tile<TCONV>(p, acc, b, n0, p0, P, wn, wp, lane);
