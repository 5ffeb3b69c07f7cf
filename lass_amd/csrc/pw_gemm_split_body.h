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
    Act T;
    // The scalar loads of a stage are issued in FRONT of a chunk's MFMAs, into T, and handed to the stage behind them: issued
    // with the vector loads they would sit right in front of the barrier's lgkmcnt(0), their latency exposed in every chunk
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
    const auto sstore = [&](const Stage& st, int buf) {  // the prologue and the split are applied here, once per staged element
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = TCONV ? leaky(fmaf(st.x[j], st.a.s[j], st.a.h[j])) : st.x[j];  // (resunet.py:247)
        bf16x8 xp[3];
        split3(x, xp[0], xp[1], xp[2]);
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
    const auto mma = [&](int buf) {
        bf16x8 fa[3][2], fb[3][2];  // [piece][tile]: all fragments of the chunk requested up front
#pragma unroll
        for (int pc = 0; pc < 3; ++pc)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                fa[pc][t] = lds[buf][0][pc][fo + wn * 64 + t * 32];
                fb[pc][t] = lds[buf][1][pc][fo + wp * 64 + t * 32];
            }
        __builtin_amdgcn_sched_barrier(0);  // (pinned, as in the f32 kernel)
        // the six products in ONE fixed order, smallest first; every accumulator sees the same order whatever the batch
        constexpr int WP[6] = {2, 0, 1, 1, 0, 0}, XP[6] = {0, 2, 1, 0, 1, 0};  // (lh, hl, mm, mh, hm, hh): 0 = h, 1 = m, 2 = l
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            if constexpr (ACC2) {
                if (t < 5) {  // the small products: their own accumulators
                    accs[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][0], accs[0][0], 0, 0, 0);
                    accs[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][1], accs[0][1], 0, 0, 0);
                    accs[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][0], accs[1][0], 0, 0, 0);
                    accs[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][1], accs[1][1], 0, 0, 0);
                    continue;
                }
            }
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][0], acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][0], fb[XP[t]][1], acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][0], acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[WP[t]][1], fb[XP[t]][1], acc[1][1], 0, 0, 0);
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
    sstore(S0, 0);
    aload(S0.a, min(2, nch - 1));
    gload(S0, min(2, nch - 1));
    __syncthreads();
    for (int ch = 0; ch < nch; ch += 2) {
        aload(T, min(ch + 3, nch - 1));
        mma(0);  // chunk ch
        sstore(S1, 1);
        S1.a = T;
        gload(S1, min(ch + 3, nch - 1));
        __syncthreads();
        aload(T, min(ch + 4, nch - 1));
        mma(1);  // chunk ch + 1
        sstore(S0, 0);  // (behind the last chunk: unused)
        S0.a = T;
        gload(S0, min(ch + 4, nch - 1));
        __syncthreads();
    }
    if constexpr (ACC2) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += accs[i][j][r];  // (element by element: a vector add is v_pk_add_f32)
    }
    store_tile<TCONV>(p, acc, b, n0, p0, P, wn, wp, lane);
