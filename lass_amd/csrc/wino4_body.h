// wino4_body.h - the body of wino4.hip's conv kernels, included ONCE PER KERNEL inside the function braces: wino4_kernel
// (ConvArgs alone), wino4_splitk_kernel (ConvArgs + Wino4Split), wino4_vpre_kernel (+ Wino4VPre) and wino4_sclogit_kernel (ConvArgs + HeadScPlanes).  In scope: TC, FLAGS, `p`, `sk`, `vp`, `hs`.  Text inclusion and not an
// inlined device function on purpose: hipcc schedules a kernel whose body arrives through a call differently, and the unsplit
// kernels are to stay instruction for instruction what they were before the split-K variant existed.
    constexpr bool PRO = (FLAGS & F_PRO) != 0, EPI = (FLAGS & F_EPIACT) != 0, SC = (FLAGS & F_PHASEB) != 0;
    constexpr bool PRE = (FLAGS & F_PRECONV) != 0;   // the input is the 1-channel x0: channel c = pre_w[c] * x0 + pre_b[c] (resunet.py:555)
    constexpr bool RESPRE = (FLAGS & F_RESPRE) != 0; // identity residual = pre_conv(x0), never materialised (encoder_block1.conv2)
    constexpr bool MASK = (FLAGS & F_MASK) != 0;     // epilogue = after_conv + complex ratio mask; the block output is not written
    constexpr bool RES = (FLAGS & F_RES) != 0;       // + residual: pre_conv(x0) (RESPRE) or read from p.res, possibly in place
    static_assert(!SC || (FLAGS & F_BIAS) != 0, "the shortcut conv has a bias");
    static_assert(!PRE || PRO, "pre_conv is folded into the prologue's affine");
    static_assert(!RESPRE || ((FLAGS & F_RES) != 0 && !SC && !EPI), "conv2 with the identity residual");
    static_assert(!MASK || SC, "the output head sits behind decoder_block6's conv2 + shortcut");
    static_assert(!RES || (!SC && !EPI), "conv2 with a residual in place of the fused shortcut");
    constexpr bool SPLIT = (FLAGS & F_SPLITK) != 0;  // partial sums only: the epilogue runs in wino4_combine_kernel
    static_assert(!SPLIT || (FLAGS & ~(F_SPLITK | F_PRO | F_VPRE)) == 0, "a split launch has a prologue at most");
    // the transformed input arrives from memory (Wino4VPre, written by wino4_vprep_kernel): no patch loads, prologue or transform here
    constexpr bool VPRE = (FLAGS & F_VPRE) != 0;
    static_assert(!VPRE || (FLAGS & ~(F_VPRE | F_SPLITK | F_EPIACT | F_RES)) == 0, "conv1 / identity conv2 / split share: the prologue ran in the prep launch");
    // encoder_block1.conv2 of the head_sc_fold route (conv_route.h): the epilogue also forms the folded head's shortcut logits of the
    // skip, hs.skip[b][q] = sum_c hs.w[q][c] x1[c], from the registers the skip is stored from
    constexpr bool SCL = (FLAGS & F_SCLOGIT) != 0;
    static_assert(!SCL || (FLAGS == (F_RES | F_RESPRE | F_SCLOGIT) && TC == 16), "the skip's logits: encoder_block1.conv2 on the 8 x 64 blocks");
    constexpr int TR = 32 / TC;
    constexpr int OR_ = 4 * TR, OC = 4 * TC;
    constexpr int NCO = 32;  // output channels of the workgroup
    __shared__ __attribute__((aligned(16))) float lds[U_F + V_F + 2 * NCO + (MASK ? 100 : 0) + (SCL ? 96 : 0)];
    float* lu = lds;
    float* lv = lds + U_F;
    float* lds_es = lv + V_F;
    float* lds_eh = lds_es + NCO;
    float* lds_mw = lds_eh + NCO;  // MASK: after_conv weight [3][32] + bias [3]; SCL: Wsc'_skip [3][32]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wco = wave >> 1, wwt = wave & 1;  // cout tile (16 couts, 0 .. 1) / tile group (16 tiles) of this wave
    int bx_, by_, b, ks = 0;
    if constexpr (SPLIT) {
        // (block, clip, split) triples take the place of block_coords' (block, clip) pairs: with xcd_map the gy cout groups of
        // a triple - which read the same input channels - run on one XCD
        const unsigned lin = blockIdx.x, ngrp = (unsigned)(p.gx * p.B * sk.n);
        unsigned grp;
        if (p.xcd_map) {
            const unsigned j = lin >> 3;
            grp = (lin & 7u) * (ngrp >> 3) + j / (unsigned)p.gy;
            by_ = (int)(j % (unsigned)p.gy);
        } else {
            grp = lin / (unsigned)p.gy;
            by_ = (int)(lin % (unsigned)p.gy);
        }
        ks = (int)(grp % (unsigned)sk.n);
        const unsigned xz = grp / (unsigned)sk.n;
        b = (int)(xz / (unsigned)p.gx);
        bx_ = (int)(xz % (unsigned)p.gx);
    } else {
        block_coords(p, bx_, by_, b);
    }
    const int n0 = by_ * NCO;
    const int tiles_x = p.W / OC;
    const int y0 = (bx_ / tiles_x) * OR_, x0 = (bx_ % tiles_x) * OC;
    const int HW = p.H * p.W;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = PRO ? p.pro_scale : nullptr;
    const float* sh = PRO ? p.pro_shift + (size_t)b * p.pro_shift_bs : nullptr;

    if (EPI && tid < NCO) {
        lds_es[tid] = p.epi_scale[n0 + tid];
        lds_eh[tid] = p.epi_shift[(size_t)b * p.epi_shift_bs + n0 + tid];
    }
    if (SC && tid < NCO) lds_es[tid] = p.bias[n0 + tid];  // (SC and EPI exclude each other: one table)
    if (RESPRE && tid < 32) {                               // residual affine of this block's 32 output channels
        lds_es[tid] = p.pre_w[n0 + tid];
        lds_eh[tid] = p.pre_b[n0 + tid];
    }
    if (MASK && tid < 99) lds_mw[tid] = tid < 96 ? p.mask_w[tid] : p.mask_b[tid - 96];
    if constexpr (SCL) {
        if (tid < 96) lds_mw[tid] = hs.w[tid];
    }

    f32x4 acc[NXI];
#pragma unroll
    for (int xi = 0; xi < NXI; ++xi)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[xi][r] = 0.f;

    const int kq = lane >> 4, l15 = lane & 15;
    // fragments: U image [xi][t][kq][l15][k]: this lane's {k-step 0, k-step 1} of cout tile wco; V image [xi][kq][tile ^ swz][k]
    // (wco >> 1 is 0: one 32-cout slab.  Kept spelled out, as is the redundant mask of c8 below: either simplification changes
    // the compiled kernels - one VGPR more for the F_MASK ones)
    const float* afrag = lu + (wco >> 1) * U_F + (wco & 1) * 128 + (kq * 16 + l15) * 2;
    const float* bfrag = lv + (kq * 32 + ((wwt * 16 + l15) ^ ((kq & 1) << 4))) * 2;
    const unsigned slab_pitch = (unsigned)(p.Nw / 32) * (unsigned)(U_F * 4);  // bytes between the slabs of consecutive chunks
    const unsigned slab_n0 = (unsigned)(n0 / 32) * (unsigned)(U_F * 4);
    const unsigned lu_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lu;
    const unsigned ulane = (unsigned)lane * 16u;
    const v4i32 uw = make_rsrc_words(p.w_wino4, (unsigned)(NXI * p.Cin * p.Nw) * 4u);

#include "wino4_input.h"
    // VPRE: the V slabs of this (clip, block), one per chunk, each the LDS image byte for byte
    const unsigned lv_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lv;
    const v4i32 vw = make_rsrc_words(VPRE ? vp.v + ((size_t)b * p.gx + bx_) * (size_t)(p.Cin / KC) * V_F : nullptr,
                                     (unsigned)(p.Cin / KC) * (unsigned)(V_F * 4));

    // chunks [ch0, nch) of 8 input channels: all of them, or share ks of a split launch
    const int ch0 = SPLIT ? ks * (p.Cin / KC) / sk.n : 0;
    const int nch = SPLIT ? (ks + 1) * (p.Cin / KC) / sk.n : p.Cin / KC;
    if constexpr (!VPRE) pload(ch0);
    lds_barrier();  // epilogue tables visible
    for (int ch = ch0; ch < nch; ++ch) {
        lds_barrier();  // previous chunk's MFMAs have finished reading V / U
        __builtin_amdgcn_s_setprio(2);
        // The patch of this chunk was requested a whole MFMA phase ago.  Pin it as arrived HERE: hipcc counts only its own
        // loads, so a wait placed behind the LDS-DMA below would be vmcnt(0) and drain the weight slab before the transform.
        if constexpr (!VPRE) {
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                asm volatile("" : "+v"(pc[i].x), "+v"(pc[i].y), "+v"(pc[i].z), "+v"(pc[i].w), "+v"(pl[i]), "+v"(pr[i]));
            }
            if (PRO) asm volatile("" : "+v"(ps), "+v"(ph));
        }
        // weight slab of (chunk ch, cout group n0 / 32): 36 pieces of 1 KiB, 9 per wave
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const unsigned piece = (unsigned)(wave * 9 + i) * 1024u;
            lds_dma_16B(uw, ulane, (unsigned)ch * slab_pitch + slab_n0 + piece, lu_addr + piece);
        }
        if constexpr (VPRE) {  // ... and the V slab of (chunk ch, this block): 9 more pieces per wave, nothing else in flight
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                const unsigned piece = (unsigned)(wave * 9 + i) * 1024u;
                lds_dma_16B(vw, ulane, (unsigned)ch * (unsigned)(V_F * 4) + piece, lv_addr + piece);
            }
            wait_vmcnt<0>();
        } else {
            __builtin_amdgcn_sched_barrier(0);
            pprocess();
            __builtin_amdgcn_sched_barrier(0);
            const bool pf = ch + 1 < nch;
            if (pf) pload(ch + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (pf)
                wait_vmcnt<NLOAD>();  // this wave's pieces of U(ch) have landed; the patch of chunk ch+1 stays in flight
            else
                wait_vmcnt<0>();
        }
        lds_barrier();  // V visible, every wave's U pieces landed
        __builtin_amdgcn_s_setprio(0);
        // 36 GEMM steps x 2 k-steps; two xi in flight so that no MFMA depends on its predecessor (40-cycle dependent latency)
        constexpr int PFD = 2;  // pairs of fragment reads ahead
        f32x2v av[PFD + 1][2], bv[PFD + 1][2];
        auto rd = [&](int s) {  // step s = xi pair (2s, 2s+1)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                av[s % (PFD + 1)][q] = *reinterpret_cast<const f32x2v*>(afrag + (2 * s + q) * 256);
                bv[s % (PFD + 1)][q] = *reinterpret_cast<const f32x2v*>(bfrag + (2 * s + q) * 256);
            }
        };
#pragma unroll
        for (int s = 0; s < PFD; ++s) rd(s);
#pragma unroll
        for (int s = 0; s < NXI / 2; ++s) {
            if (s + PFD < NXI / 2) rd(s + PFD);
            __builtin_amdgcn_sched_barrier(0);
            const f32x2v a0 = av[s % (PFD + 1)][0], a1 = av[s % (PFD + 1)][1];
            const f32x2v b0 = bv[s % (PFD + 1)][0], b1 = bv[s % (PFD + 1)][1];
            acc[2 * s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, acc[2 * s], 0, 0, 0);
            acc[2 * s + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, acc[2 * s + 1], 0, 0, 0);
            acc[2 * s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, acc[2 * s], 0, 0, 0);
            acc[2 * s + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, acc[2 * s + 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- output transform Y = A^T M A: this lane's 4 couts (D rows kq * 4 + r) x the 16 pixels of its tile ----------------
    const int ot = wwt * 16 + l15;  // this lane's tile
    const int oy = y0 + 4 * (ot / TC), ox = x0 + 4 * (ot % TC);
    f32x4 ysp[16];  // [sub-pixel a * 4 + c][r]: tile s of the MFMA D layout [16 couts][16 tiles]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int nl = wco * 16 + kq * 4 + r;
        float tmp[4][6];
#pragma unroll
        for (int jx = 0; jx < 6; ++jx) {
            const float m[6] = {acc[0 + jx][r], acc[6 + jx][r], acc[12 + jx][r], acc[18 + jx][r], acc[24 + jx][r], acc[30 + jx][r]};
            float y[4];
            at6(m, y);
#pragma unroll
            for (int a = 0; a < 4; ++a) tmp[a][jx] = y[a];
        }
        const float es = (EPI || SC) ? lds_es[nl] : 0.f, eh = EPI ? lds_eh[nl] : 0.f;  // SC: es = the shortcut's bias
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float y[4];
            at6(tmp[a], y);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                float v = y[c];
                if (EPI) v = leaky(fmaf(v, es, eh));  // bn2 + FiLM + leaky (resunet.py:151)
                if (SC) v += es;
                ysp[a * 4 + c][r] = v;
            }
        }
    }
    if constexpr (SPLIT) {  // the output transform is linear: this share's 4 couts x 16 pixels go out as they are
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = n0 + wco * 16 + kq * 4 + r;
            float* dst = sk.part + (((size_t)ks * p.B + b) * p.N + n) * HW + (size_t)oy * p.W + ox;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float4 o = make_float4(ysp[a * 4 + 0][r], ysp[a * 4 + 1][r], ysp[a * 4 + 2][r], ysp[a * 4 + 3][r]);
                if (oy + a < p.H) *reinterpret_cast<float4*>(dst + (size_t)a * p.W) = o;
            }
        }
        return;
    }
    if constexpr (RESPRE) {  // + pre_conv(x0) at this lane's 16 pixels (resunet.py:555,165)
        const float* xr = p.res + (size_t)b * p.res_bs + (size_t)min(oy, p.H - 4) * p.W + ox;
        float4 xv[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) xv[a] = *reinterpret_cast<const float4*>(xr + (size_t)a * p.W);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pw = lds_es[wco * 16 + kq * 4 + r], pb = lds_eh[wco * 16 + kq * 4 + r];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                ysp[a * 4 + 0][r] += fmaf(xv[a].x, pw, pb);
                ysp[a * 4 + 1][r] += fmaf(xv[a].y, pw, pb);
                ysp[a * 4 + 2][r] += fmaf(xv[a].z, pw, pb);
                ysp[a * 4 + 3][r] += fmaf(xv[a].w, pw, pb);
            }
        }
    }
    if constexpr (SCL) {
        // ---- the skip's share of the head's shortcut logits, in the shape of the F_MASK reduction below: the 32 channels of a
        // pixel sit in the 4 kq lane groups of the 2 cout waves.  Every lane forms its partial logits (3 x 16 pixels over its 4
        // channels, fixed order) and leaves them in the dead U / V region, [source = wco * 4 + kq][logit][pixel = tile * 16 + s];
        // they are summed behind the skip's stores, which need no LDS.
        float* part = lds;  // 8 * 3 * 512 floats = 48 KiB <= U_F + V_F
        lds_barrier();      // every wave is past its last MFMA phase
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float w4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) w4[r] = lds_mw[q * 32 + wco * 16 + kq * 4 + r];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                float4 o;
                float* op = &o.x;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 v = ysp[a * 4 + c];
                    op[c] = fmaf(v[3], w4[3], fmaf(v[2], w4[2], fmaf(v[1], w4[1], v[0] * w4[0])));
                }
                *reinterpret_cast<float4*>(part + ((wco * 4 + kq) * 3 + q) * 512 + ot * 16 + a * 4) = o;
            }
        }
    }
    if constexpr (RES && !RESPRE) {
        // + the residual at this lane's 4 couts x 16 pixels (resunet.py:165): for the routed shortcut layers bias + Wsc x, which
        // pw_gemm.hip wrote into the output slot itself - read here and overwritten below by the same lane.  All 16 rows are
        // fetched in one batch in front of the stores (a load behind a store to `out` cannot be hoisted over it).
        float4 rv[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float* rr = p.res + (size_t)b * p.res_bs + (size_t)(n0 + wco * 16 + kq * 4 + r) * HW + (size_t)min(oy, p.H - 4) * p.W + ox;
#pragma unroll
            for (int a = 0; a < 4; ++a) rv[r][a] = *reinterpret_cast<const float4*>(rr + (size_t)a * p.W);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                ysp[a * 4 + 0][r] += rv[r][a].x;
                ysp[a * 4 + 1][r] += rv[r][a].y;
                ysp[a * 4 + 2][r] += rv[r][a].z;
                ysp[a * 4 + 3][r] += rv[r][a].w;
            }
    }
    if constexpr (SC) {
        // ---- 1x1 shortcut over the raw block input (resunet.py:163), direct: per 4 input channels 16 MFMAs, one per sub-pixel;
        // B[k = kq][col = l15] = x[channel 4 ks + kq][this lane's tile, sub-pixel s] (four 16-byte row loads),
        // A[row = l15][k = kq] = Wsc[cout wco * 16 + l15][channel 4 ks + kq]; operands of k-step ks + 1 are requested first
        const float* x2 = p.in2 + (size_t)b * p.in2_bs + (size_t)min(oy, p.H - 4) * p.W + ox;
        const float* wsc = p.w2 + n0 + wco * 16 + l15;  // [Cin2][Nw]
        const int nks = p.Cin2 / 4;
        // operands of the next THREE k-steps are in flight behind the 16 MFMAs of the current one (512 cycles: less than one
        // L2 round trip under load); the accumulators of the main phase are dead here, registers are free
        constexpr int NSB = 4;
        float4 xb[NSB][4];
        float wa[NSB];
        auto ldk = [&](int ks, int buf) {
            const float* xp = x2 + (size_t)(4 * ks + kq) * HW;
#pragma unroll
            for (int a = 0; a < 4; ++a) xb[buf][a] = *reinterpret_cast<const float4*>(xp + (size_t)a * p.W);
            wa[buf] = wsc[(size_t)(4 * ks + kq) * p.Nw];
        };
        auto mmk = [&](int buf) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                ysp[a * 4 + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[buf], xb[buf][a].x, ysp[a * 4 + 0], 0, 0, 0);
                ysp[a * 4 + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[buf], xb[buf][a].y, ysp[a * 4 + 1], 0, 0, 0);
                ysp[a * 4 + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[buf], xb[buf][a].z, ysp[a * 4 + 2], 0, 0, 0);
                ysp[a * 4 + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[buf], xb[buf][a].w, ysp[a * 4 + 3], 0, 0, 0);
            }
        };
        ldk(0, 0);
        ldk(1, 1);
        ldk(2, 2);
        for (int ks = 0; ks < nks; ks += NSB) {  // Cin2 % 16 == 0 (host-checked): whole groups of NSB k-steps
#pragma unroll
            for (int u = 0; u < NSB; ++u) {
                ldk(min(ks + u + 3, nks - 1), (u + 3) % NSB);  // (behind the end: the last k-step again, unused)
                __builtin_amdgcn_sched_barrier(0);
                mmk(u);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    if constexpr (MASK) {
        // ---- fused output head (resunet.py:570-574,436-519): after_conv needs all 32 channels of a pixel; they sit in the 4 kq
        // lane groups of the 2 cout waves.  Every lane forms its partial logits (3 x 16 pixels over its 4 channels) and leaves
        // them in the dead U / V region, [source = wco * 4 + kq][logit][pixel = tile * 16 + s]; then every thread finishes 2 pixels.
        float* part = lds;  // 8 * 3 * 512 floats = 48 KiB <= U_F + V_F
        lds_barrier();      // every wave is past its last MFMA phase
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float w4[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) w4[r] = lds_mw[q * 32 + wco * 16 + kq * 4 + r];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                float4 o;
                float* op = &o.x;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const f32x4 v = ysp[a * 4 + c];
                    op[c] = v[0] * w4[0] + v[1] * w4[1] + v[2] * w4[2] + v[3] * w4[3];
                }
                *reinterpret_cast<float4*>(part + ((wco * 4 + kq) * 3 + q) * 512 + ot * 16 + a * 4) = o;
            }
        }
        lds_barrier();
        const int px = tid * 2;  // pixels px, px + 1: same tile, same row
        const int mt = px >> 4, ms = px & 15;
        const int my = y0 + 4 * (mt / TC) + (ms >> 2), mx = x0 + 4 * (mt % TC) + (ms & 3);
        float lg[3][2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float2 sum = make_float2(lds_mw[96 + q], lds_mw[96 + q]);
#pragma unroll
            for (int src = 0; src < 8; ++src) {
                const float2 v = *reinterpret_cast<const float2*>(part + (src * 3 + q) * 512 + px);
                sum.x += v.x;
                sum.y += v.y;
            }
            lg[q][0] = sum.x;
            lg[q][1] = sum.y;
        }
        if (my < p.mask_T) {
            mask_pixel(p, b, my, mx, lg[0][0], lg[1][0], lg[2][0]);
            mask_pixel(p, b, my, mx + 1, lg[0][1], lg[1][1], lg[2][1]);
        }
        return;
    }
    // ---- stores: 16-byte rows; the block's 2x2 avg-pool (resunet.py:197) from the same registers -----------------------------
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = n0 + wco * 16 + kq * 4 + r;
        float* dst = p.out + (size_t)b * p.out_bs + (size_t)n * HW + (size_t)oy * p.W + ox;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float4 o = make_float4(ysp[a * 4 + 0][r], ysp[a * 4 + 1][r], ysp[a * 4 + 2][r], ysp[a * 4 + 3][r]);
            if (oy + a < p.H) *reinterpret_cast<float4*>(dst + (size_t)a * p.W) = o;
        }
        if constexpr (TC == 4 && RES) {  // the 16-bin level pools 1 x 2 (encoder_block6); pool_h == 2 falls through
            if (p.pool_out && p.pool_h == 1) {
                const int Wo = p.W / 2;
                float* pd = p.pool_out + (size_t)b * (p.pool_bs ? (size_t)p.pool_bs : (size_t)p.N * p.H * Wo) + (size_t)n * p.H * Wo +
                            (size_t)oy * Wo + (ox >> 1);
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    float2 o;
                    o.x = (ysp[a * 4 + 0][r] + ysp[a * 4 + 1][r]) * 0.5f;
                    o.y = (ysp[a * 4 + 2][r] + ysp[a * 4 + 3][r]) * 0.5f;
                    if (oy + a < p.H) *reinterpret_cast<float2*>(pd + (size_t)a * Wo) = o;
                }
                continue;
            }
        }
        if ((SC || RES) && p.pool_out) {  // wave-uniform; pool_h == 2 (host-checked): row-major summation order of F.avg_pool2d
            const int Ho = p.H / 2, Wo = p.W / 2;
            float* pd = p.pool_out + (size_t)b * (p.pool_bs ? (size_t)p.pool_bs : (size_t)p.N * Ho * Wo) + (size_t)n * Ho * Wo +
                        (size_t)(oy >> 1) * Wo + (ox >> 1);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float2 o;
                float s0 = ysp[(2 * i) * 4 + 0][r] + ysp[(2 * i) * 4 + 1][r];
                s0 += ysp[(2 * i + 1) * 4 + 0][r];
                s0 += ysp[(2 * i + 1) * 4 + 1][r];
                float s1 = ysp[(2 * i) * 4 + 2][r] + ysp[(2 * i) * 4 + 3][r];
                s1 += ysp[(2 * i + 1) * 4 + 2][r];
                s1 += ysp[(2 * i + 1) * 4 + 3][r];
                o.x = s0 * 0.25f;
                o.y = s1 * 0.25f;
                if (oy + 2 * i + 1 < p.H) *reinterpret_cast<float2*>(pd + (size_t)i * Wo) = o;
            }
        }
    }
    if constexpr (SCL) {
        // ---- every thread sums 2 pixels (same tile, same row) over the 8 sources, in source order: a clip's planes depend on
        // nothing but the clip
        const float* part = lds;
        lds_barrier();
        const int px = tid * 2;
        const int mt = px >> 4, ms = px & 15;
        const int my = y0 + 4 * (mt / TC) + (ms >> 2), mx = x0 + 4 * (mt % TC) + (ms & 3);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            float2 sum = *reinterpret_cast<const float2*>(part + q * 512 + px);
#pragma unroll
            for (int src = 1; src < 8; ++src) {
                const float2 v = *reinterpret_cast<const float2*>(part + (src * 3 + q) * 512 + px);
                sum.x += v.x;
                sum.y += v.y;
            }
            if (my < p.H) *reinterpret_cast<float2*>(hs.skip + ((size_t)b * 3 + q) * HW + (size_t)my * p.W + mx) = sum;
        }
    }
