// wino4_head_body.h - the body of wino4.hip's folded-head kernels, included ONCE PER KERNEL inside the function braces (as
// wino4_body.h, and for its reason): wino4_headfold_kernel (ConvArgs alone: the composed shortcut runs here, over in2) and
// wino4_headfold_planes_kernel (ConvArgs + HeadScPlanes: the shortcut's logits arrive as two sets of planes, conv_route.h's
// head_sc_fold).  In scope: TC, PLANES, `p`, `hs`.
//
// The chunk loop contracts on v_mfma_f32_4x4x1_16b_f32: 16 independent 4 x 4 blocks with K = 1, lane 4 b + i holding A row i and
// B column i of block b and, in D register r, element (r, i).  A block's rows are the 3 logits and one zero row, its columns 4
// tiles; the 16 blocks of one instruction are (k-step 2) x (8 groups of 4 tiles) at ONE xi and ONE input channel of the k-step, so
// the 64 B values of an instruction are one whole 256-byte row of the V image.  Wave w owns xi 9 w .. 9 w + 8: per chunk 4
// channels x 9 xi = 36 instructions into 9 accumulators, the channel outermost (9 independent instructions between two on one
// accumulator), each accumulator summing its k-step's channels in ascending order, chunk by chunk - the order of the 16x16x4 form
// this replaces, whose 16 rows held the same 3 logits.
    constexpr bool PRO = false, PRE = false;  // conv2 reads conv1's activated output as it is
    constexpr int TR = 32 / TC;
    constexpr int OR_ = 4 * TR, OC = 4 * TC;
    constexpr int UH_F = kHeadFoldU4Floats;     // 5 KiB: [k-step][row 4][xi][kq], 4.5 KiB of it live (head_fold_u4_index)
    constexpr int NQ = 3;                       // logits
    constexpr int NXW = NXI / 4;                // xi of a wave
    // the hand-over of the accumulators behind the chunk loop, in the dead U / V region: [k-step][logit][xi][tile], the strides
    // padded so that neither its writers (lanes = k-step x tile) nor its readers (lanes = logit x 16 tiles) meet in a bank ...
    constexpr int XQ_F = NXI * 32 + 16, XK_F = NQ * XQ_F + 48, X_F = 2 * XK_F;
    // ... and behind it the partial logits [k-step][logit][pixel = tile * 16 + s] (2 x 3 x 512 floats)
    static_assert(X_F % 4 == 0 && X_F + 2 * NQ * 512 <= UH_F + V_F, "the hand-over images fit into the dead U / V region");
    __shared__ __attribute__((aligned(16))) float lds[UH_F + V_F + kHeadFoldRows];
    float* lu = lds;
    float* lv = lds + UH_F;
    float* lds_b = lv + V_F;  // b'

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, wwt = wave & 1;  // behind the chunk loop: k-step (and half of the shortcut's channels) / tile group of this wave
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);  // (gy = 1)
    const int tiles_x = p.W / OC;
    const int y0 = (bx_ / tiles_x) * OR_, x0 = (bx_ % tiles_x) * OC;
    // Every row of this block lies at or beyond mask_T: mask_pixel is skipped for all of them below, nothing is written.  (The
    // head only: another conv's padded rows feed valid rows further down.)
    if (y0 >= p.mask_T) return;
    const int HW = p.H * p.W;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = nullptr;
    const float* sh = nullptr;
    if (tid < kHeadFoldRows) lds_b[tid] = p.bias[tid];

    f32x4 acc[NXW];  // [xi - 9 wave][logit]: k-step lane >> 5, tile lane & 31
#pragma unroll
    for (int g = 0; g < NXW; ++g)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[g][r] = 0.f;

    const int kq = lane >> 4, l15 = lane & 15;
    const int l31 = lane & 31, lks = lane >> 5;
    // fragments: A = U[k-step lks][row lane & 3][xi 9 wave + g][channel 0 .. 3] in one 16-byte read per xi;
    // B = V[xi][channel c][tile l31 ^ swz(c)][lks], the two swizzles of even and odd c as two bases
    const float* afrag = lu + ((lks * kHeadFoldRows4 + (lane & 3)) * NXI + wave * NXW) * 4;
    const float* bfrag0 = lv + wave * NXW * 256 + l31 * 2 + lks;
    const float* bfrag1 = lv + wave * NXW * 256 + (l31 ^ 16) * 2 + lks;
    const unsigned lu_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lu;
    const unsigned ulane = (unsigned)lane * 16u;
    const v4i32 uw = make_rsrc_words(p.w_wino4, (unsigned)(p.Cin / KC) * (unsigned)(UH_F * 4));

#include "wino4_input.h"

    const int nch = p.Cin / KC;
    pload(0);
    lds_barrier();  // b' visible
    for (int ch = 0; ch < nch; ++ch) {
        lds_barrier();  // previous chunk's MFMAs have finished reading V / U
        __builtin_amdgcn_s_setprio(2);
        // (as wino4_body.h: the patch of this chunk is pinned as arrived in front of the LDS-DMA)
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            asm volatile("" : "+v"(pc[i].x), "+v"(pc[i].y), "+v"(pc[i].z), "+v"(pc[i].w), "+v"(pl[i]), "+v"(pr[i]));
        }
        // weight image of chunk ch: 5 pieces of 1 KiB, one per wave and the last one to wave 0
        static_assert(UH_F == 5 * 256, "5 pieces");
        const unsigned slab = (unsigned)ch * (unsigned)(UH_F * 4);
        {
            const unsigned piece = (unsigned)wave * 1024u;
            lds_dma_16B(uw, ulane, slab + piece, lu_addr + piece);
        }
        if (wave == 0) lds_dma_16B(uw, ulane, slab + 4096u, lu_addr + 4096u);
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
        lds_barrier();  // V visible, every wave's U pieces landed
        __builtin_amdgcn_s_setprio(0);
        // A stays in registers for the chunk; the B values of channel c + 1 are requested in front of the MFMAs of channel c
        f32x4 av[NXW];
        float bv[2][NXW];
        auto rdb = [&](int c) {
            const float* bp = ((c & 1) ? bfrag1 : bfrag0) + c * 64;
#pragma unroll
            for (int g = 0; g < NXW; ++g) bv[c & 1][g] = bp[g * 256];
        };
#pragma unroll
        for (int g = 0; g < NXW; ++g) av[g] = *reinterpret_cast<const f32x4*>(afrag + g * 4);
        rdb(0);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c + 1 < 4) rdb(c + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int g = 0; g < NXW; ++g) acc[g] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[g][c], bv[c & 1][g], acc[g], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // PLANES: the shortcut's logits at the 2 pixels this thread finishes (below), requested here, behind the chunk loop
    // (the patch registers are dead; in front of it they cost the 12 VGPRs the loop does not have) and in front of the output transform
    float2 lsk[NQ], lup[NQ];
    if constexpr (PLANES) {
        const int ppx = tid * 2, pmt = ppx >> 4, pms = ppx & 15;
        const size_t po = (size_t)b * NQ * HW + (size_t)(y0 + 4 * (pmt / TC) + (pms >> 2)) * p.W + (x0 + 4 * (pmt % TC) + (pms & 3));
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            lsk[q] = *reinterpret_cast<const float2*>(hs.skip + po + (size_t)q * HW);
            lup[q] = *reinterpret_cast<const float2*>(hs.up + po + (size_t)q * HW);
        }
    }
    // ---- the accumulators change hands ONCE per workgroup: a lane holds 9 of the 36 xi of (k-step, tile) for all logits, the output
    // transform wants all 36 of one (k-step, logit, tile).  Lane (kq, l15) of wave (wk, wwt) then transforms logit kq of tile
    // wwt * 16 + l15 for k-step wk (the kq = 3 lanes run along on logit 2 and store nothing) --------------------------------------
    float* xh = lds;
    float* part = lds + X_F;
    lds_barrier();  // every wave is past its last MFMA phase: U / V are dead
#pragma unroll
    for (int g = 0; g < NXW; ++g)
#pragma unroll
        for (int r = 0; r < NQ; ++r) xh[lks * XK_F + r * XQ_F + (wave * NXW + g) * 32 + l31] = acc[g][r];
    lds_barrier();
    const int ot = wwt * 16 + l15;  // this lane's tile
    const int oy = y0 + 4 * (ot / TC), ox = x0 + 4 * (ot % TC);
    {
        const float* xs = xh + wk * XK_F + min(kq, NQ - 1) * XQ_F + ot;
        float mm[NXI];
#pragma unroll
        for (int xi = 0; xi < NXI; ++xi) mm[xi] = xs[xi * 32];
        // output transform Y = A^T M A
        float tmp[4][6];
#pragma unroll
        for (int jx = 0; jx < 6; ++jx) {
            const float m[6] = {mm[0 + jx], mm[6 + jx], mm[12 + jx], mm[18 + jx], mm[24 + jx], mm[30 + jx]};
            float y[4];
            at6(m, y);
#pragma unroll
            for (int a = 0; a < 4; ++a) tmp[a][jx] = y[a];
        }
        // ---- the two waves of a tile group hold the logits of their half of the channels: left as [wk][logit][pixel = tile * 16 + s]
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float y[4];
            at6(tmp[a], y);
            if (kq < NQ) *reinterpret_cast<float4*>(part + (wk * NQ + kq) * 512 + ot * 16 + a * 4) = make_float4(y[0], y[1], y[2], y[3]);
        }
    }
    if constexpr (!PLANES) {
        // ---- the composed 1x1 shortcut over the raw block input, as wino4_body.h's: 16 MFMAs per 4 input channels, B straight
        // from global memory, on top of the transformed logits in the 16x16x4 D layout (rows 0 .. 2 = the kq = 0 lanes' registers
        // 0 .. 2 at column l15; the other rows are the zero padding of Wsc').  This wave runs k-steps [wk, wk + 1) * nks / 2 and
        // loads only those channels.
        lds_barrier();
        f32x4 ysp[16];  // [sub-pixel a * 4 + c][r]
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float4 yq[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) yq[q] = *reinterpret_cast<const float4*>(part + (wk * NQ + q) * 512 + ot * 16 + a * 4);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                ysp[a * 4 + 0][q] = kq == 0 ? yq[q].x : 0.f;
                ysp[a * 4 + 1][q] = kq == 0 ? yq[q].y : 0.f;
                ysp[a * 4 + 2][q] = kq == 0 ? yq[q].z : 0.f;
                ysp[a * 4 + 3][q] = kq == 0 ? yq[q].w : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) ysp[a * 4 + c][3] = 0.f;
        }
        const float* x2 = p.in2 + (size_t)b * p.in2_bs + (size_t)min(oy, p.H - 4) * p.W + ox;
        const float* wsc = p.w2 + l15;  // [Cin2][16]
        const int nks = p.Cin2 / 8, k0 = wk * nks;  // Cin2 % 32 == 0 (host-checked): whole groups of NSB k-steps per wave
        constexpr int NSB = 4;
        float4 xb[NSB][4];
        float wa[NSB];
        auto ldk = [&](int ks, int buf) {
            const float* xp = x2 + (size_t)(4 * ks + kq) * HW;
#pragma unroll
            for (int a = 0; a < 4; ++a) xb[buf][a] = *reinterpret_cast<const float4*>(xp + (size_t)a * p.W);
            wa[buf] = wsc[(size_t)(4 * ks + kq) * kHeadFoldRows];
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
        ldk(k0, 0);
        ldk(k0 + 1, 1);
        ldk(k0 + 2, 2);
        for (int ks = 0; ks < nks; ks += NSB) {
#pragma unroll
            for (int u = 0; u < NSB; ++u) {
                ldk(k0 + min(ks + u + 3, nks - 1), (u + 3) % NSB);  // (behind the end: the last k-step again, unused)
                __builtin_amdgcn_sched_barrier(0);
                mmk(u);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // (the kq = 0 lanes wrote and read these very addresses themselves: no barrier between the read above and this)
        if (kq == 0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int a = 0; a < 4; ++a)
                    *reinterpret_cast<float4*>(part + (wk * NQ + q) * 512 + ot * 16 + a * 4) =
                        make_float4(ysp[a * 4 + 0][q], ysp[a * 4 + 1][q], ysp[a * 4 + 2][q], ysp[a * 4 + 3][q]);
        }
    }
    // ---- then every thread finishes 2 pixels ------------------------------------------------------------------------------------
    lds_barrier();
    const int px = tid * 2;  // pixels px, px + 1: same tile, same row
    const int mt = px >> 4, ms = px & 15;
    const int my = y0 + 4 * (mt / TC) + (ms >> 2), mx = x0 + 4 * (mt % TC) + (ms & 3);
    float lg[NQ][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const float2 v0 = *reinterpret_cast<const float2*>(part + q * 512 + px);
        const float2 v1 = *reinterpret_cast<const float2*>(part + (NQ + q) * 512 + px);
        if constexpr (PLANES) {  // (k-step 0 + k-step 1) + (skip + up) + b'
            lg[q][0] = ((v0.x + v1.x) + (lsk[q].x + lup[q].x)) + lds_b[q];
            lg[q][1] = ((v0.y + v1.y) + (lsk[q].y + lup[q].y)) + lds_b[q];
        } else {
            lg[q][0] = (v0.x + v1.x) + lds_b[q];
            lg[q][1] = (v0.y + v1.y) + lds_b[q];
        }
    }
    if (my < p.mask_T) {
        mask_pixel(p, b, my, mx, lg[0][0], lg[1][0], lg[2][0]);
        mask_pixel(p, b, my, mx + 1, lg[0][1], lg[1][1], lg[2][1]);
    }
