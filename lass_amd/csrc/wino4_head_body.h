// wino4_head_body.h - the body of wino4.hip's folded-head kernels, included ONCE PER KERNEL inside the function braces (as
// wino4_body.h, and for its reason): wino4_headfold_kernel (ConvArgs alone: the composed shortcut runs here, over in2) and
// wino4_headfold_planes_kernel (ConvArgs + HeadScPlanes: the shortcut's logits arrive as two sets of planes, conv_route.h's
// head_sc_fold).  In scope: TC, PLANES, `p`, `hs`.
    constexpr bool PRO = false, PRE = false;  // conv2 reads conv1's activated output as it is
    constexpr int TR = 32 / TC;
    constexpr int OR_ = 4 * TR, OC = 4 * TC;
    constexpr int UH_F = kHeadFoldUFloats;      // 18 KiB: [xi pair][k-step][kq][row 16][xi & 1]
    constexpr int NQ = 3;                       // logits
    __shared__ __attribute__((aligned(16))) float lds[UH_F + V_F + kHeadFoldRows];
    float* lu = lds;
    float* lv = lds + UH_F;
    float* lds_b = lv + V_F;  // b'

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave >> 1, wwt = wave & 1;  // k-step of a chunk (and half of the shortcut's channels) / tile group of this wave
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);  // (gy = 1)
    const int tiles_x = p.W / OC;
    const int y0 = (bx_ / tiles_x) * OR_, x0 = (bx_ % tiles_x) * OC;
    const int HW = p.H * p.W;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = nullptr;
    const float* sh = nullptr;
    if (tid < kHeadFoldRows) lds_b[tid] = p.bias[tid];

    f32x4 acc[NXI];
#pragma unroll
    for (int xi = 0; xi < NXI; ++xi)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[xi][r] = 0.f;

    const int kq = lane >> 4, l15 = lane & 15;
    // fragments of this wave's k-step: A = {xi, xi + 1}[row l15][channel kq] in one 8-byte read; B = V[xi][kq][tile ^ swz][wk]
    const float* afrag = lu + (wk * 64 + kq * 16 + l15) * 2;
    const float* bfrag = lv + (kq * 32 + ((wwt * 16 + l15) ^ ((kq & 1) << 4))) * 2 + wk;
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
        // weight image of chunk ch: 18 pieces of 1 KiB, 4 per wave and the last two to waves 0 and 1
        static_assert(UH_F == 18 * 256, "18 pieces");
        const unsigned slab = (unsigned)ch * (unsigned)(UH_F * 4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const unsigned piece = (unsigned)(wave * 4 + i) * 1024u;
            lds_dma_16B(uw, ulane, slab + piece, lu_addr + piece);
        }
        if (wave < 2) {
            const unsigned piece = (unsigned)(16 + wave) * 1024u;
            lds_dma_16B(uw, ulane, slab + piece, lu_addr + piece);
        }
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
        // 36 GEMM steps of ONE k-step: every MFMA has an accumulator of its own
        constexpr int PFD = 3;  // pairs of fragment reads ahead
        f32x2v av[PFD + 1];
        float bv[PFD + 1][2];
        auto rd = [&](int s) {  // step s = xi pair (2s, 2s+1)
            av[s % (PFD + 1)] = *reinterpret_cast<const f32x2v*>(afrag + s * 256);
#pragma unroll
            for (int q = 0; q < 2; ++q) bv[s % (PFD + 1)][q] = bfrag[(2 * s + q) * 256];
        };
#pragma unroll
        for (int s = 0; s < PFD; ++s) rd(s);
#pragma unroll
        for (int s = 0; s < NXI / 2; ++s) {
            if (s + PFD < NXI / 2) rd(s + PFD);
            __builtin_amdgcn_sched_barrier(0);
            const f32x2v a = av[s % (PFD + 1)];
            acc[2 * s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bv[s % (PFD + 1)][0], acc[2 * s], 0, 0, 0);
            acc[2 * s + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bv[s % (PFD + 1)][1], acc[2 * s + 1], 0, 0, 0);
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
    // ---- output transform Y = A^T M A of D rows kq * 4 + r, r < 3: the logits are rows 0 .. 2 (the kq = 0 lanes); the other
    // rows of the tile are the zero padding of the images -----------------------------------------------------------------
    const int ot = wwt * 16 + l15;  // this lane's tile
    const int oy = y0 + 4 * (ot / TC), ox = x0 + 4 * (ot % TC);
    f32x4 ysp[16];  // [sub-pixel a * 4 + c][r]
#pragma unroll
    for (int s = 0; s < 16; ++s) ysp[s][3] = 0.f;
#pragma unroll
    for (int r = 0; r < NQ; ++r) {
        float tmp[4][6];
#pragma unroll
        for (int jx = 0; jx < 6; ++jx) {
            const float m[6] = {acc[0 + jx][r], acc[6 + jx][r], acc[12 + jx][r], acc[18 + jx][r], acc[24 + jx][r], acc[30 + jx][r]};
            float y[4];
            at6(m, y);
#pragma unroll
            for (int a = 0; a < 4; ++a) tmp[a][jx] = y[a];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            float y[4];
            at6(tmp[a], y);
#pragma unroll
            for (int c = 0; c < 4; ++c) ysp[a * 4 + c][r] = y[c];
        }
    }
    if constexpr (!PLANES) {
        // ---- the composed 1x1 shortcut over the raw block input, as wino4_body.h's: 16 MFMAs per 4 input channels, B straight
        // from global memory.  This wave runs k-steps [wk, wk + 1) * nks / 2 and loads only those channels.
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
    }
    // ---- the two waves of a tile group hold the logits of their half of the channels, 3 x 16 pixels per kq = 0 lane: left in the
    // dead U / V region as [wk][logit][pixel = tile * 16 + s] (2 x 3 x 512 floats), then every thread finishes 2 pixels ----------
    float* part = lds;
    lds_barrier();  // every wave is past its last MFMA phase
    if (kq == 0) {
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int a = 0; a < 4; ++a)
                *reinterpret_cast<float4*>(part + (wk * NQ + q) * 512 + ot * 16 + a * 4) =
                    make_float4(ysp[a * 4 + 0][q], ysp[a * 4 + 1][q], ysp[a * 4 + 2][q], ysp[a * 4 + 3][q]);
    }
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
