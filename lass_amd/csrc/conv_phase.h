// conv_phase.h - one K-phase of conv.hip's implicit-GEMM kernels: staging of the input halo tile and the weight slab, and the MFMA
// contraction over a chunk.  Shared by conv.hip and tconv_logits.hip (a translation unit of its own, so that conv.hip's kernels
// compile to what they were before it existed).
#pragma once
#include <hip/hip_runtime.h>
#include "conv_common.h"

namespace {

// One K-phase: per chunk, [KC] channels x (rows+halo) x (cols+halo) of input and [KC][TAPS][NT] of weights are staged
// in LDS; the registers of chunk c+1 are loaded from global memory while chunk c is contracted.
// Input staging walks the chunk in groups of G channels (G*CH_ELEMS elements, NPASS passes of 256 threads), so the
// channel of an element is (group, u >= CH_ELEMS): wave-uniform up to one select.
template <int TAPS, int KC, int NCO, int NPX, int PW, bool PRO>
struct Phase {
    static constexpr int PH = 32 / PW;
    static constexpr int WROWS = NPX * PH;
    static constexpr int PHT = 4 * WROWS;
    static constexpr int HALO = (TAPS == 9) ? 1 : 0;
    static constexpr int IR = PHT + 2 * HALO;
    static constexpr int IP = PW + 2 * HALO;
    static constexpr int NT = 32 * NCO;
    static constexpr int CH_ELEMS = IR * IP;
    static constexpr int G = (TAPS == 9) ? 2 : 1;
    static constexpr int NGRP = KC / G;
    static constexpr int GRP_ELEMS = G * CH_ELEMS;
    static constexpr int NPASS = (GRP_ELEMS + NTHREADS - 1) / NTHREADS;
    static constexpr int IN_ELEMS = KC * CH_ELEMS;
    static constexpr int W_V4 = KC * TAPS * NT / 4;
    static constexpr int NWLD = (W_V4 + NTHREADS - 1) / NTHREADS;
    static constexpr int LDS_FLOATS = IN_ELEMS + KC * TAPS * NT;
    static_assert((IN_ELEMS % 4) == 0, "weight region must stay 16-B aligned");
    static_assert(KC % G == 0 && G <= 2, "channel grouping");

    // Every global load below is UNCONDITIONAL (addresses clamped into the image / the weight slab, the padding zero
    // applied by a select when the element is written to LDS): a conditional load makes hipcc branch around it and
    // drain vmcnt at the join, which serialises the prefetch behind a full memory round trip per chunk.
    unsigned goff[NPASS];   // clamped BYTE offset of this thread's element in pass k of group 0 (lane part of a buffer address)
    unsigned woff[NWLD];    // BYTE offset of this thread's weight float4s inside a chunk's slab
    unsigned okbits;        // bit k: the element of pass k lies inside the image (else conv zero padding)
    float v[NGRP][NPASS];   // prefetched input elements
    float4 wv[NWLD];        // prefetched weights
    float psc[KC], psh[KC]; // wave-uniform prologue scale / shift of the prefetched chunk (SGPRs)

    __device__ __forceinline__ static int upos(int tid, int k) {  // element index within a channel group (clamped:
        const int u = tid + k * NTHREADS;                        // surplus threads of the last pass duplicate the
        return u < GRP_ELEMS ? u : GRP_ELEMS - 1;                 // group's last element)
    }

    __device__ __forceinline__ void init(int tid, int y0, int x0, int H, int W) {
        okbits = 0;
#pragma unroll
        for (int k = 0; k < NPASS; ++k) {
            const int u = upos(tid, k);
            const int cl = (G == 2 && u >= CH_ELEMS) ? 1 : 0;
            const int w = u - cl * CH_ELEMS;
            const int r = w / IP, x = w % IP;
            const int gy = y0 + r - HALO, gx = x0 + x - HALO;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            const int gyc = min(max(gy, 0), H - 1), gxc = min(max(gx, 0), W - 1);
            goff[k] = 4u * (unsigned)(cl * H * W + gyc * W + gxc);
            okbits |= (ok ? 1u : 0u) << k;
        }
    }

    __device__ __forceinline__ void init_w(int tid, int Nw) {
#pragma unroll
        for (int i = 0; i < NWLD; ++i) {
            const int e0 = tid + i * NTHREADS;  // float4 index into [KC*TAPS][NT/4]
            const int e = e0 < W_V4 ? e0 : W_V4 - 1;
            const int row = e / (NT / 4), col = e % (NT / 4);
            woff[i] = 4u * (unsigned)(row * Nw + col * 4);
        }
    }
    // Buffer-addressed (descriptor + scalar byte offset + constant lane offset: no VALU address arithmetic, which the f32
    // MFMA would have to share the SIMD's VALU issue with).  in_rs: this clip's planes, c0b: byte offset of channel c0;
    // w_rs: Wt from column n0 on, wb: byte offset of row c0*TAPS.
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t in_rs, unsigned c0b, int HW, __amdgpu_buffer_rsrc_t w_rs,
                                         unsigned wb, const float* __restrict__ sc, const float* __restrict__ sh) {
#pragma unroll
        for (int q = 0; q < NGRP; ++q)
#pragma unroll
            for (int k = 0; k < NPASS; ++k)
                v[q][k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                        in_rs, (int)goff[k], (int)(c0b + (unsigned)(q * G * HW) * 4u), 0));
#pragma unroll
        for (int i = 0; i < NWLD; ++i)
            wv[i] = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(w_rs, (int)woff[i], (int)wb, 0));
        if (PRO) {
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                psc[c] = sc[c];
                psh[c] = sh[c];
            }
        }
    }

    __device__ __forceinline__ void store(float* lds, int tid) {
#pragma unroll
        for (int q = 0; q < NGRP; ++q)
#pragma unroll
            for (int k = 0; k < NPASS; ++k) {
                const int u = upos(tid, k);
                float t = v[q][k];
                if (PRO) {
                    const bool hi = (G == 2) && (u >= CH_ELEMS);
                    const float s = hi ? psc[q * G + G - 1] : psc[q * G];
                    const float h = hi ? psh[q * G + G - 1] : psh[q * G];
                    t = leaky(t * s + h);
                }
                t = ((okbits >> k) & 1u) ? t : 0.f;  // conv zero padding comes after the activation
                lds[q * GRP_ELEMS + u] = t;
            }
        float4* lw = reinterpret_cast<float4*>(lds + IN_ELEMS);
#pragma unroll
        for (int i = 0; i < NWLD; ++i) {
            const int e0 = tid + i * NTHREADS;
            lw[e0 < W_V4 ? e0 : W_V4 - 1] = wv[i];
        }
    }

    __device__ __forceinline__ static void compute(const float* lds, f32x16 (&acc)[NCO][NPX], int lane, int wave) {
        const int khalf = lane >> 5, j = lane & 31;
        const int ty = j / PW, tx = j % PW;
        const float* bbase = lds + khalf * CH_ELEMS + (wave * WROWS + ty) * IP + tx;
        const float* abase = lds + IN_ELEMS + khalf * (TAPS * NT) + j;
        constexpr int S = (KC / 2) * TAPS;  // k-steps: (channel pair, tap)
        // register double-buffered fragments: the reads of step s+1 are issued before the MFMAs of step s
        float a[2][NCO], b[2][NPX];
        auto rd = [&](int s, float (&aa)[NCO], float (&bb)[NPX]) {
            const int kk = s / TAPS, tap = s % TAPS;
#pragma unroll
            for (int co = 0; co < NCO; ++co) aa[co] = abase[(kk * 2 * TAPS + tap) * NT + co * 32];
#pragma unroll
            for (int px = 0; px < NPX; ++px)
                bb[px] = bbase[kk * 2 * CH_ELEMS + (px * PH + (TAPS == 9 ? tap / 3 : 0)) * IP +
                               (TAPS == 9 ? tap % 3 : 0)];
        };
        rd(0, a[0], b[0]);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s + 1 < S) rd(s + 1, a[(s + 1) & 1], b[(s + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ABOVE this step's MFMAs (hipcc sinks it otherwise)
#pragma unroll
            for (int co = 0; co < NCO; ++co)
#pragma unroll
                for (int px = 0; px < NPX; ++px)
                    acc[co][px] =
                        __builtin_amdgcn_mfma_f32_32x32x2f32(a[s & 1][co], b[s & 1][px], acc[co][px], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // Double-buffered variant: chunk c+1 is written into the other LDS buffer at the top of iteration c (its registers
    // were loaded one iteration earlier), chunk c+2's global loads are issued, then chunk c is contracted: ONE barrier
    // per chunk.  The chunk loop is unrolled by two so both buffer addresses are compile-time constants.
    __device__ __forceinline__ void run_db(float* lds, int buf_stride, const float* __restrict__ in_b, int Cin, int HW,
                                           const float* __restrict__ Wt, int Nw, int n0,
                                           const float* __restrict__ sc, const float* __restrict__ sh,
                                           f32x16 (&acc)[NCO][NPX], int tid, int y0, int x0, int H, int W) {
        const int lane = tid & 63, wave = tid >> 6;
        float* buf0 = lds;
        float* buf1 = lds + buf_stride;
        init(tid, y0, x0, H, W);
        init_w(tid, Nw);
        const int nchunks = Cin / KC;  // even (host-checked)
        const __amdgpu_buffer_rsrc_t in_rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b), 0, Cin * HW * 4, 0x00020000);
        const __amdgpu_buffer_rsrc_t w_rs =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(Wt + n0), 0, (Cin * TAPS * Nw - n0) * 4, 0x00020000);
        auto ld = [&](int c) {
            load(in_rs, (unsigned)(c * KC * HW) * 4u, HW, w_rs, (unsigned)(c * KC * TAPS * Nw) * 4u, sc + c * KC, sh + c * KC);
        };
        ld(0);
        __syncthreads();  // previous phase's LDS reads complete; epilogue tables visible
        store(buf0, tid);
        ld(1);
        __syncthreads();
        for (int ch = 0; ch < nchunks; ch += 2) {
            store(buf1, tid);  // chunk ch+1 (always exists)
            if (ch + 2 < nchunks) ld(ch + 2);
            compute(buf0, acc, lane, wave);
            __syncthreads();
            if (ch + 2 < nchunks) {
                store(buf0, tid);  // chunk ch+2
                if (ch + 3 < nchunks) ld(ch + 3);
            }
            compute(buf1, acc, lane, wave);
            __syncthreads();
        }
    }
};

}  // namespace
