// wino.hip - Winograd F(2x2,3x3) 3x3 convolutions on the gfx950 f32 MFMA.
//
// Same reference semantics as conv.hip (models/resunet.py:147-165): a 3x3/stride-1/pad-1 cross-correlation, with the
// BN+FiLM+leaky prologue, epilogue activation, residual / 1x1-shortcut(+bias) and avg-pool fusions.  Only the
// contraction changes: every 2x2 output tile is computed from its 4x4 input patch through
//      Y = A^T [ sum_c (G g_c G^T) .* (B^T d_c B) ] A                                   (Lavin & Gray 2016)
// i.e. 16 independent GEMMs  M_xi[cout][tile] = sum_cin U_xi[cout][cin] * V_xi[cin][tile]  with 4 multiplies per output
// pixel and (cin,cout) pair instead of 9: 2.25x fewer MFMA FLOPs, all of them still plain f32 FMAs.
//
// Mapping: v_mfma_f32_16x16x4_f32; a wave owns 32 couts x 16 Winograd tiles (one row pair of 32 pixels) and keeps all
// 16 xi accumulators (16 xi x 2 cout-tiles x 4 regs = 128 AGPRs), so the output transform is register-local:
// D row = (lane>>4)*4 + reg -> cout, D col = lane&15 -> tile.  Per chunk of 8 input channels a workgroup (4 waves)
//   1. stages the activated halo tile [8][rows+2][34] (same unconditional-load staging as conv.hip),
//   2. transforms it to V[16][8][tiles] in LDS (32 add/sub per 4x4 patch),
//   3. stages U[16][8][NT] (weights pre-transformed once in lass_finalize),
//   4. runs 16 xi x 2 k-steps x 2 cout-tiles MFMAs per wave.
// The 1x1 shortcut is the same kernel family in the transform domain: a centre-only 3x3 kernel has G g G^T non-zero
// at the four xi in {1,2}x{1,2} only, and its B^T d B there needs just the 2x2 centre of the patch.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "kernels.h"
#include "pixel_ops.h"
#include "wino_common.h"
#include "wino_epilogue.h"

namespace {

constexpr int F_PRO = 1, F_PHASEB = 2, F_BIAS = 4, F_RES = 8, F_EPIACT = 16;
constexpr int F_MASK = 1024;    // epilogue = after_conv + complex ratio mask (ConvArgs::mask_*); the block output is not written
constexpr int F_PRECONV = 64;   // input is the 1-channel x0; channel c = pre_w[c]*x0 + pre_b[c] is formed while staging
constexpr int F_RESPRE = 128;   // with F_RES: the residual is pre_w[n]*x0 + pre_b[n]
constexpr int NTHREADS = 256;
constexpr int KC = kWinoKC;
constexpr int KCB = 32;  // shortcut phase: 32 channels x 4 xi per chunk (the same 128 LDS rows and 64 MFMAs as a 3x3 chunk)

// Wave priority by phase.  A wave's staging / transform chain (a few dozen VALU and LDS instructions strung between
// barriers) is longer than its MFMA phase, and its VALU instructions queue behind the SIMD partner's back-to-back f32
// MFMAs (which occupy the vector issue port): the preparing wave is the critical path, so it gets the higher priority.
__device__ __forceinline__ void prep_prio() { __builtin_amdgcn_s_setprio(2); }
__device__ __forceinline__ void mfma_prio() { __builtin_amdgcn_s_setprio(0); }

// Halo-tile staging: [KC][IR][IP] raw (activated) input, walked in channel pairs (see conv.hip Phase).
template <int IR, int IP, int HALO, int KCH, bool PRO, bool PRE = false, int NTH = NTHREADS>
struct RawStage {
    static constexpr int CH_ELEMS = IR * IP;
    static constexpr int G = 2;
    static constexpr int NGRP = KCH / G;
    static constexpr int GRP_ELEMS = G * CH_ELEMS;
    static constexpr int NPASS = (GRP_ELEMS + NTH - 1) / NTH;
    unsigned goff[NPASS];  // BYTE offset of this thread's element from the chunk's first channel (uniform base + 32-bit lane offset -> saddr loads)
    unsigned okbits;
    float v[PRE ? 1 : 2][PRE ? 1 : NGRP][NPASS];  // two chunks in flight (PRE: x0 at this thread's positions, loaded once)

    __device__ __forceinline__ static int upos(int tid, int k) {
        const int u = tid + k * NTH;
        return u < GRP_ELEMS ? u : GRP_ELEMS - 1;
    }
    __device__ __forceinline__ void init(int tid, int y0, int x0, int H, int W) {
        okbits = 0;
#pragma unroll
        for (int k = 0; k < NPASS; ++k) {
            const int u = upos(tid, k);
            const int cl = u >= CH_ELEMS ? 1 : 0;
            const int w = u - cl * CH_ELEMS;
            const int r = w / IP, x = w % IP;
            const int gy = y0 + r - HALO, gx = x0 + x - HALO;
            const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
            goff[k] = 4u * (unsigned)(cl * H * W + min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1));
            okbits |= (ok ? 1u : 0u) << k;
        }
    }
    static constexpr int NLOADS = NGRP * NPASS;  // vector-memory loads load() issues (counted by the vmcnt waits)
    // rsrc: buffer descriptor of this batch item's input planes; c0_bytes: byte offset of the chunk's first channel.
    // buffer_load with a scalar offset + constant 32-bit lane offset: no VALU address arithmetic per load.
    template <int BUF>
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rsrc, unsigned c0_bytes, int HW) {
        if (PRE) return;  // nothing per chunk: every channel is an affine function of the one x0 plane
#pragma unroll
        for (int q = 0; q < NGRP; ++q)
#pragma unroll
            for (int k = 0; k < NPASS; ++k)
                v[BUF][q][k] = __builtin_bit_cast(
                    float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)goff[k], (int)(c0_bytes + (unsigned)(q * G * HW) * 4u), 0));
    }
    __device__ __forceinline__ void load_x0(const float* __restrict__ x0_b, int HW) {  // PRE only
#pragma unroll
        for (int k = 0; k < NPASS; ++k) {
            const unsigned e = goff[k] / 4u;
            v[0][0][k] = x0_b[e >= (unsigned)HW ? e - HW : e];
        }
    }
    // lsc / lsh: the prologue scale / shift of this chunk's channels in LDS (staged once per workgroup); all table reads
    // are issued up front (uniform b128 reads) so the element loop below has no LDS read behind an LDS write.
    // PRE: lpw / lpb = pre_conv weight / bias of this chunk's channels (LDS), else unused
    template <int BUF>
    __device__ __forceinline__ void store(float* lds, const float* lsc, const float* lsh, int tid,
                                          const float* lpw = nullptr, const float* lpb = nullptr) {
        float tsc[KCH], tsh[KCH], tpw[KCH], tpb[KCH];
        if (PRE) {
#pragma unroll
            for (int c = 0; c < KCH; c += 4) {
                const float4 a = *reinterpret_cast<const float4*>(lpw + c);
                const float4 b = *reinterpret_cast<const float4*>(lpb + c);
                tpw[c] = a.x; tpw[c + 1] = a.y; tpw[c + 2] = a.z; tpw[c + 3] = a.w;
                tpb[c] = b.x; tpb[c + 1] = b.y; tpb[c + 2] = b.z; tpb[c + 3] = b.w;
            }
        }
        if (PRO) {
#pragma unroll
            for (int c = 0; c < KCH; c += 4) {
                const float4 a = *reinterpret_cast<const float4*>(lsc + c);
                const float4 b = *reinterpret_cast<const float4*>(lsh + c);
                tsc[c] = a.x; tsc[c + 1] = a.y; tsc[c + 2] = a.z; tsc[c + 3] = a.w;
                tsh[c] = b.x; tsh[c + 1] = b.y; tsh[c + 2] = b.z; tsh[c + 3] = b.w;
            }
        }
#pragma unroll
        for (int q = 0; q < NGRP; ++q)
#pragma unroll
            for (int k = 0; k < NPASS; ++k) {
                const int u = upos(tid, k);
                float t = PRE ? 0.f : v[PRE ? 0 : BUF][PRE ? 0 : q][k];
                if (PRE) {
                    const bool hi0 = u >= CH_ELEMS;
                    t = v[0][0][k] * (hi0 ? tpw[q * G + 1] : tpw[q * G]) + (hi0 ? tpb[q * G + 1] : tpb[q * G]);
                }
                if (PRO) {
                    const bool hi = u >= CH_ELEMS;
                    t = leaky(t * (hi ? tsc[q * G + 1] : tsc[q * G]) + (hi ? tsh[q * G + 1] : tsh[q * G]));
                }
                t = ((okbits >> k) & 1u) ? t : 0.f;
                lds[q * GRP_ELEMS + u] = t;
            }
    }
};

// Weight-slab staging by LDS-DMA (buffer_load ... lds, 16 B per lane, no VGPRs).  The transform-domain weights are stored
// in global memory as the exact LDS image of a (chunk, 32-cout group) slab (wino_weights_kernel): 16 rows-of-xi x 4 kq x
// 16 couts x {(k0,t0),(k0,t1),(k1,t0),(k1,t1)} = 16 KiB, so that a lane's A fragment for a whole xi step is one aligned
// 16-byte word and the DMA is a plain linear copy: piece i of the workgroup's slab (WCO adjacent groups) goes from
// slab + 1 KiB * i to lu + 1 KiB * i.
template <int WCO, int NW = 4>
struct UDma {
    static constexpr int NINSTR = 16 * WCO / NW;  // wave-instructions per wave (16 * WCO pieces over NW waves)
    static constexpr int SLAB_BYTES = 16384 * WCO;
    // slab_byte0: byte offset of this chunk's slab in the weight buffer (wave-uniform)
    __device__ __forceinline__ static void issue(v4i32 rsrc, unsigned lane_off, unsigned slab_byte0, unsigned lds_base,
                                                 int wave) {
#pragma unroll
        for (int i = 0; i < NINSTR; ++i) {
            const unsigned piece = (unsigned)(wave * NINSTR + i) * 1024u;  // wave-uniform
            lds_dma_16B(rsrc, lane_off, slab_byte0 + piece, lds_base + piece);
        }
    }
};

// WCO x WWT waves (product 4): block = 32*WCO couts x 16*WWT Winograd tiles, PWT of them per row pair: the block covers
// 2*PWT output columns x 2*(16*WWT/PWT) output rows (PWT = 16: 32 columns; 8 / 4: the 16- and 8-bin layers at the bottom
// of the U-Net, whose 32-tile blocks are folded into more rows).
// PATCH: every thread loads its 4x4 input patch(es) straight from global (two 8-byte loads per patch row, two chunks
// ahead), applies the prologue and the zero padding and transforms in registers - no raw LDS tile, two barriers per chunk
// instead of three (the barrier -> LDS -> transform -> LDS -> barrier latency chain is what the chunk time is made of).
template <int WCO, int WWT, int FLAGS, int PWT = 16, bool PATCH = false>
__global__ __launch_bounds__(NTHREADS, 2) void wino_kernel(ConvArgs p) {
    static_assert(WCO * WWT == 4, "4 waves");
    constexpr bool PRO = (FLAGS & F_PRO) != 0;
    constexpr bool HASB = (FLAGS & F_PHASEB) != 0;
    constexpr bool EPI = (FLAGS & F_EPIACT) != 0;
    constexpr bool BIAS = (FLAGS & F_BIAS) != 0;
    constexpr bool RES = (FLAGS & F_RES) != 0;
    constexpr bool PRE = (FLAGS & F_PRECONV) != 0;
    constexpr bool RESPRE = (FLAGS & F_RESPRE) != 0;
    constexpr int NT = 32 * WCO;
    constexpr int NWT = 16 * WWT;
    constexpr int OR_ = 2 * (NWT / PWT), OC = 2 * PWT;  // output rows / cols of the block
    constexpr int IR = OR_ + 2, IP = OC + 2;
    // V image: 64 rows (xi, kq) of NWT tiles x {k-step 0, k-step 1}; the row pitch is = 128 B mod 256 B so that the two
    // kq rows a 32-lane group reads with one ds_read_b64 fall into different halves of the 64 banks
    constexpr int VP = 2 * NWT + 32;
    using RA = RawStage<IR, IP, 1, KC, PRO, PRE>;
    using UA = UDma<WCO>;
    constexpr int RAW_F = PATCH ? 0 : KC * IR * IP;
    constexpr int V_F = 64 * VP;
    constexpr int U_F = 16 * KC * NT;
    constexpr int MAXC = 768;  // largest Cin of a 3x3 conv in the network (decoder_block1/2.conv1)
    constexpr bool MASK = (FLAGS & F_MASK) != 0;
    static_assert(!MASK || WCO == 1, "the fused output head needs all 32 channels in one wave");
    constexpr int NTAB = (EPI ? 2 * NT : 0) + (BIAS ? NT : 0) + (PRO ? 2 * MAXC : 0) + ((PRE || RESPRE) ? 64 : 0) + (MASK ? 100 : 0);
    static_assert(RAW_F % 4 == 0 && V_F % 4 == 0, "16-B alignment of the LDS regions");

    __shared__ __attribute__((aligned(16))) float lds[RAW_F + V_F + U_F + NTAB];
    float* lraw = lds;
    float* lv = lds + RAW_F;
    float* lu = lv + V_F;
    float* lds_es = lu + U_F;
    float* lds_eh = lds_es + NT;
    float* lds_bias = lu + U_F + (EPI ? 2 * NT : 0);
    float* lds_sc = lu + U_F + (EPI ? 2 * NT : 0) + (BIAS ? NT : 0);  // PRO: scale / shift of every input channel
    float* lds_sh = lds_sc + MAXC;
    float* lds_pw = lu + U_F + (EPI ? 2 * NT : 0) + (BIAS ? NT : 0) + (PRO ? 2 * MAXC : 0);  // pre_conv weight / bias (32+32)
    float* lds_pb = lds_pw + 32;
    float* lds_mw = lds + RAW_F + V_F + U_F + NTAB - 100;  // MASK: after_conv weight [3][32] + bias [3]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // uniform to the compiler too
    const int wco = wave / WWT, wwt = wave % WWT;
    int bx_, by_, b;
    block_coords(p, bx_, by_, b);
    const int n0 = by_ * NT;
    const int tiles_x = p.W / OC;
    const int y0 = (bx_ / tiles_x) * OR_, x0 = (bx_ % tiles_x) * OC;
    const int HW = p.H * p.W;
    const float* in_b = p.in + (size_t)b * p.in_bs;
    const float* sc = PRO ? p.pro_scale : nullptr;
    const float* sh = PRO ? p.pro_shift + (size_t)b * p.pro_shift_bs : nullptr;

    if (EPI && tid < NT) {
        lds_es[tid] = p.epi_scale[n0 + tid];
        lds_eh[tid] = p.epi_shift[(size_t)b * p.epi_shift_bs + n0 + tid];
    }
    if (BIAS && tid < NT) lds_bias[tid] = p.bias[n0 + tid];
    if (PRO) {
        for (int c = tid; c < p.Cin; c += NTHREADS) {
            lds_sc[c] = sc[c];
            lds_sh[c] = sh[c];
        }
    }
    if ((PRE || RESPRE) && tid < 32) {
        lds_pw[tid] = p.pre_w[tid];
        lds_pb[tid] = p.pre_b[tid];
    }
    if (MASK && tid < 99) lds_mw[tid] = tid < 96 ? p.mask_w[tid] : p.mask_b[tid - 96];

    f32x4 acc[16][2];
#pragma unroll
    for (int xi = 0; xi < 16; ++xi)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[xi][t][r] = 0.f;

    const int kq = lane >> 4, l15 = lane & 15;
    const float* bfrag = lv + kq * VP + (wwt * 16 + l15) * 2;   // row (xi, kq), this lane's tile: {k-step 0, k-step 1}
    const float* afrag = lu + wco * 4096 + kq * 64 + l15 * 4;   // group wco, row (xi, kq), this lane's cout: 4 floats
    const unsigned slab_pitch = (unsigned)(p.Nw / 32) * 16384u;  // bytes between the slabs of consecutive chunks
    const unsigned slab_n0 = (unsigned)(n0 / 32) * 16384u;

    // ---- main phase: 3x3 over p.in ------------------------------------------------------------------------------
    // Per chunk:  barrier | raw(ch) regs->LDS | issue U(ch) LDS-DMA | issue raw(ch+2) loads | barrier |
    //             transform raw->V | wait U(ch) (counted vmcnt: the raw(ch+2) loads stay in flight) | barrier |
    //             MFMAs
    const unsigned lu_addr = (unsigned)(size_t)(__attribute__((address_space(3))) float*)lu;
    if constexpr (PATCH) {
        constexpr int CSTEP = NTHREADS / NWT;  // a thread owns ONE tile position and channels cb + i*CSTEP of the chunk
        constexpr int NIT = KC / CSTEP;        // patches per thread and chunk
        typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));
        const int wt = tid % NWT, cb = tid / NWT;
        const int pty = wt / PWT, ptx = wt % PWT;
        const int gy0 = y0 + 2 * pty - 1, gx0 = x0 + 2 * ptx - 1;
        const bool left = gx0 < 0, right = gx0 + 3 >= p.W;
        unsigned voa[4], vob[4], rowok = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gy = gy0 + i;
            const int row = min(max(gy, 0), p.H - 1) * p.W + (PRE ? 0 : cb * HW);
            voa[i] = 4u * (unsigned)(row + (left ? 0 : gx0));            // pair (gx0, gx0+1); at the left edge (0, 1)
            vob[i] = 4u * (unsigned)(row + (right ? p.W - 2 : gx0 + 2));  // pair (gx0+2, gx0+3); right edge (W-2, W-1)
            rowok |= (gy >= 0 && gy < p.H ? 1u : 0u) << i;
        }
        const __amdgpu_buffer_rsrc_t in_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b), 0, (int)((unsigned)(PRE ? 1 : p.Cin) * (unsigned)HW * 4u), 0x00020000);
        f2u ps[PRE ? 1 : 2][NIT][8];
        auto pload = [&](int ch, auto buf) {
            constexpr int BUF = decltype(buf)::value;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const unsigned soff = PRE ? 0u : (unsigned)((ch * KC + it * CSTEP) * HW) * 4u;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // (PRE: one patch set, loaded once - the BUF = 1 instantiation is never called but is compiled)
                    ps[PRE ? 0 : BUF][it][2 * i] = __builtin_bit_cast(f2u, __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, (int)voa[i], (int)soff, 0));
                    ps[PRE ? 0 : BUF][it][2 * i + 1] = __builtin_bit_cast(f2u, __builtin_amdgcn_raw_buffer_load_b64(in_rsrc, (int)vob[i], (int)soff, 0));
                }
            }
        };
        auto pprocess = [&](int ch, auto buf) {
            constexpr int BUF = decltype(buf)::value;
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = ch * KC + cb + it * CSTEP;
                const float s1 = PRO ? lds_sc[c] : 0.f, s2 = PRO ? lds_sh[c] : 0.f;
                const float pw = PRE ? lds_pw[c] : 0.f, pb = PRE ? lds_pb[c] : 0.f;
                float d[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f2u a = ps[PRE ? 0 : BUF][PRE ? 0 : it][2 * i], bq = ps[PRE ? 0 : BUF][PRE ? 0 : it][2 * i + 1];
                    float v0 = a.x, v1 = left ? a.x : a.y, v2 = right ? bq.y : bq.x, v3 = bq.y;
                    if (PRE) { v0 = v0 * pw + pb; v1 = v1 * pw + pb; v2 = v2 * pw + pb; v3 = v3 * pw + pb; }
                    if (PRO) {
                        v0 = leaky(v0 * s1 + s2); v1 = leaky(v1 * s1 + s2);
                        v2 = leaky(v2 * s1 + s2); v3 = leaky(v3 * s1 + s2);
                    }
                    const bool rok = ((rowok >> i) & 1u) != 0;  // zero padding comes AFTER the activation
                    d[i][0] = (rok && !left) ? v0 : 0.f;
                    d[i][1] = rok ? v1 : 0.f;
                    d[i][2] = rok ? v2 : 0.f;
                    d[i][3] = (rok && !right) ? v3 : 0.f;
                }
                float tt[4][4];
#pragma unroll
                for (int jx = 0; jx < 4; ++jx) {
                    tt[0][jx] = d[0][jx] - d[2][jx];
                    tt[1][jx] = d[1][jx] + d[2][jx];
                    tt[2][jx] = d[2][jx] - d[1][jx];
                    tt[3][jx] = d[1][jx] - d[3][jx];
                }
                const int cl = cb + it * CSTEP;  // channel within the chunk: k-step cl / 4, row kq = cl % 4
                float* dst = lv + (cl & 3) * VP + wt * 2 + (cl >> 2);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dst[(4 * i + 0) * (4 * VP)] = tt[i][0] - tt[i][2];
                    dst[(4 * i + 1) * (4 * VP)] = tt[i][1] + tt[i][2];
                    dst[(4 * i + 2) * (4 * VP)] = tt[i][2] - tt[i][1];
                    dst[(4 * i + 3) * (4 * VP)] = tt[i][1] - tt[i][3];
                }
            }
        };
        const int nch = p.Cin / KC;  // even (host-checked)
        pload(0, std::integral_constant<int, 0>{});
        if (!PRE) pload(1, std::integral_constant<int, 1>{});
        const unsigned ulane = (unsigned)lane * 16u;
        const v4i32 uw_n0 = make_rsrc_words(p.w_wino, (unsigned)(16 * p.Cin * p.Nw) * 4u);
        lds_barrier();  // prologue tables visible
        auto chunk = [&](int ch, auto buf) {
            constexpr int BUF = decltype(buf)::value;
            lds_barrier();  // previous chunk's MFMAs have finished reading V / U
            prep_prio();
            pprocess(ch, buf);
            __builtin_amdgcn_sched_barrier(0);
            UA::issue(uw_n0, ulane, (unsigned)ch * slab_pitch + slab_n0, lu_addr, wave);
            __builtin_amdgcn_sched_barrier(0);
            const bool pf = !PRE && ch + 2 < nch;
            if (pf) pload(ch + 2, buf);
            __builtin_amdgcn_sched_barrier(0);
            if (pf)
                wait_vmcnt<NIT * 8>();  // this wave's U(ch) rows have landed; the patches of chunk ch+2 stay in flight
            else
                wait_vmcnt<0>();
            lds_barrier();  // V visible, every wave's U rows landed
            mfma_prio();
            gemm_steps<16, 256, 4 * VP>(afrag, bfrag, acc, [](int s) { return s; });
        };
        for (int ch = 0; ch < nch; ch += 2) {
            chunk(ch, std::integral_constant<int, 0>{});
            chunk(ch + 1, std::integral_constant<int, 1>{});
        }
    } else {
        RA ra;
        ra.init(tid, y0, x0, p.H, p.W);
        const int nch = p.Cin / KC;  // even (host-checked)
        if (PRE) ra.load_x0(in_b, HW);
        const __amdgpu_buffer_rsrc_t in_rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in_b), 0, (int)((unsigned)(PRE ? 1 : p.Cin) * (unsigned)HW * 4u), 0x00020000);
        ra.template load<0>(in_rsrc, 0u, HW);
        ra.template load<1>(in_rsrc, (unsigned)(KC * HW) * 4u, HW);
        const unsigned ulane = (unsigned)lane * 16u;
        const v4i32 uw_n0 = make_rsrc_words(p.w_wino, (unsigned)(16 * p.Cin * p.Nw) * 4u);
        lds_barrier();  // prologue tables visible
        auto chunk = [&](int ch, auto buf) {
            constexpr int BUF = decltype(buf)::value;
            lds_barrier();  // previous chunk's MFMAs have finished reading V / U
            prep_prio();
            ra.template store<BUF>(lraw, lds_sc + ch * KC, lds_sh + ch * KC, tid, lds_pw + ch * KC, lds_pb + ch * KC);
            __builtin_amdgcn_sched_barrier(0);
            UA::issue(uw_n0, ulane, (unsigned)ch * slab_pitch + slab_n0, lu_addr, wave);
            __builtin_amdgcn_sched_barrier(0);
            const bool pf = ch + 2 < nch;
            if (pf) ra.template load<BUF>(in_rsrc, (unsigned)((ch + 2) * KC * HW) * 4u, HW);
            __builtin_amdgcn_sched_barrier(0);
            lds_barrier();  // raw tile visible
            // input transform V = B^T d B: one (channel, tile) item per thread and pass
#pragma unroll
            for (int it = 0; it < (KC * NWT) / NTHREADS; ++it) {
                const int item = tid + it * NTHREADS;
                const int c = item / NWT, wt = item % NWT;
                const int wty = wt / PWT, wtx = wt % PWT;
                const float* src = lraw + c * (IR * IP) + (2 * wty) * IP + 2 * wtx;
                float d[4][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float2 lo = *reinterpret_cast<const float2*>(src + i * IP);
                    const float2 hi = *reinterpret_cast<const float2*>(src + i * IP + 2);
                    d[i][0] = lo.x; d[i][1] = lo.y; d[i][2] = hi.x; d[i][3] = hi.y;
                }
                float tt[4][4];
#pragma unroll
                for (int jx = 0; jx < 4; ++jx) {
                    tt[0][jx] = d[0][jx] - d[2][jx];
                    tt[1][jx] = d[1][jx] + d[2][jx];
                    tt[2][jx] = d[2][jx] - d[1][jx];
                    tt[3][jx] = d[1][jx] - d[3][jx];
                }
                float* dst = lv + (c & 3) * VP + wt * 2 + (c >> 2);  // row kq = c % 4, k-step c / 4
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    dst[(4 * i + 0) * (4 * VP)] = tt[i][0] - tt[i][2];
                    dst[(4 * i + 1) * (4 * VP)] = tt[i][1] + tt[i][2];
                    dst[(4 * i + 2) * (4 * VP)] = tt[i][2] - tt[i][1];
                    dst[(4 * i + 3) * (4 * VP)] = tt[i][1] - tt[i][3];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            if (pf && !PRE)
                wait_vmcnt<RA::NLOADS>();  // this wave's U(ch) rows have landed; raw(ch+2) may still be in flight
            else
                wait_vmcnt<0>();
            lds_barrier();  // V visible, every wave's U rows landed
            // 16 GEMMs: M_xi += U_xi (32 couts x 8 cin) * V_xi (8 cin x 16 tiles)
            mfma_prio();
            gemm_steps<16, 256, 4 * VP>(afrag, bfrag, acc, [](int s) { return s; });
        };
        for (int ch = 0; ch < nch; ch += 2) {
            chunk(ch, std::integral_constant<int, 0>{});
            chunk(ch + 1, std::integral_constant<int, 1>{});
        }
    }
    // ---- shortcut phase: 1x1 over p.in2, in the transform domain (xi in {5,6,9,10}) -------------------------------
    // Chunks of 32 channels: a thread owns one tile position and channels cb + i*CSTEP; it loads the 2x2 patch centres
    // straight from global (two aligned 8-byte loads per item, issued one chunk ahead: they land during the MFMAs) and
    // writes B^T d B to V - no raw tile, two barriers per 64 MFMAs.
    if (HASB) {
        constexpr int CSTEP = NTHREADS / NWT;
        constexpr int NITB = KCB / CSTEP;
        const int wt = tid % NWT, cb = tid / NWT;
        const int wty = wt / PWT, wtx = wt % PWT;
        const int oy = y0 + 2 * wty, ox = x0 + 2 * wtx;
        const bool okB = oy + 1 < p.H;
        const __amdgpu_buffer_rsrc_t in2_rsrc = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<float*>(p.in2 + (size_t)b * p.in2_bs), 0, (int)((unsigned)p.Cin2 * (unsigned)HW * 4u), 0x00020000);
        const unsigned voff1 = (unsigned)(cb * HW + min(oy, p.H - 2) * p.W + ox) * 4u, voff2 = voff1 + (unsigned)p.W * 4u;
        float2 rb[2 * NITB];
        auto loadB = [&](int ch) {
#pragma unroll
            for (int it = 0; it < NITB; ++it) {
                const unsigned soff = (unsigned)((ch * KCB + it * CSTEP) * HW) * 4u;
                rb[2 * it] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(in2_rsrc, (int)voff1, (int)soff, 0));
                rb[2 * it + 1] = __builtin_bit_cast(float2, __builtin_amdgcn_raw_buffer_load_b64(in2_rsrc, (int)voff2, (int)soff, 0));
            }
        };
        const int nch = p.Cin2 / KCB;
        loadB(0);
        const unsigned ulane = (unsigned)lane * 16u;
        const v4i32 uw_n0 = make_rsrc_words(p.w2_wino, (unsigned)(4 * p.Cin2 * p.Nw) * 4u);
        for (int ch = 0; ch < nch; ++ch) {
            lds_barrier();  // previous chunk's MFMAs have finished reading V / U
            prep_prio();
#pragma unroll
            for (int it = 0; it < NITB; ++it) {
                float2 r1 = rb[2 * it], r2 = rb[2 * it + 1];  // patch rows 1,2 x cols 1,2
                if (!okB) { r1 = make_float2(0.f, 0.f); r2 = r1; }
                const float t1a = r1.x + r2.x, t1b = r1.y + r2.y;  // tt[1][1], tt[1][2]
                const float t2a = r2.x - r1.x, t2b = r2.y - r1.y;  // tt[2][1], tt[2][2]
                // channel cl of the 32-chunk: 8-channel pair-step cl / 8, k-step (cl % 8) / 4, row kq = cl % 4; the image
                // rows are (xi slot, pair-step, kq): one xi slot = 16 rows
                const int cl = cb + it * CSTEP;
                float* dst = lv + ((cl >> 3) * 4 + (cl & 3)) * VP + wt * 2 + ((cl >> 2) & 1);
                dst[0 * (16 * VP)] = t1a + t1b;  // V[1][1]
                dst[1 * (16 * VP)] = t1b - t1a;  // V[1][2]
                dst[2 * (16 * VP)] = t2a + t2b;  // V[2][1]
                dst[3 * (16 * VP)] = t2b - t2a;  // V[2][2]
            }
            __builtin_amdgcn_sched_barrier(0);
            UA::issue(uw_n0, ulane, (unsigned)ch * slab_pitch + slab_n0, lu_addr, wave);
            __builtin_amdgcn_sched_barrier(0);
            const bool pf = ch + 1 < nch;
            if (pf) loadB(ch + 1);
            __builtin_amdgcn_sched_barrier(0);
            if (pf)
                wait_vmcnt<2 * NITB>();  // this wave's U rows have landed; the centre loads of chunk ch+1 stay in flight
            else
                wait_vmcnt<0>();
            lds_barrier();  // V visible, every wave's U rows landed
            mfma_prio();
            gemm_steps<16, 256, 4 * VP>(afrag, bfrag, acc, [](int s) {
                const int q = s / 4;                // 4 pair-steps (32 channels) per xi slot
                return (q >> 1) * 4 + (q & 1) + 5;  // 5, 6, 9, 10
            });
        }
    }

    // ---- output transform Y = A^T M A and epilogue (wino_epilogue.h) ---------------------------------------------------
    {
        const int wty = (wwt * 16 + l15) / PWT, wtx = (wwt * 16 + l15) % PWT;  // this lane's tile within the block
        wino_epilogue<FLAGS>(p, acc, b, n0, wco * 32, y0 + 2 * wty, x0 + 2 * wtx, lane, lds_bias, lds_es, lds_eh, lds_pw, lds_pb,
                             lds_mw);
    }
}

// Transform-domain weights U_xi[cin][cout] = (G g G^T)[xi] for g = w[cout][cin][3][3], G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],
// [0,0,1]], stored as the LDS images the kernel DMAs (see UDma): slab (chunk = cin / 8, group = cout / 32) of 4096 floats,
// element [xi][kq = cin % 4][l15 = cout % 16][j = 2 * ((cin % 8) / 4) + (cout % 32) / 16].
__global__ __launch_bounds__(256) void wino_weights_kernel(const float* __restrict__ w, int Cout, int Cin,
                                                           float* __restrict__ U) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (cin, cout), cout fastest
    if (i >= (long)Cout * Cin) return;
    const int co = (int)(i % Cout), ci = (int)(i / Cout);
    const float* g = w + ((size_t)co * Cin + ci) * 9;
    double gg[3][3];
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) gg[a][c] = g[a * 3 + c];
    const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    double t[4][3];
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 3; ++c) t[a][c] = G[a][0] * gg[0][c] + G[a][1] * gg[1][c] + G[a][2] * gg[2][c];
    float* slab = U + ((size_t)(ci / 8) * (Cout / 32) + co / 32) * 4096;
    const int e = (ci & 3) * 64 + (co & 15) * 4 + 2 * ((ci & 7) >> 2) + ((co & 31) >> 4);
    for (int a = 0; a < 4; ++a)
        for (int c = 0; c < 4; ++c) {
            const double u = t[a][0] * G[c][0] + t[a][1] * G[c][1] + t[a][2] * G[c][2];
            slab[(a * 4 + c) * 256 + e] = (float)u;
        }
}

// Shortcut (1x1) weights in the transform domain: q = (i-1)*2 + (j-1), i,j in {1,2}: G[i][1]*w*G[j][1] = +-w/4.
// Slab (chunk = cin / 32, group = cout / 32) of 4096 floats, element [q][pair-step = (cin % 32) / 8][kq][l15][j].
__global__ __launch_bounds__(256) void wino_shortcut_weights_kernel(const float* __restrict__ w, int Cout, int Cin,
                                                                    float* __restrict__ U) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)Cout * Cin) return;
    const int co = (int)(i % Cout), ci = (int)(i / Cout);
    const float v = w[(size_t)co * Cin + ci] * 0.25f;
    const float sgn[4] = {1.f, -1.f, -1.f, 1.f};
    float* slab = U + ((size_t)(ci / 32) * (Cout / 32) + co / 32) * 4096;
    const int e = (((ci & 31) >> 3) * 4 + (ci & 3)) * 64 + (co & 15) * 4 + 2 * ((ci & 7) >> 2) + ((co & 31) >> 4);
    for (int q = 0; q < 4; ++q) slab[q * 1024 + e] = sgn[q] * v;
}

template <int FLAGS, bool PATCH>
hipError_t launch_wino_v(const ConvArgs& p0, hipStream_t stream) {
    ConvArgs p = p0;
    const bool wide = p.N % 64 == 0;  // 32-cout blocks on the >= 64-cout layers: measured 10 % slower (V work doubles)
    auto set_grid = [&](int gx, int gy) {  // 1-D grid, decoded by block_coords()
        p.gx = gx; p.gy = gy;
        p.xcd_map = ((long)gx * p.B) % 8 == 0;
        return dim3((unsigned)((long)gx * gy * p.B));
    };
    if (p.W < 32) {  // 16- / 8-bin layers: 64-cout blocks of 8 x 16 or 16 x 8 output pixels
        if constexpr ((FLAGS & (F_MASK | F_PRECONV | F_RESPRE)) != 0) {
            return hipErrorInvalidValue;
        } else {
            if (!wide || (p.W != 16 && p.W != 8)) return hipErrorInvalidValue;
            if (p.W == 16)
                { const dim3 g8 = set_grid((p.H + 7) / 8, p.N / 64); hipLaunchKernelGGL((wino_kernel<2, 2, FLAGS, 8, PATCH>), g8, dim3(NTHREADS), 0, stream, p); }
            else
                { const dim3 g4 = set_grid((p.H + 15) / 16, p.N / 64); hipLaunchKernelGGL((wino_kernel<2, 2, FLAGS, 4, PATCH>), g4, dim3(NTHREADS), 0, stream, p); }
            return hipGetLastError();
        }
    }
    const dim3 grid = wide ? set_grid((p.W / 32) * ((p.H + 3) / 4), p.N / 64) : set_grid((p.W / 32) * ((p.H + 7) / 8), p.N / 32);
    if constexpr ((FLAGS & F_MASK) != 0) {
        if (wide) return hipErrorInvalidValue;  // N == 32 only (host-checked)
        hipLaunchKernelGGL((wino_kernel<1, 4, FLAGS, 16, PATCH>), grid, dim3(NTHREADS), 0, stream, p);
    } else {
        if (wide)
            hipLaunchKernelGGL((wino_kernel<2, 2, FLAGS, 16, PATCH>), grid, dim3(NTHREADS), 0, stream, p);
        else
            hipLaunchKernelGGL((wino_kernel<1, 4, FLAGS, 16, PATCH>), grid, dim3(NTHREADS), 0, stream, p);
    }
    return hipGetLastError();
}

// The patch-staging schedule wins on the 16- / 8-bin layers (-9...-13 %: few, short tiles) and loses 3-7 % on the large
// ones (its 16 instead of ~9 prologue evaluations per thread and chunk are VALU work next to f32 MFMAs), so it is the
// default below W = 32 only.
template <int FLAGS>
hipError_t launch_wino(const ConvArgs& p, hipStream_t stream) {
    return p.W < 32 ? launch_wino_v<FLAGS, true>(p, stream) : launch_wino_v<FLAGS, false>(p, stream);
}

}  // namespace

bool lass_wino_supported(const ConvArgs& p) { return lass_wino_shape(lass_conv_shape(p)); }

hipError_t lass_launch_wino(ConvKind kind, const ConvArgs& p, hipStream_t stream) {
    if (!lass_wino_supported(p) || !p.w_wino || !p.in || (!p.out && !p.mask_re)) return hipErrorInvalidValue;
    switch (kind) {
        case CONV1_ACT:
            if (!p.pro_scale || !p.pro_shift || !p.epi_scale || !p.epi_shift) return hipErrorInvalidValue;
            return launch_wino<F_PRO | F_EPIACT>(p, stream);
        case CONV2_IDENT:
            if (!p.res) return hipErrorInvalidValue;
            return launch_wino<F_RES>(p, stream);
        case CONV2_SHORTCUT:
            if (!p.in2 || !p.w2_wino || !p.bias || p.Cin2 % KCB != 0) return hipErrorInvalidValue;
            if (p.mask_re) {  // fused output head: decoder_block6 geometry only
                if (p.N != 32 || p.W + 1 != p.mask_nbins || !p.mask_w || !p.mask_b || !p.mask_mag || !p.mask_cos || !p.mask_sin ||
                    !p.mask_im || p.mask_T <= 0 || p.mask_T > p.H)
                    return hipErrorInvalidValue;
                return launch_wino<F_PHASEB | F_BIAS | F_MASK>(p, stream);
            }
            return launch_wino<F_PHASEB | F_BIAS>(p, stream);
        case CONV1_ACT_PRE:
            if (!p.pro_scale || !p.pro_shift || !p.epi_scale || !p.epi_shift || !p.pre_w || !p.pre_b || p.N != 32 ||
                p.Cin != 32)
                return hipErrorInvalidValue;
            return launch_wino<F_PRO | F_EPIACT | F_PRECONV>(p, stream);
        case CONV2_IDENT_PRE:
            if (!p.res || !p.pre_w || !p.pre_b || p.N != 32) return hipErrorInvalidValue;
            return launch_wino<F_RES | F_RESPRE>(p, stream);
        default:
            return hipErrorInvalidValue;
    }
}

hipError_t lass_launch_wino_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream) {
    const long n = (long)Cout * Cin;
    hipLaunchKernelGGL(wino_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, Cout, Cin, U);
    return hipGetLastError();
}

hipError_t lass_launch_wino_shortcut_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream) {
    const long n = (long)Cout * Cin;
    hipLaunchKernelGGL(wino_shortcut_weights_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, w, Cout,
                       Cin, U);
    return hipGetLastError();
}
