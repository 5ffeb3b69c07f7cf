// conv_bf16_fused.hip - bf16 mode: the three residual blocks whose 32-channel intermediate never leaves the CU, each ONE kernel.
//   enc1_fused_bf16_kernel   encoder_block1's ConvBlockRes behind pre_conv: skip and 2x2 avg-pool out as blocked bf16 copies
//   dec6_fused_bf16_kernel   decoder_block6's ConvBlockRes (conv1 over the 64-channel concat, 1x1 shortcut) with the output head
//   dec6u_fused_bf16_kernel  the same with decoder_block6's transposed conv inside (the up-sampled half never exists in HBM)
// The blocks are byte-bound in bf16 (32 channels at 1024 x 512: MFMA busy 0.10-0.13 in the two-launch form), and half of their
// bytes were the intermediate going out to HBM from conv1's epilogue and coming back into conv2.
//
// Shared tile geometry: a workgroup owns an 8 x 32 output tile (4 waves x 2 rows).  conv1 (3x3, 16-channel chunks) runs over the
// 10 x 34 pixels conv2 needs (a 1-pixel recomputed halo: ten 32-pixel row tiles plus one tile holding the two halo columns)
// from a 12 x 36 input tile in LDS, image [octet][12][36]; its epilogue (bn2 + FiLM + leaky, zero outside the image) writes
// the bf16 intermediate into LDS; conv2 (3x3, 32 -> 32) contracts that.  Same MFMA (v_mfma_f32_32x32x16_bf16), LDS layouts and
// fragment reads as conv_bf16.hip; conv1 runs 11 pixel tiles where the two-launch form ran 8 (x 1.19 MFMAs: free at this load).
//
// The parts (above the first kernel) are what the kernels have in common: the tile coordinates, conv1's slot map, contraction
// and epilogue, a thread's units of the input tile with their load and LDS write, the weight moves by LDS-DMA, conv2's
// contraction over the plain intermediate and the bias start.  A kernel body is its own schedule: which chunk is requested
// when, which barrier guards which buffer, what waits for what.
#include <hip/hip_runtime.h>
#include "conv_common.h"
#include "kernels.h"
#include "wino_common.h"  // make_rsrc_words, lds_dma_16B, wait_vmcnt

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

namespace {

// ---- tile constants ------------------------------------------------------------------------------------------------------------
constexpr int FPW = kBf16FusedTileW, FPHT = 8;                 // output tile: 8 rows x 32 columns, 4 waves x 2 rows
constexpr int IRI = FPHT + 4, IPI = FPW + 4, NPI = IRI * IPI;  // input image (halo 2): 12 x 36 pixels
constexpr int IRM = FPHT + 2, IPM = FPW + 2, NPM = IRM * IPM;  // conv1 output = conv2 input (halo 1): 10 x 34 pixels
constexpr int NPPI = (NPI + NTHREADS - 1) / NTHREADS;          // input pixels per thread
constexpr int W_U4 = 9 * 2 * 32;                               // 16-byte units of one 16-channel weight chunk (32 couts)
constexpr int IMG1_U4 = 2 * NPI, MID_U4 = 4 * NPM + 64;        // (+ slack: lanes of a discarded tile read past the image)
// dec6 / dec6u: conv1's image and weight chunk are double-buffered, chunk c in buffer c & 1
constexpr int BUF_U4 = IMG1_U4 + W_U4;                         // one (image, weights) buffer
constexpr int NCH = 4;                                         // 16-channel chunks of the 64 concat channels
// dec6u
constexpr int LRI = IRI / 2, LPI = IPI / 2, NLP = LRI * LPI;   // low-resolution halo tile: 6 x 18 = 108 pixels
constexpr int MPH = 20, MPITCH = 2 * MPH;                      // parity-split intermediate row (17 of 20 units used per parity;
                                                               // two rows = 80 units = 0 mod 16: lanes 16-31 fall on the banks behind lanes 0-15)
constexpr int MROWS_U4 = IRM * MPITCH, MIDP_U4 = 4 * MROWS_U4;

// Tiles of one image; the grid is one workgroup per tile and clip.
__host__ __device__ __forceinline__ int fused_tiles(int H, int W) { return (W / FPW) * ((H + FPHT - 1) / FPHT); }
inline dim3 fused_grid(const ConvArgs& p) { return dim3((unsigned)((long)fused_tiles(p.H, p.W) * p.B)); }

// ---- parts -----------------------------------------------------------------------------------------------------------------------
// Clip b and output-tile origin (y0, x0) of this workgroup.  Workgroup g runs on XCD g % 8 (its own L2); every XCD walks ONE
// contiguous range of tiles, so the tiles that share halo rows / columns run side by side under the same L2 (as block_coords,
// wino_common.h).
struct FusedTile {
    int b, y0, x0;
};
__device__ __forceinline__ FusedTile fused_tile(int H, int W) {
    const unsigned lin = blockIdx.x;
    const unsigned tile = (gridDim.x & 7u) == 0 ? (lin & 7u) * (gridDim.x >> 3) + (lin >> 3) : lin;
    const int tiles_x = W / FPW, tiles = fused_tiles(H, W);
    const int b = tile / (unsigned)tiles;
    const int bxy = tile - b * tiles;
    return {b, (bxy / tiles_x) * FPHT, (bxy % tiles_x) * FPW};
}

template <int N>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[N]) {
#pragma unroll
    for (int s = 0; s < N; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
}

// conv1 over the 10 x 34 intermediate pixels: three pixel tiles (slots) per wave.  Slot s of wave w: rows w, w + 4, w + 8 (< 10)
// at columns 1..32; the third slot of wave 2 holds the halo columns 0 and 33 (lane j: row j / 2, column 33 * (j & 1)); surplus
// lanes / slots (ir == IRM) compute on a valid address and are not written.
struct Conv1Slots {
    int ir[3], ic[3];
};
__device__ __forceinline__ Conv1Slots conv1_slots(int wave, int j) {
    Conv1Slots sl;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        int ir = wave + 4 * s, ic = 1 + j;
        if (s == 2 && wave >= 2) {
            ir = wave == 2 ? (j >> 1) : IRM;  // wave 3: nothing
            ic = (j & 1) ? IPM - 1 : 0;
        }
        sl.ir[s] = ir;
        sl.ic[s] = ic;
    }
    return sl;
}

// conv1's contraction of one 16-channel chunk: 9 taps x 3 slots from the image [2 octets][12][36] and the weights of one buffer
__device__ __forceinline__ void conv1_contract(const uint4* img, const uint4* w, const Conv1Slots& sl, int khalf, int j,
                                               f32x16 (&acc1)[3]) {
    const bf16x8* abase = reinterpret_cast<const bf16x8*>(w) + khalf * 32 + j;
    const bf16x8* ibase = reinterpret_cast<const bf16x8*>(img) + khalf * NPI;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const bf16x8 a = abase[tap * 64];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int ir = min(sl.ir[s], IRM - 1);
            const bf16x8 bb = ibase[(ir + tap / 3) * IPI + sl.ic[s] + tap % 3];
            acc1[s] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bb, acc1[s], 0, 0, 0);
        }
    }
}

// Where the 16-byte unit of channel octet g at intermediate pixel (ir, ic) lies: plain [octet][10][34] (enc1, dec6), or
// parity-split [octet][row][column parity][20] (dec6u: a wave's B fragments of one sub-pixel class are contiguous units)
struct MidPlain {
    uint4* mid;
    __device__ __forceinline__ uint4* operator()(int g, int ir, int ic) const { return mid + g * NPM + ir * IPM + ic; }
};
struct MidParity {
    uint4* mid;
    __device__ __forceinline__ uint4* operator()(int g, int ir, int ic) const {
        return mid + g * MROWS_U4 + ir * MPITCH + (ic & 1) * MPH + (ic >> 1);
    }
};

// conv1's epilogue: bn2 + FiLM + leaky (resunet.py:151) with the tables lds_es / lds_eh, ZERO outside the image (conv2's zero
// padding: a border tile's halo pixels are not conv1 outputs), bf16 -> the intermediate image at unit_at(g, ir, ic)
template <class UnitAt>
__device__ __forceinline__ void conv1_epilogue(const f32x16 (&acc1)[3], const Conv1Slots& sl, const float* lds_es, const float* lds_eh,
                                               int khalf, const FusedTile& tile, int H, int W, UnitAt unit_at) {
    float es4[4][4], eh4[4][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 a = *reinterpret_cast<const float4*>(lds_es + 8 * g + 4 * khalf);
        const float4 c = *reinterpret_cast<const float4*>(lds_eh + 8 * g + 4 * khalf);
        es4[g][0] = a.x; es4[g][1] = a.y; es4[g][2] = a.z; es4[g][3] = a.w;
        eh4[g][0] = c.x; eh4[g][1] = c.y; eh4[g][2] = c.z; eh4[g][3] = c.w;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int ir = sl.ir[s], ic = sl.ic[s];
        const int gy = tile.y0 - 1 + ir, gx = tile.x0 - 1 + ic;
        const bool inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
        if (ir < IRM) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 v;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float r = leaky(acc1[s][4 * g + i] * es4[g][i] + eh4[g][i]);
                    v[i] = (__bf16)(inside ? r : 0.f);
                }
                *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(unit_at(g, ir, ic)) + khalf * 8) = v;
            }
        }
    }
}

// This thread's NPPI pixels of the 12 x 36 input tile: the pixel's offset in the H x W plane (clamped into the image) and
// whether it is inside (bit k of okbits; outside = conv1's zero padding, applied when the pixel is written to LDS)
struct TileUnits {
    unsigned off[NPPI], okbits;
};
__device__ __forceinline__ TileUnits tile_units(int tid, const FusedTile& tile, int H, int W) {
    TileUnits un;
    un.okbits = 0;
#pragma unroll
    for (int k = 0; k < NPPI; ++k) {
        const int u = min(tid + k * NTHREADS, NPI - 1);
        const int gy = tile.y0 + u / IPI - 2, gx = tile.x0 + u % IPI - 2;
        const bool ok = gy >= 0 && gy < H && gx >= 0 && gx < W;
        un.off[k] = (unsigned)(min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1));
        un.okbits |= (ok ? 1u : 0u) << k;
    }
    return un;
}

// dec6 / dec6u: chunk c (2 octets) of the blocked activated copy -> registers, set c & 1 of the two in flight.  One 16-byte unit
// = 8 channels of a pixel.  2 * NPPI memory requests per call, which the callers' wait_vmcnt counts are written in.
__device__ __forceinline__ void load_chunk(const uint4* act, int HW, int c, const TileUnits& un, uint4 (&stage)[2][2][NPPI]) {
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int k = 0; k < NPPI; ++k) stage[c & 1][o][k] = act[(size_t)(2 * c + o) * HW + un.off[k]];
}

// ... and the staged units of chunk c -> image buffer c & 1 (conv zero padding applied here; waits for the units)
__device__ __forceinline__ void put_chunk(uint4* lds4, int c, const uint4 (&stage)[2][2][NPPI], const TileUnits& un, int tid) {
    uint4* img = lds4 + (c & 1) * BUF_U4;
#pragma unroll
    for (int o = 0; o < 2; ++o)
#pragma unroll
        for (int k = 0; k < NPPI; ++k) {
            const int u = tid + k * NTHREADS;
            const bool ok = (un.okbits >> k) & 1u;
            if (u < NPI) img[o * NPI + u] = ok ? stage[c & 1][o][k] : uint4{0u, 0u, 0u, 0u};
        }
}

// n_u4 16-byte units of weights, from unit src_u4 of the buffer behind rs, to the LDS byte address dst by LDS-DMA: 1-KiB pieces
// dealt over the four waves, each one memory request of its wave.  Nothing waits here: the caller's wait_vmcnt and barrier do.
__device__ __forceinline__ void dma_weights(v4i32 rs, int src_u4, int n_u4, unsigned dst, int lane, int wave) {
    for (int piece = wave; piece < n_u4 / 64; piece += 4)
        lds_dma_16B(rs, (unsigned)lane * 16u, (unsigned)((src_u4 + piece * 64) * 16), dst + (unsigned)(piece * 1024));
}
// dec6 / dec6u: conv1's weight chunk c -> the weight region of buffer c & 1
__device__ __forceinline__ void dma_w1(v4i32 w1_rs, int c, unsigned lds0, int lane, int wave) {
    dma_weights(w1_rs, c * W_U4, W_U4, lds0 + (unsigned)(((c & 1) * BUF_U4 + IMG1_U4) * 16), lane, wave);
}
// conv2's two weight chunks -> the start of LDS, which conv1 has left behind (the caller's barrier says when)
__device__ __forceinline__ void dma_w2(v4i32 w2_rs, unsigned lds0, int lane, int wave) {
    dma_weights(w2_rs, 0, 2 * W_U4, lds0, lane, wave);
}

// conv2 over the plain intermediate image: the fragment scheme of conv_bf16.hip (image [octet][10][34], 2 rows per wave)
__device__ __forceinline__ void conv2_contract(const uint4* mid, const uint4* w2, int khalf, int j, int wave, f32x16 (&acc2)[2]) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bf16x8* bbase = reinterpret_cast<const bf16x8*>(mid) + (2 * c + khalf) * NPM + (wave * 2) * IPM + j;
        const bf16x8* abase = reinterpret_cast<const bf16x8*>(w2 + c * W_U4) + khalf * 32 + j;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bf16x8 a = abase[tap * 64];
#pragma unroll
            for (int px = 0; px < 2; ++px)
                acc2[px] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bbase[(px + tap / 3) * IPM + tap % 3], acc2[px], 0, 0, 0);
        }
    }
}

// conv2's two accumulators start at the shortcut's bias (resunet.py:163: conv bias of the 1x1)
__device__ __forceinline__ void start_at_bias(const float* bias, int khalf, f32x16 (&acc2)[2]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float bb = bias[(r & 3) + 8 * (r >> 2) + 4 * khalf];
        acc2[0][r] = bb;
        acc2[1][r] = bb;
    }
}

// ---- encoder_block1's ConvBlockRes (models/resunet.py:147-165 at the shape of :315-323), ONE kernel ----------------------------
//   x0 tile (f32, 12 x 36)  --pre_conv + BN/FiLM/leaky, bf16-->  LDS image [octet][12][36]
//   conv1 (3x3, 32 -> 32), + bn2/FiLM/leaky, zero outside the image  -->  LDS image [octet][10][34]
//   conv2 (3x3, 32 -> 32) over it  + pre_conv(x0) residual  -->  the skip as blocked bf16 copies and the 2x2 avg-pool as
//   blocked bf16 copies (the epilogue of conv_bf16.hip's kernels, store_tile).
// p: conv1 of the block (CONV1_ACT_PRE arguments: x0, pre_w / pre_b, prologue and epilogue tables, w_bf16);
// q: conv2 (CONV2_IDENT_PRE arguments with blocked bf16 outputs: res = x0, out_bf16 (+ _act), pool_bf16 (+ _act), w_bf16).
__global__ __launch_bounds__(NTHREADS, 3) void enc1_fused_bf16_kernel(ConvArgs p, ConvArgs q) {
    // conv2's weights (2 chunks) take over the input image + conv1 weight regions once conv1 is done: 47 KB per workgroup,
    // three workgroups per CU
    static_assert(2 * W_U4 <= IMG1_U4 + W_U4, "conv2's weights must fit the regions conv1 leaves behind");
    __shared__ uint4 lds4[IMG1_U4 + W_U4 + MID_U4 + (64 + 128) / 4];
    uint4* img1 = lds4;
    uint4* w1 = img1 + IMG1_U4;
    uint4* mid = w1 + W_U4;
    uint4* w2 = lds4;
    float* tabs = reinterpret_cast<float*>(mid + MID_U4);
    float* lds_es = tabs;        // conv1 epilogue (bn2 + FiLM) scale / shift
    float* lds_eh = tabs + 32;
    float* lds_act = tabs + 64;  // store_tile: skip activation scale / shift, pooled activation scale / shift

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int khalf = lane >> 5, j = lane & 31;
    const FusedTile tile = fused_tile(p.H, p.W);

    if (tid < 32) {
        lds_es[tid] = p.epi_scale[tid];
        lds_eh[tid] = p.epi_shift[(size_t)tile.b * p.epi_shift_bs + tid];
        if (q.out_bf16_act) {
            lds_act[tid] = q.act_scale[tid];
            lds_act[32 + tid] = q.act_shift[(size_t)tile.b * q.act_shift_bs + tid];
        }
        if (q.pool_bf16) {
            lds_act[64 + tid] = q.pool_act_scale[tid];
            lds_act[96 + tid] = q.pool_act_shift[(size_t)tile.b * q.act_shift_bs + tid];
        }
    }

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) uint4*)lds4;
    const v4i32 w1_rs = make_rsrc_words(p.w_bf16, 2u * W_U4 * 16u);
    const v4i32 w2_rs = make_rsrc_words(q.w_bf16, 2u * W_U4 * 16u);

    // ---- x0 at this thread's pixels of the 12 x 36 input tile (loaded once; every channel is an affine function of it) -----
    const float* x0_b = p.in + (size_t)tile.b * p.in_bs;
    const TileUnits un = tile_units(tid, tile, p.H, p.W);
    float x0v[NPPI];
#pragma unroll
    for (int k = 0; k < NPPI; ++k) x0v[k] = x0_b[un.off[k]];

    // ---- conv1 over the 10 x 34 intermediate pixels ---------------------------------------------------------------------------
    const Conv1Slots sl = conv1_slots(wave, j);
    f32x16 acc1[3];
    zero_acc(acc1);
    for (int c = 0; c < 2; ++c) {
        if (c) __syncthreads();  // chunk 0 has been contracted: image and weight regions are free
        dma_weights(w1_rs, c * W_U4, W_U4, lds0 + (unsigned)(IMG1_U4 * 16), lane, wave);
        float pcw[16], pcb[16], psc[16], psh[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            pcw[i] = p.pre_w[c * 16 + i];
            pcb[i] = p.pre_b[c * 16 + i];
            psc[i] = p.pro_scale[c * 16 + i];
            psh[i] = p.pro_shift[(size_t)tile.b * p.pro_shift_bs + c * 16 + i];
        }
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int k = 0; k < NPPI; ++k) {
                const int u = tid + k * NTHREADS;
                const bool ok = (un.okbits >> k) & 1u;
                bf16x8 pk;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    float v = x0v[k] * pcw[o * 8 + i] + pcb[o * 8 + i];       // pre_conv (resunet.py:555)
                    v = leaky(v * psc[o * 8 + i] + psh[o * 8 + i]);           // bn1 + FiLM + leaky (:150)
                    pk[i] = (__bf16)(ok ? v : 0.f);                           // conv zero padding comes after the activation
                }
                if (u < NPI) *reinterpret_cast<bf16x8*>(img1 + o * NPI + u) = pk;
            }
        wait_vmcnt<0>();
        __syncthreads();
        conv1_contract(img1, w1, sl, khalf, j, acc1);
    }

    __syncthreads();  // every wave has finished with the input image and conv1's weights: conv2's weights move in (LDS-DMA)
    dma_w2(w2_rs, lds0, lane, wave);
    conv1_epilogue(acc1, sl, lds_es, lds_eh, khalf, tile, p.H, p.W, MidPlain{mid});
    // residual = pre_conv(x0) at this lane's output pixels (resunet.py:555,165), fetched while the intermediate settles
    const int x = tile.x0 + j;
    float rtmp[2][16];
#pragma unroll
    for (int px = 0; px < 2; ++px) {
        const int y = min(tile.y0 + wave * 2 + px, q.H - 1);
        const float xv = q.res[(size_t)tile.b * q.res_bs + (size_t)y * q.W + x];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = (r & 3) + 8 * (r >> 2) + 4 * khalf;
            rtmp[px][r] = xv * q.pre_w[n] + q.pre_b[n];
        }
    }
    wait_vmcnt<0>();  // conv2's weights
    __syncthreads();

    f32x16 acc2[1][2];
    zero_acc(acc2[0]);
    conv2_contract(mid, w2, khalf, j, wave, acc2[0]);
    store_tile<1, 2, FPW, F_RES | F_RESPRE | F_OUTBF16, true>(q, acc2, rtmp, nullptr, nullptr, tile.b, 0, tile.y0, tile.x0, lane, wave, nullptr,
                                                                 lds_act);
}


// ---- decoder_block6's ConvBlockRes (resunet.py:147-165 at the shape of :408-418) with the output head, ONE kernel ----------
//   cat (activated blocked-bf16 copy, 64 channels, 12 x 36 tile)  --global -> registers -> LDS, 4 chunks of 16 channels-->
//   conv1 (3x3, 64 -> 32) over the 10 x 34 pixels conv2 needs, + bn2/FiLM/leaky, zero outside the image --> LDS image
//   conv2 (3x3, 32 -> 32) over it  +  the 1x1 shortcut over the RAW copy of the cat (operands straight from global memory
//   into the MFMA: a lane's B fragment is one 16-byte unit of the blocked layout, its A fragment one unit of the weights)
//   + bias  -->  after_conv + complex ratio mask (store_tile's F_MASK epilogue): out_real / out_imag.
// The 32-channel intermediate (0.54 GB written and read back with its halo per step) never leaves the CU.
// p: conv1 (CONV1_ACT arguments in the blocked pipeline: in_bf16 = activated cat copy, w_bf16, epilogue tables);
// q: conv2 (CONV2_SHORTCUT arguments: w_bf16, in2_bf16 = raw cat copy, w2_bf16, bias, mask head).
__global__ __launch_bounds__(NTHREADS, 3) void dec6_fused_bf16_kernel(ConvArgs p, ConvArgs q) {
    // conv1's image and weight chunk are double-buffered (one barrier per chunk, the next chunk's units and weights arrive
    // behind this chunk's MFMAs).  Once conv1 is done conv2's weights (2 chunks) take over buffer 0 and the intermediate
    // image buffer 1: 47 KB per workgroup, three workgroups per CU (launch bounds: 168 registers)
    static_assert(2 * W_U4 <= BUF_U4 && MID_U4 <= BUF_U4, "conv2's weights / the intermediate must fit one buffer each");
    __shared__ uint4 lds4[2 * BUF_U4 + (64 + 100 + 28) / 4];
    uint4* mid = lds4 + BUF_U4;
    uint4* w2 = lds4;
    float* tabs = reinterpret_cast<float*>(lds4 + 2 * BUF_U4);
    float* lds_es = tabs;        // conv1 epilogue (bn2 + FiLM) scale / shift
    float* lds_eh = tabs + 32;
    float* lds_mw = tabs + 64;   // after_conv weight [3][32] + bias [3]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int khalf = lane >> 5, j = lane & 31;
    const FusedTile tile = fused_tile(p.H, p.W);
    const int HW = p.H * p.W;

    if (tid < 32) {
        lds_es[tid] = p.epi_scale[tid];
        lds_eh[tid] = p.epi_shift[(size_t)tile.b * p.epi_shift_bs + tid];
    }
    if (tid < 99) lds_mw[tid] = tid < 96 ? q.mask_w[tid] : q.mask_b[tid - 96];

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) uint4*)lds4;
    const v4i32 w1_rs = make_rsrc_words(p.w_bf16, 4u * W_U4 * 16u);
    const v4i32 w2_rs = make_rsrc_words(q.w_bf16, 2u * W_U4 * 16u);

    // ---- this thread's units of the 12 x 36 input tile; two chunks in flight ------------------------------------------------
    const uint4* act = reinterpret_cast<const uint4*>(p.in_bf16) + (size_t)tile.b * (p.Cin / 8) * HW;
    const TileUnits un = tile_units(tid, tile, p.H, p.W);
    uint4 stage[2][2][NPPI];
    load_chunk(act, HW, 0, un, stage);
    load_chunk(act, HW, 1, un, stage);

    const Conv1Slots sl = conv1_slots(wave, j);
    f32x16 acc1[3];
    zero_acc(acc1);

    dma_w1(w1_rs, 0, lds0, lane, wave);
    put_chunk(lds4, 0, stage, un, tid);
    load_chunk(act, HW, 2, un, stage);
    wait_vmcnt<2 * NPPI>();  // weights of chunk 0: only the units of chunk 2 are younger (those of chunk 1 were requested first)
    __syncthreads();
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) dma_w1(w1_rs, c + 1, lds0, lane, wave);  // its buffer was last read in chunk c-1: every wave is past that (barrier below)
        if (c == NCH - 1) dma_w2(w2_rs, lds0, lane, wave);        // buffer 0 is free for good: conv2's weights move in behind the last chunk's MFMAs
        const uint4* buf = lds4 + (c & 1) * BUF_U4;
        conv1_contract(buf, buf + IMG1_U4, sl, khalf, j, acc1);
        if (c + 1 < NCH) {
            put_chunk(lds4, c + 1, stage, un, tid);  // image buffer (c+1) & 1 was last read in chunk c-1; the units were requested two chunks ago
            if (c + 3 < NCH) load_chunk(act, HW, c + 3, un, stage);
            // this wave's weight pieces of chunk c+1 must have landed before the barrier; younger than them are only the
            // units requested just now (in-order return): with nothing requested, everything is waited for
            if (c + 3 < NCH) wait_vmcnt<2 * NPPI>(); else wait_vmcnt<0>();
            __syncthreads();
        }
    }

    __syncthreads();  // every wave is done with image buffer 1 (chunk 3): the intermediate image goes there
    // ---- shortcut operands (1x1 over the raw cat copy, resunet.py:163): requested here (they arrive behind the epilogue below), contracted behind conv2 -------------
    const uint4* raw = reinterpret_cast<const uint4*>(q.in2_bf16) + (size_t)tile.b * (q.Cin2 / 8) * HW;
    const uint4* wsc = reinterpret_cast<const uint4*>(q.w2_bf16);  // [chunk][octet][cout]
    const int x = tile.x0 + j;
    unsigned poff[2];
#pragma unroll
    for (int px = 0; px < 2; ++px) poff[px] = (unsigned)(min(tile.y0 + wave * 2 + px, q.H - 1) * q.W + x);
    uint4 sa[NCH], sb[NCH][2];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        sa[c] = wsc[c * 64 + khalf * 32 + j];
#pragma unroll
        for (int px = 0; px < 2; ++px) sb[c][px] = raw[(size_t)(2 * c + khalf) * HW + poff[px]];
    }
    f32x16 acc2[1][2];
    start_at_bias(q.bias, khalf, acc2[0]);
    conv1_epilogue(acc1, sl, lds_es, lds_eh, khalf, tile, p.H, p.W, MidPlain{mid});
    wait_vmcnt<0>();  // conv2's weights, the shortcut operands
    __syncthreads();

    conv2_contract(mid, w2, khalf, j, wave, acc2[0]);
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int px = 0; px < 2; ++px)
            acc2[0][px] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, sa[c]), __builtin_bit_cast(bf16x8, sb[c][px]),
                                                                   acc2[0][px], 0, 0, 0);
    store_tile<1, 2, FPW, F_MASK, false>(q, acc2, nullptr, nullptr, nullptr, tile.b, 0, tile.y0, tile.x0, lane, wave, lds_mw, nullptr);
}


// ---- decoder_block6 with its transposed conv INSIDE (resunet.py:240-264 at the shape of :408-418) --------------------------
// The up-sampled half of the concat (32 channels at the full resolution: 1.1 GB written as two copies and read back with its
// halo per step) never exists in HBM.  A workgroup forms it for its own 12 x 36 input tile from the 6 x 18 low-resolution
// pixels underneath: kernel = stride, so ConvTranspose2d is a pointwise GEMM  up[(co, a, bb)][pixel] = sum_ci Wt[ci][(co, a, bb)]
// x[ci][pixel]  (x = decoder_block5's output with this conv's BN+FiLM+leaky already applied, blocked bf16) - 16 MFMAs per wave
// with BOTH operands straight from global memory (a lane's fragment is one 16-byte unit of either).  An accumulator tile is one
// channel octet x 4 sub-pixels; the khalf pair swaps halves (as tconv_store), applies conv_block2.bn1 + FiLM + leaky and writes
// 16-byte units into the image buffers of conv1's chunks 0 and 1; chunks 2 and 3 (the encoder skip) come from the activated cat
// copy as before.
// The 1x1 shortcut over the up-sampled half is linear in x as well:  Wsc[:, :32] up = W' x  with the composed weights
// W'[(a, bb, n)][ci] = sum_co Wsc[n][co] Wt[ci][(co, a, bb)]  (lass_finalize, f32 products rounded to bf16 once).  Its
// accumulator tile for sub-pixel (a, bb) is [32 couts][low-res pixels], so conv2 runs in THAT layout: wave w owns sub-pixel
// class (a, bb) = (w >> 1, w & 1) of the 8 x 32 output tile, column tile t, lane j = low-res pixel (2t + (j >> 4), j & 15); the
// intermediate image is kept parity-split ([row][column parity][20]) so that a wave's B fragments are contiguous 16-byte units.
// p, q: as dec6_fused_bf16_kernel (p.pro_scale / pro_shift = conv_block2.bn1 of the concat channels);  u: the transposed conv
// (in_bf16 = x, w_bf16 = Wt [4][2][128] units, w2_bf16 = W' [4][2][128] units, H x W = the low resolution).
__global__ __launch_bounds__(NTHREADS, 3) void dec6u_fused_bf16_kernel(ConvArgs p, ConvArgs q, ConvArgs u) {
    static_assert(2 * W_U4 + MIDP_U4 <= 2 * BUF_U4 && 2 * W_U4 <= BUF_U4, "conv2's weights fit buffer 0; the intermediate starts behind them");
    __shared__ uint4 lds4[2 * BUF_U4 + 57];
    uint4* w2 = lds4;
    uint4* mid = w2 + 2 * W_U4;  // behind conv2's weights; written only after conv1's last chunk
    float* tabs = reinterpret_cast<float*>(lds4 + 2 * BUF_U4);
    float* lds_es = tabs;        // conv1 epilogue (bn2 + FiLM) scale / shift
    float* lds_eh = tabs + 32;
    float* lds_mw = tabs + 64;   // after_conv weight [3][32] + bias [3]
    float* lds_us = tabs + 164;  // conv_block2.bn1 + FiLM of the up-sampled channels (concat channels 0..31)
    float* lds_uh = tabs + 196;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int khalf = lane >> 5, j = lane & 31;
    const FusedTile tile = fused_tile(p.H, p.W);
    const int b = tile.b, y0 = tile.y0, x0 = tile.x0;
    const int HW = p.H * p.W;
    const int lh = u.H, lw = u.W, lhw = lh * lw;

    if (tid < 32) {
        lds_es[tid] = p.epi_scale[tid];
        lds_eh[tid] = p.epi_shift[(size_t)b * p.epi_shift_bs + tid];
        lds_us[tid] = p.pro_scale[tid];
        lds_uh[tid] = p.pro_shift[(size_t)b * p.pro_shift_bs + tid];
    }
    if (tid < 99) lds_mw[tid] = tid < 96 ? q.mask_w[tid] : q.mask_b[tid - 96];

    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) uint4*)lds4;
    const v4i32 w1_rs = make_rsrc_words(p.w_bf16, 4u * W_U4 * 16u);
    const v4i32 w2_rs = make_rsrc_words(q.w_bf16, 2u * W_U4 * 16u);
    dma_w1(w1_rs, 0, lds0, lane, wave);
    dma_w1(w1_rs, 1, lds0, lane, wave);

    // ---- phase 0: the transposed conv of this tile's 6 x 18 low-resolution pixels -> conv1's image chunks 0 and 1 ------------
    const uint4* xa = reinterpret_cast<const uint4*>(u.in_bf16) + (size_t)b * (u.Cin / 8) * lhw;
    const uint4* wt = reinterpret_cast<const uint4*>(u.w_bf16);
    const int qpx = wave * 32 + j;  // this lane's low-resolution pixel (MFMA column) in the 6 x 18 tile
    const bool qvalid = qpx < NLP;
    const int qq = qvalid ? qpx : NLP - 1;
    const int ly = qq / LPI, lx = qq - ly * LPI;
    const int gly = (y0 >> 1) - 1 + ly, glx = (x0 >> 1) - 1 + lx;
    const bool qin = qvalid && gly >= 0 && gly < lh && glx >= 0 && glx < lw;  // outside the image: conv1's zero padding
    const unsigned xoff = (unsigned)(min(max(gly, 0), lh - 1) * lw + min(max(glx, 0), lw - 1));
    // every operand of the 16 MFMAs is requested up front (80 registers, free at this point of the kernel): one exposed
    // round trip instead of one per accumulator tile (hipcc sinks the loads to their uses otherwise)
    uint4 xb[4], wa[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s) xb[s] = xa[(size_t)(2 * s + khalf) * lhw + xoff];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int s = 0; s < 4; ++s) wa[m][s] = wt[(s * 2 + khalf) * 128 + 32 * m + j];
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();  // tables visible
#pragma unroll
    for (int m = 0; m < 4; ++m) {  // accumulator tile m = concat channels 8m .. 8m+7 x 4 sub-pixels
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wa[m][s]), __builtin_bit_cast(bf16x8, xb[s]), acc, 0, 0, 0);
        // register r = row (r & 3) + 8 (r >> 2) + 4 khalf = channel 2 (r >> 2) + khalf, sub-pixel r & 3 = (a, bb).  One
        // v_permlane32_swap per (channel pair, bb) hands lane khalf output row a = khalf with all 8 channels (two adjacent
        // units, bb = 0, 1): it swaps lanes 32-63 of its first operand (a = 0 values of the odd channel) with lanes 0-31 of
        // the second (a = 1 values of the even channel)
        float ch[2][8];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const float a0 = acc[4 * g + bb], a1 = acc[4 * g + 2 + bb];  // (named floats: hipcc's bit_cast of a vector ELEMENT reads element 0)
                const auto sw = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a0), __builtin_bit_cast(unsigned, a1), false, false);
                const unsigned r0 = sw[0], r1 = sw[1];
                ch[bb][2 * g] = __builtin_bit_cast(float, r0);
                ch[bb][2 * g + 1] = __builtin_bit_cast(float, r1);
            }
        float us[8], uh[8];
        {
            const float4 a0 = *reinterpret_cast<const float4*>(lds_us + 8 * m), a1 = *reinterpret_cast<const float4*>(lds_us + 8 * m + 4);
            const float4 h0 = *reinterpret_cast<const float4*>(lds_uh + 8 * m), h1 = *reinterpret_cast<const float4*>(lds_uh + 8 * m + 4);
            us[0] = a0.x; us[1] = a0.y; us[2] = a0.z; us[3] = a0.w; us[4] = a1.x; us[5] = a1.y; us[6] = a1.z; us[7] = a1.w;
            uh[0] = h0.x; uh[1] = h0.y; uh[2] = h0.z; uh[3] = h0.w; uh[4] = h1.x; uh[5] = h1.y; uh[6] = h1.z; uh[7] = h1.w;
        }
        uint4* img = lds4 + (m >> 1) * BUF_U4 + (m & 1) * NPI + (2 * ly + khalf) * IPI + 2 * lx;
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            bf16x8 v;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float t = leaky(ch[bb][k] * us[k] + uh[k]);  // conv_block2.bn1 + FiLM + leaky (resunet.py:150)
                v[k] = (__bf16)(qin ? t : 0.f);
            }
            if (qvalid) *reinterpret_cast<bf16x8*>(img + bb) = v;
        }
    }

    // ---- the encoder skip (concat channels 32..63 = chunks 2, 3): this thread's units of the 12 x 36 tile, staged in registers
    const uint4* act = reinterpret_cast<const uint4*>(p.in_bf16) + (size_t)b * (p.Cin / 8) * HW;
    const TileUnits un = tile_units(tid, tile, p.H, p.W);
    uint4 stage[2][2][NPPI];
    load_chunk(act, HW, 2, un, stage);
    load_chunk(act, HW, 3, un, stage);

    const Conv1Slots sl = conv1_slots(wave, j);
    f32x16 acc1[3];
    zero_acc(acc1);

    // conv2 / shortcut pixel classes (see the header): sub-pixel (spa, spb) = wave, column tile t, lane j
    const int spa = wave >> 1, spb = wave & 1;
    int oy[2];
    const int ox = 2 * (j & 15) + spb;
#pragma unroll
    for (int t = 0; t < 2; ++t) oy[t] = 2 * (2 * t + (j >> 4)) + spa;
    uint4 xs[2][4], au[4];  // shortcut over the up-sampled half: W' (rows of this wave's sub-pixel) and x at the inner 4 x 16 pixels

    wait_vmcnt<2 * 2 * NPPI>();  // conv1's weight chunks 0 and 1 have landed (only the skip units are younger)
    __syncthreads();             // ... and everyone's image units of chunks 0 and 1 are written
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c >= 1 && c + 1 < NCH) dma_w1(w1_rs, c + 1, lds0, lane, wave);  // its buffer was last read in chunk c-1: every wave is past that (barrier below)
        if (c == NCH - 1) {              // buffer 0 is free for good: conv2's weights move in behind the last chunk's MFMAs
            dma_w2(w2_rs, lds0, lane, wave);
            const uint4* wsu = reinterpret_cast<const uint4*>(u.w2_bf16);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                au[s] = wsu[(s * 2 + khalf) * 128 + wave * 32 + j];
#pragma unroll
                for (int t = 0; t < 2; ++t)
                    xs[t][s] = xa[(size_t)(2 * s + khalf) * lhw + (size_t)min((y0 >> 1) + 2 * t + (j >> 4), lh - 1) * lw + (x0 >> 1) + (j & 15)];
            }
        }
        const uint4* buf = lds4 + (c & 1) * BUF_U4;
        conv1_contract(buf, buf + IMG1_U4, sl, khalf, j, acc1);
        if (c + 1 < NCH) {
            if (c + 1 >= 2) put_chunk(lds4, c + 1, stage, un, tid);  // image buffer (c+1) & 1 was last read in chunk c-1
            wait_vmcnt<0>();                                         // this wave's weight pieces of chunk c+1
            __syncthreads();
        }
    }
    // accumulators of conv2 start at the shortcut's bias + the shortcut over the up-sampled half
    f32x16 acc2[2];
    start_at_bias(q.bias, khalf, acc2);
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, au[s]), __builtin_bit_cast(bf16x8, xs[t][s]), acc2[t], 0, 0, 0);

    __syncthreads();  // every wave is done with buffer 1 (chunk 3): the intermediate image goes there
    // ---- shortcut over the skip half (1x1 over the RAW cat copy, resunet.py:163): requested here, contracted behind conv2 ------
    const uint4* raw = reinterpret_cast<const uint4*>(q.in2_bf16) + (size_t)b * (q.Cin2 / 8) * HW;
    const uint4* wsc = reinterpret_cast<const uint4*>(q.w2_bf16);  // [chunk][octet][cout]
    uint4 sa[2], sb[2][2];
#pragma unroll
    for (int c = 2; c < NCH; ++c) {
        sa[c - 2] = wsc[c * 64 + khalf * 32 + j];
#pragma unroll
        for (int t = 0; t < 2; ++t)
            sb[c - 2][t] = raw[(size_t)(2 * c + khalf) * HW + (size_t)min(y0 + oy[t], q.H - 1) * q.W + x0 + ox];
    }
    conv1_epilogue(acc1, sl, lds_es, lds_eh, khalf, tile, p.H, p.W, MidParity{mid});
    wait_vmcnt<0>();  // conv2's weights, the shortcut operands
    __syncthreads();

    // ---- conv2 over the intermediate image, sub-pixel class (spa, spb) ----------------------------------------------------------
    int lbase[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) lbase[t] = 2 * (2 * t + (j >> 4)) * MPITCH + (j & 15);
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const bf16x8* bbase = reinterpret_cast<const bf16x8*>(mid) + (2 * c + khalf) * MROWS_U4;
        const bf16x8* abase = reinterpret_cast<const bf16x8*>(w2 + c * W_U4) + khalf * 32 + j;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const bf16x8 a = abase[tap * 64];
            const int col = spb + tap % 3;  // intermediate column = 2 lx + col, row = 2 ly + spa + tap / 3
            const int off = (spa + tap / 3) * MPITCH + (col & 1) * MPH + (col >> 1);
#pragma unroll
            for (int t = 0; t < 2; ++t)
                acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bbase[lbase[t] + off], acc2[t], 0, 0, 0);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            acc2[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, sa[c]), __builtin_bit_cast(bf16x8, sb[c][t]), acc2[t], 0, 0, 0);

    // ---- after_conv + complex ratio mask (resunet.py:570-574,436-519): the khalf pair holds all 32 channels of a pixel; lane
    // khalf finishes the pixel of column tile t = khalf
    float lg[3];
#pragma unroll
    for (int qd = 0; qd < 3; ++qd) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float wv = lds_mw[qd * 32 + (r & 3) + 8 * (r >> 2) + 4 * khalf];
            s0 += wv * acc2[0][r];
            s1 += wv * acc2[1][r];
        }
        s0 += __shfl_xor(s0, 32, 64);
        s1 += __shfl_xor(s1, 32, 64);
        lg[qd] = (khalf ? s1 : s0) + lds_mw[96 + qd];
    }
    const int yy = y0 + (khalf ? oy[1] : oy[0]);
    if (yy < q.mask_T) mask_pixel(q, b, yy, x0 + ox, lg[0], lg[1], lg[2]);
}


// W'[(sp, n)][ci] = sum_co Wsc[n][co] * Wt[ci][co][sp]  (sp = a * 2 + bb): the 1x1 shortcut of decoder_block6's ConvBlockRes
// composed with the transposed conv in front of it (both linear; resunet.py:122-128,163 and :216-224,250), f32.
// wsc (Nsc, Ccat, 1, 1) - only its first Cup input channels (the up-sampled half of torch.cat((x, skip), 1)); wt (Cin, Cup, 2, 2).
__global__ __launch_bounds__(256) void compose_up_shortcut_kernel(const float* __restrict__ wsc, const float* __restrict__ wt,
                                                                  int Cin, int Cup, int Ccat, int Nsc, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;  // ((sp * Nsc) + n) * Cin + ci
    if (i >= 4 * Nsc * Cin) return;
    const int ci = i % Cin, n = (i / Cin) % Nsc, sp = i / (Cin * Nsc);
    double s = 0.0;
    for (int co = 0; co < Cup; ++co) s += (double)wsc[(size_t)n * Ccat + co] * (double)wt[((size_t)ci * Cup + co) * 4 + sp];
    out[i] = (float)s;
}

}  // namespace

// lass_*_fused_bf16_shape (conv_route.h) && the pointers are there
bool lass_enc1_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q) {
    return lass_enc1_fused_bf16_shape(lass_conv_shape(p), lass_conv_shape(q), q.pool_bf16 != nullptr) && p.w_bf16 && q.w_bf16 &&
           !p.w_bf16_lo && !q.w_bf16_lo && p.pre_w && p.pre_b && p.pro_scale && p.pro_shift && p.epi_scale && p.epi_shift && q.res &&
           q.pre_w && q.pre_b && q.out_bf16 && !q.out_bf16_lo && q.out_noct > 0 && (!q.pool_bf16 || q.pool_bf16_act) && q.B == p.B;
}

hipError_t lass_launch_enc1_fused_bf16(const ConvArgs& p, const ConvArgs& q, hipStream_t stream) {
    if (!lass_enc1_fused_bf16_supported(p, q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(enc1_fused_bf16_kernel, fused_grid(p), dim3(NTHREADS), 0, stream, p, q);
    return hipGetLastError();
}

bool lass_dec6_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q) {
    return lass_dec6_fused_bf16_shape(lass_conv_shape(p), lass_conv_shape(q)) && p.in_bf16 && !p.in_bf16_lo && p.w_bf16 && q.w_bf16 &&
           !p.w_bf16_lo && !q.w_bf16_lo && p.epi_scale && p.epi_shift && q.in2_bf16 && q.w2_bf16 && !q.w2_bf16_lo && q.bias &&
           q.mask_im && q.mask_w && q.mask_b && q.mask_mag && q.mask_cos && q.mask_sin && q.W + 1 == q.mask_nbins && q.mask_T > 0 &&
           q.mask_T <= q.H && !q.pool_bf16 && q.B == p.B;
}

hipError_t lass_launch_dec6_fused_bf16(const ConvArgs& p, const ConvArgs& q, hipStream_t stream) {
    if (!lass_dec6_fused_bf16_supported(p, q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec6_fused_bf16_kernel, fused_grid(p), dim3(NTHREADS), 0, stream, p, q);
    return hipGetLastError();
}

bool lass_dec6u_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q, const ConvArgs& u) {
    return lass_dec6_fused_bf16_supported(p, q) && lass_dec6u_fused_bf16_shape(lass_conv_shape(p), lass_conv_shape(q), u.Cin, u.H, u.W) &&
           p.pro_scale && p.pro_shift && u.in_bf16 && u.w_bf16 && u.w2_bf16 && u.B == p.B;
}

hipError_t lass_launch_dec6u_fused_bf16(const ConvArgs& p, const ConvArgs& q, const ConvArgs& u, hipStream_t stream) {
    if (!lass_dec6u_fused_bf16_supported(p, q, u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dec6u_fused_bf16_kernel, fused_grid(p), dim3(NTHREADS), 0, stream, p, q, u);
    return hipGetLastError();
}

hipError_t lass_launch_compose_up_shortcut(const float* wsc, const float* wt, int Cin, int Cup, int Ccat, int Nsc, float* out,
                                           hipStream_t stream) {
    const int n = 4 * Nsc * Cin;
    hipLaunchKernelGGL(compose_up_shortcut_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, wsc, wt, Cin, Cup, Ccat, Nsc, out);
    return hipGetLastError();
}
