// export.hip - planar float32 at the model rate -> a WAV data chunk at the file's rate in one launch: the polyphase FIR of
// polyphase.h (y[n] = sum_m x[m] * h[n*down - m*up + half], zeros outside the plane; resample.hip's tap chain, so the
// value before quantisation is bit-identical to lass_decode_resample's for that plane), truncation to frames_out, PCM
// quantisation and channel interleave.  The mirror of resample.hip; DESIGN.md section 16.
//
// One workgroup makes `tile` consecutive output frames of one recording.  Beside polyphase.h's table and span (the table staged
// once per workgroup, the span once per channel) it keeps in LDS
//   stage = the tile's encoded bytes, frame-major and interleaved as they go to memory, at the byte offset (first byte & 3), so
//           that LDS and global dwords line up.
// The stage is then written out as contiguous dwords; a 2-byte store is made only where the tile's byte range starts or ends off
// a 4-byte boundary (PCM16 alone, and with an even tile the end of the row alone).
//
// Both kernels are templates over where an output y goes (Sink): quantised into the stage (kEncode, lass_resample_encode), the
// same after one multiplication by the row's gain (kEncodeGain, lass_resample_encode_gain), or into the row's peak |y| with no
// stage and no store (kPeak, lass_resample_peak).  Up to that point the three are one body, so they see the same y.
//
// They are templates, too, over a dry source (Dry...: none, or one DryRows): with one, the value that goes to the sink is
//   v = fl(x + fl(amount[b] * y)),  x the sample of the original payload row at the same frame and channel (wav_sample.h)
// - the remix of lass_remix_encode and lass_remix_peak.  y, the tile plan, the stage and the sinks are the
// same code; without a dry source a kernel takes no further argument and is the instantiation it was.
//
// k_true_peak (lass_resample_true_peak) is a fourth use of the same chain: it keeps the y of its tile and a halo as floats in LDS
// and runs polyphase.h's chain once more over them, at (os, 1), for the peak between the samples.  DESIGN.md section 19.
#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

#include "polyphase.h"
#include "wav_sample.h"

constexpr int kTilePlain = 1024;        // k_encode: 1024 frames x 8 channels x 4 bytes = 32 KiB of stage

// wavio.write_wav_pcm16 / write_wav_pcm32 on a float32: y * 2^15 (2^31) is exact, rintf rounds ties to even as numpy.round does,
// the clip is the writers'.  NaN -> 0.  *clips counts the samples the clip changed.
__device__ __forceinline__ int quantise(float y, int enc, unsigned* clips) {
    if (y != y) return 0;
    if (enc == LASS_WAV_PCM16) {
        const float r = rintf(y * 32768.0f);
        if (r > 32767.0f) { ++*clips; return 32767; }
        if (r < -32768.0f) { ++*clips; return -32768; }
        return (int)r;
    }
    const float r = rintf(y * 2147483648.0f);
    if (r >= 2147483648.0f) { ++*clips; return 2147483647; }
    if (r < -2147483648.0f) { ++*clips; return -2147483647 - 1; }
    return (int)r;
}

// sample k (frame-major, interleaved) of the tile into the stage
__device__ __forceinline__ void stage_put(unsigned char* stage, int k, float y, int enc, unsigned* clips) {
    if (enc == LASS_WAV_PCM16) reinterpret_cast<short*>(stage)[k] = (short)quantise(y, enc, clips);
    else if (enc == LASS_WAV_PCM32) reinterpret_cast<int*>(stage)[k] = quantise(y, enc, clips);
    else reinterpret_cast<float*>(stage)[k] = y;
}

// stage0 (16-byte aligned LDS) holds the bytes [a, a + nbytes) of the row at offset a & 3: head and tail halves, dwords between
__device__ __forceinline__ void store_tile(const unsigned char* stage0, unsigned char* __restrict__ row, size_t a, size_t nbytes,
                                           int tid) {
    const size_t e = a + nbytes;
    const size_t a4 = (a + 3) & ~(size_t)3, e4 = e & ~(size_t)3;      // a, e are even: a4 - a and e - e4 are 0 or 2
    const unsigned* src = reinterpret_cast<const unsigned*>(stage0) + (a4 - (a & ~(size_t)3)) / 4;
    unsigned* dst = reinterpret_cast<unsigned*>(row + a4);
    if (e4 > a4) {
        const size_t nd = (e4 - a4) / 4;
        for (size_t w = tid; w < nd; w += kThreads) dst[w] = src[w];
    }
    if (tid == 0 && a4 > a && a4 <= e)
        *reinterpret_cast<unsigned short*>(row + a) = *reinterpret_cast<const unsigned short*>(stage0 + (a & 3));
    if (tid == 64 && e > e4 && e4 >= a4)
        *reinterpret_cast<unsigned short*>(row + e4) = *reinterpret_cast<const unsigned short*>(stage0 + (a & 3) + (e4 - a));
}

__device__ __forceinline__ int sample_bytes(int enc) { return enc == LASS_WAV_PCM16 ? 2 : 4; }

enum Sink { kEncode, kEncodeGain, kPeak };

// the row's gain (1 where the sink takes none)
template <Sink kSink>
__device__ __forceinline__ float row_gain(const float* __restrict__ gain) {
    if constexpr (kSink == kEncodeGain) return gain[blockIdx.y];
    return 1.0f;
}

// output y, sample k of the tile: into the stage (times g, rounded once, for kEncodeGain), or its |y| bits into pk (NaN skipped)
template <Sink kSink>
__device__ __forceinline__ void emit(unsigned char* stage, int k, float y, float g, int enc, unsigned* clips, unsigned* pk) {
    if constexpr (kSink == kPeak) {
        const unsigned a = __float_as_uint(y) & 0x7fffffffu;
        if (a <= 0x7f800000u && a > *pk) *pk = a;
    } else {
        if constexpr (kSink == kEncodeGain) y = __fmul_rn(g, y);
        stage_put(stage, k, y, enc, clips);
    }
}

// The dry source of a remix: B payload rows (enc = LASS_WAV_*, row_stride bytes apart) and one amount per row.
struct DryRows {
    const unsigned char* rows;
    long long row_stride;
    const float* amount;
    int enc;
};

// What a workgroup with a dry source makes of an output y, sample idx (frame-major, interleaved; 64-bit: a row's samples pass 2^31
// before a plane's do) of its row, before the sink has it: fl(x + fl(k * y)) with x = sample idx of the payload row and k the row's
// amount - two roundings, so numpy float32 restates them.  (__fadd_rn(x, __fmul_rn(k, y)) does not say so here: the toolchain's
// header defines the two as plain + and *, and under HIP's default -ffp-contract=fast they inline to one v_fmac_f32.  The pragma
// takes the contract flag off both operations instead.)  x is read straight from memory: consecutive lanes are on consecutive
// frames and the channel loop comes back to the same lines, so the stage and the tile plan are those of a launch without a dry
// source.  Without one (the empty pack) the kernels, which ask `if constexpr`, make the call they always made and compile to the
// instructions they were.
template <class... Dry>
struct Mix {};
template <>
struct Mix<DryRows> {
    const unsigned char* row;
    float k;
    int enc;
    __device__ __forceinline__ Mix(DryRows d) : row(d.rows + (size_t)blockIdx.y * d.row_stride), k(d.amount[blockIdx.y]), enc(d.enc) {}
    __device__ __forceinline__ float operator()(long long idx, float y) const {
#pragma clang fp contract(off)
        const float p = k * y;
        return sample_at(row, idx, enc) + p;
    }
};

// the tile's end: the stage to memory and the clip count, or the workgroup's peak, to the row's counter
template <Sink kSink>
__device__ __forceinline__ void finish(const unsigned char* stage0, unsigned char* __restrict__ out, long long out_row_stride, size_t a,
                                       size_t nbytes, int tid, unsigned clips, unsigned* __restrict__ clipped, unsigned pk,
                                       unsigned* __restrict__ peak) {
    if constexpr (kSink == kPeak) {
        for (int w = 32; w > 0; w >>= 1) {
            const unsigned o = (unsigned)__shfl_xor((int)pk, w);
            pk = o > pk ? o : pk;
        }
        if ((tid & 63) == 0 && pk) atomicMax(peak + blockIdx.y, pk);
    } else {
        __syncthreads();
        store_tile(stage0, out + (size_t)blockIdx.y * out_row_stride, a, nbytes, tid);
        if (clipped && clips) atomicAdd(clipped + blockIdx.y, clips);
    }
}

// up == down == 1: quantise and interleave only
template <Sink kSink, class... Dry>
__global__ __launch_bounds__(kThreads) void k_encode(const float* __restrict__ planes, long long row_stride, long long plane_stride,
                                                     int ch, int enc, unsigned char* __restrict__ out, long long out_row_stride,
                                                     int frames_out, unsigned* __restrict__ clipped, const float* __restrict__ gain,
                                                     unsigned* __restrict__ peak, Dry... dry) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char* stage0 = reinterpret_cast<unsigned char*>(lds);
    const int tid = threadIdx.x;
    const int bps = sample_bytes(enc);
    const long long n0 = (long long)blockIdx.x * kTilePlain;
    const int nout = (int)(frames_out - n0 < kTilePlain ? frames_out - n0 : kTilePlain);
    const size_t a = (size_t)n0 * ch * bps;
    unsigned char* stage = stage0 + (a & 3);
    const float* x = planes + (size_t)blockIdx.y * row_stride + n0;
    const float g = row_gain<kSink>(gain);
    const Mix<Dry...> mix{dry...};
    unsigned clips = 0, pk = 0;
    for (int c = 0; c < ch; ++c)
        for (int i = tid; i < nout; i += kThreads) {
            if constexpr (sizeof...(Dry) == 0) emit<kSink>(stage, i * ch + c, x[(size_t)c * plane_stride + i], g, enc, &clips, &pk);
            else emit<kSink>(stage, i * ch + c, mix((n0 + i) * ch + c, x[(size_t)c * plane_stride + i]), g, enc, &clips, &pk);
        }
    finish<kSink>(stage0, out, out_row_stride, a, (size_t)nout * ch * bps, tid, clips, clipped, pk, peak);
}

template <Sink kSink, class... Dry>
__global__ __launch_bounds__(kThreads) void k_resample_encode(const float* __restrict__ planes, long long row_stride,
                                                              long long plane_stride, int L_in, int ch, int enc, int up, int down,
                                                              const float* __restrict__ taps, int n_taps, int J, int tile,
                                                              int span_floats, unsigned char* __restrict__ out,
                                                              long long out_row_stride, int frames_out,
                                                              unsigned* __restrict__ clipped, const float* __restrict__ gain,
                                                              unsigned* __restrict__ peak, Dry... dry) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int bps = sample_bytes(enc);
    const float* rec = planes + (size_t)blockIdx.y * row_stride;
    const FirTile T = fir_tile(lds, up, down, n_taps, J, tile, frames_out);
    unsigned char* stage0 = reinterpret_cast<unsigned char*>(lds + (((size_t)up * T.Jp + span_floats + 3) & ~(size_t)3));
    const size_t a = (size_t)T.n0 * ch * bps;
    unsigned char* stage = stage0 + (a & 3);
    fir_table(T, taps, n_taps);

    const float g = row_gain<kSink>(gain);
    const Mix<Dry...> mix{dry...};
    unsigned clips = 0, pk = 0;
    for (int c = 0; c < ch; ++c) {
        const float* x0 = rec + (size_t)c * plane_stride;
        if (c) __syncthreads();                           // the previous channel's reads of the span
        fir_fill(T, L_in, [&](long long m) { return x0[m]; });
        __syncthreads();
        for (int i = tid; i < T.nout; i += kThreads) {
            if constexpr (sizeof...(Dry) == 0) emit<kSink>(stage, i * ch + c, fir_output(T, i), g, enc, &clips, &pk);
            else emit<kSink>(stage, i * ch + c, mix((T.n0 + i) * ch + c, fir_output(T, i)), g, enc, &clips, &pk);
        }
    }
    finish<kSink>(stage0, out, out_row_stride, a, (size_t)T.nout * ch * bps, tid, clips, clipped, pk, peak);
}

// ---- the true-peak sink (lass_resample_true_peak) --------------------------------------------------------
// The peak of y and of y interpolated os times: z[k] = sum_m y[m] * g[k - m*os + 10*os], g the 20*os + 1 taps of the (os, 1)
// filter, which polyphase.h evaluates as J2 = 21 taps per phase over the frames n - 10 ... n + 10 of output k = n*os + p.  One
// workgroup makes the y of its tile and of kOsHalo frames on either side (J2 - 1 = 20 frames of reach in all, zeros outside the
// row's frames_out frames) into a float stage in LDS, one channel at a time, and runs the os - 1 interpolated phases of its own
// frames over the stage with polyphase.h's fir_output itself: the stage is the span and the second table the table of a
// FirTile of (up, down) = (os, 1) whose first output is the stage's frame kOsHalo.  Phase 0 is y itself.
constexpr int kOsJ = 21;                // taps per phase of the second filter: ceil((20*os + 1) / os)
constexpr int kOsHalo = (kOsJ - 1) / 2;

__host__ __device__ __forceinline__ size_t true_peak_stage_floats(int tile) { return ((size_t)tile + 2 * kOsHalo + 3) & ~(size_t)3; }

// kFir false: up == down == 1, the planes go straight into the stage (no first table, no span)
template <bool kFir>
__global__ __launch_bounds__(kThreads) void k_true_peak(const float* __restrict__ planes, long long row_stride, long long plane_stride,
                                                        int L_in, int ch, int up, int down, const float* __restrict__ taps, int n_taps,
                                                        int J, int tile, int span_floats, int frames_out, int os,
                                                        const float* __restrict__ os_taps, int n_os_taps, unsigned* __restrict__ peak) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const float* rec = planes + (size_t)blockIdx.y * row_stride;
    const long long n0 = (long long)blockIdx.x * tile;
    const int nout = (int)(frames_out - n0 < tile ? frames_out - n0 : tile);
    const long long lo = n0 - kOsHalo;                                          // the frame stage[0] holds
    const long long first = lo < 0 ? 0 : lo;                                    // the frames of the row among the stage's
    const long long last = n0 + nout + kOsHalo < frames_out ? n0 + nout + kOsHalo : frames_out;
    float* stage = lds + (kFir ? (((size_t)up * (J | 1) + span_floats + 3) & ~(size_t)3) : 0);
    FirTile T, T2;
    if constexpr (kFir) {
        T = fir_tile_at(lds, up, down, n_taps, J, first, (int)(last - first));
        fir_table(T, taps, n_taps);
    }
    T2.J = kOsJ;
    T2.Jp = kOsJ | 1;
    T2.up = os;
    T2.down = 1;
    T2.tab = stage + true_peak_stage_floats(tile);
    T2.span = stage;
    T2.r0 = 0;
    fir_table(T2, os_taps, n_os_taps);

    unsigned pk = 0;
    for (int c = 0; c < ch; ++c) {
        const float* x0 = rec + (size_t)c * plane_stride;
        if (c) __syncthreads();                           // the previous channel's reads of the stage
        if constexpr (kFir) {
            fir_fill(T, L_in, [&](long long m) { return x0[m]; });
            __syncthreads();
        }
        for (int s = tid; s < nout + 2 * kOsHalo; s += kThreads) {
            const long long f = lo + s;
            float y = 0.f;
            if (f >= first && f < last) {
                if constexpr (kFir) y = fir_output(T, (int)(f - first));
                else y = x0[f];
            }
            stage[s] = y;
        }
        __syncthreads();
        for (int i = tid; i < nout; i += kThreads) {
            emit<kPeak>(nullptr, 0, stage[i + kOsHalo], 1.0f, 0, nullptr, &pk);
            for (int p = 1; p < os; ++p) emit<kPeak>(nullptr, 0, fir_output(T2, i * os + p), 1.0f, 0, nullptr, &pk);
        }
    }
    finish<kPeak>(nullptr, nullptr, 0, 0, 0, tid, 0, nullptr, pk, peak);
}

// floats of LDS a tile of t frames needs: table and span of t + 2 * kOsHalo first-stage outputs, the stage, the second table
size_t true_peak_floats(int up, int down, int n_taps, int os, int t) {
    const size_t head = (up == 1 && down == 1) ? 0
        : (lass_resample_table_floats(up, n_taps) + lass_resample_span_floats(up, down, n_taps, t + 2 * kOsHalo) + 3) & ~(size_t)3;
    return head + true_peak_stage_floats(t) + (size_t)os * (kOsJ | 1);
}

}  // namespace

// One launch for the three sinks, with or without a dry source.  kPeak keeps no stage (enc, out and clipped unused), so its tiles
// are as large as the span allows.
template <Sink kSink, class... Dry>
static hipError_t launch(const PlaneRows& P, const RationalFilter& F, int enc, unsigned char* o, long long out_row_stride, int frames_out,
                         unsigned* clipped, const float* gain, unsigned* peak, hipStream_t stream, Dry... dry) {
    const int B = P.B, ch = P.ch, up = F.up, down = F.down, n_taps = F.n_taps;
    if (B <= 0 || B > 65535 || ch < 1 || ch > 8 || P.L <= 0 || frames_out <= 0 || up < 1 || down < 1) return hipErrorInvalidValue;
    const int bps = enc == LASS_WAV_PCM16 ? 2 : 4;
    if (up == 1 && down == 1) {
        const size_t lds = kSink == kPeak ? 0 : (size_t)kTilePlain * ch * bps + 4;
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_encode<kSink, Dry...>), dim3((frames_out + kTilePlain - 1) / kTilePlain, B), dim3(kThreads),
                           lds, stream, P.p, P.row_stride, P.plane_stride, ch, enc, o, out_row_stride, frames_out, clipped, gain, peak,
                           dry...);
        return hipGetLastError();
    }
    // the largest tile whose span and stage fit beside the table (one frame needs J floats of span and at most 9 of stage: it
    // always fits under the caps); the stage starts on a multiple of four floats
    FirPlan plan;
    hipError_t e = fir_plan(reinterpret_cast<const void*>(k_resample_encode<kSink, Dry...>), up, down, n_taps, frames_out, [&](int t) {
        const size_t head = (lass_resample_table_floats(up, n_taps) + lass_resample_span_floats(up, down, n_taps, t) + 3) & ~(size_t)3;
        return kSink == kPeak ? head : head + ((size_t)t * ch * bps + 4 + 3) / 4;
    }, &plan);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_resample_encode<kSink, Dry...>), dim3(plan.nblk, B), dim3(kThreads), plan.lds, stream, P.p,
                       P.row_stride, P.plane_stride, P.L, ch, enc, up, down, F.taps, n_taps, plan.J, plan.tile,
                       (int)lass_resample_span_floats(up, down, n_taps, plan.tile), o, out_row_stride, frames_out, clipped, gain, peak,
                       dry...);
    return hipGetLastError();
}

static DryRows dry_rows(const DrySource& d) {
    return {static_cast<const unsigned char*>(d.rows.p), d.rows.row_stride_bytes, d.amount, d.rows.enc};
}

hipError_t lass_launch_encode(const PlaneRows& P, const RationalFilter& F, const DrySource* dry, const float* gain, const PayloadRows& out,
                              unsigned* clipped, hipStream_t stream) {
    auto go = [&](auto... d) {
        unsigned char* o = static_cast<unsigned char*>(const_cast<void*>(out.p));   // the one PayloadRows that is written
        return gain ? launch<kEncodeGain>(P, F, out.enc, o, out.row_stride_bytes, out.frames, clipped, gain, nullptr, stream, d...)
                    : launch<kEncode>(P, F, out.enc, o, out.row_stride_bytes, out.frames, clipped, nullptr, nullptr, stream, d...);
    };
    return dry ? go(dry_rows(*dry)) : go();
}

hipError_t lass_launch_sample_peak(const PlaneRows& P, const RationalFilter& F, const DrySource* dry, int frames_out, float* peak,
                                   hipStream_t stream) {
    if (P.B <= 0) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(peak, 0, (size_t)P.B * sizeof(float), stream);
    if (e != hipSuccess) return e;
    auto go = [&](auto... d) {
        return launch<kPeak>(P, F, LASS_WAV_F32, nullptr, 0, frames_out, nullptr, nullptr, reinterpret_cast<unsigned*>(peak), stream, d...);
    };
    return dry ? go(dry_rows(*dry)) : go();
}

bool lass_resample_true_peak_fits(int up, int down, int n_taps, int os) {
    return true_peak_floats(up, down, n_taps, os, 1) <= (size_t)kLdsFloats;
}

hipError_t lass_launch_resample_true_peak(const PlaneRows& P, const RationalFilter& F, int frames_out, const Oversampler& O, float* peak,
                                          hipStream_t stream) {
    const int B = P.B, up = F.up, down = F.down, n_taps = F.n_taps, os = O.os;
    if (B <= 0 || B > 65535 || P.ch < 1 || P.ch > 8 || P.L <= 0 || frames_out <= 0 || up < 1 || down < 1 || (os != 2 && os != 4) ||
        O.n_taps != 20 * os + 1)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(peak, 0, (size_t)B * sizeof(float), stream);
    if (e != hipSuccess) return e;
    unsigned* pk = reinterpret_cast<unsigned*>(peak);
    if (up == 1 && down == 1) {
        const size_t lds = true_peak_floats(1, 1, 1, os, kTileMax) * sizeof(float);
        hipLaunchKernelGGL(k_true_peak<false>, dim3((frames_out + kTileMax - 1) / kTileMax, B), dim3(kThreads), lds, stream, P.p,
                           P.row_stride, P.plane_stride, P.L, P.ch, 1, 1, nullptr, 1, 1, kTileMax, 0, frames_out, os, O.taps, O.n_taps, pk);
        return hipGetLastError();
    }
    // the stage costs LDS beside table and span, and the span reaches 2 * kOsHalo outputs further: never a larger tile than kPeak's
    FirPlan plan;
    e = fir_plan(reinterpret_cast<const void*>(k_true_peak<true>), up, down, n_taps, frames_out,
                 [&](int t) { return true_peak_floats(up, down, n_taps, os, t); }, &plan);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_true_peak<true>, dim3(plan.nblk, B), dim3(kThreads), plan.lds, stream, P.p, P.row_stride, P.plane_stride, P.L,
                       P.ch, up, down, F.taps, n_taps, plan.J, plan.tile,
                       (int)lass_resample_span_floats(up, down, n_taps, plan.tile + 2 * kOsHalo), frames_out, os, O.taps, O.n_taps, pk);
    return hipGetLastError();
}
