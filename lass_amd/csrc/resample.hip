// resample.hip - WAV payload -> mono float32 at the target rate in one launch: PCM decode, mono down-mix and a polyphase FIR
// (scipy.signal.resample_poly's arithmetic: y[n] = sum_m x[m] * h[n*down - m*up + half], zeros outside the clip).  Stands in for
// librosa.load(path, sr=16000, mono=True) (dcase_evaluator.py:73-74) on files that are not mono at the target rate; DESIGN.md
// section 12 has the filter, the indexing and what is pinned to what.
//
// One workgroup makes `tile` consecutive outputs of one clip.  With t = n*down + half, output n reads the input frames
// m0 - j (m0 = t / up, j = 0 ... J-1, J = ceil(n_taps / up)) against the taps h[p + j*up] of its phase p = t % up, so the workgroup
// keeps in LDS
//   tab[p][j] = h[p + j*up] (0 past the filter's end), row pitch J | 1: the lanes of a wave sit on different phases, and an odd
//               pitch spreads their rows over the banks; with up == 1 there is one row, which every lane reads at the same j (a
//               broadcast);
//   span[s]   = the decoded, down-mixed frame (first frame of the tile's reach) + s, zero outside the clip.
// Every output is one f32 fmaf chain over j = 0 ... J-1 in that order, whatever the batch, the row stride or the tile it falls in:
// results are bit-identical per clip.  No atomics.
//
// k_decode_planar / k_decode_resample_planar are the same two kernels without the down-mix: one output plane per channel, for
// callers that separate every channel on its own (export.hip is the way back out).
#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileMax = 2048;          // outputs per workgroup (fewer when the input span would not fit in LDS)
constexpr int kLdsFloats = 160 * 256;   // 160 KiB per CU

// One frame of the clip as read_wav makes it: x/32768 (PCM16), round-to-nearest int -> float then * 2^-31 (PCM32: equal to
// read_wav's float64 division rounded once, the scaling being exact), the float itself (float32); channels summed in ascending
// order in f32 and divided by their count, correctly rounded (numpy's mean over the channel axis).
__device__ __forceinline__ float sample_at(const unsigned char* __restrict__ row, long long idx, int enc) {
    if (enc == LASS_WAV_PCM16) return (float)reinterpret_cast<const short*>(row)[idx] * (1.0f / 32768.0f);
    if (enc == LASS_WAV_PCM32) return __int2float_rn(reinterpret_cast<const int*>(row)[idx]) * (1.0f / 2147483648.0f);
    return reinterpret_cast<const float*>(row)[idx];
}

__device__ __forceinline__ float frame_at(const unsigned char* __restrict__ row, long long m, int ch, int enc) {
    float s = sample_at(row, m * ch, enc);
    if (ch == 1) return s;
    for (int c = 1; c < ch; ++c) s += sample_at(row, m * ch + c, enc);
    return __fdiv_rn(s, (float)ch);
}

// up == down == 1: decode + down-mix only (a stereo or PCM file already at the target rate)
__global__ __launch_bounds__(kThreads) void k_decode(const unsigned char* __restrict__ raw, long long row_stride, int frames,
                                                     int ch, int enc, float* __restrict__ out) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= frames) return;
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;
    out[(size_t)blockIdx.y * frames + n] = frame_at(row, n, ch, enc);
}

__global__ __launch_bounds__(kThreads) void k_decode_resample(const unsigned char* __restrict__ raw, long long row_stride,
                                                              int frames, int ch, int enc, int up, int down,
                                                              const float* __restrict__ taps, int n_taps, int J, int tile,
                                                              float* __restrict__ out, int L_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Jp = J | 1;
    float* tab = lds;                        // [up][Jp]
    float* span = lds + (size_t)up * Jp;     // [(up - 1 + (tile - 1) * down) / up + J]
    const int tid = threadIdx.x;
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;

    // 64-bit: n*down and m*up pass 2^31 on long clips (44.1 -> 16 kHz: after 304 s)
    const long long n0 = (long long)blockIdx.x * tile;
    const long long t0 = n0 * down + (n_taps - 1) / 2;
    const long long q0 = t0 / up;
    const unsigned r0 = (unsigned)(t0 - q0 * up);
    const int nout = (int)(L_out - n0 < tile ? L_out - n0 : tile);
    const int S = (int)((r0 + (unsigned)(nout - 1) * (unsigned)down) / (unsigned)up) + J;
    const long long mlo = q0 - (J - 1);

    // only the last tap of a phase can lie past the filter's end
    for (int p = tid; p < up; p += kThreads) tab[p * Jp + J - 1] = 0.f;
    __syncthreads();
    for (int k = tid; k < n_taps; k += kThreads) tab[(k % up) * Jp + k / up] = taps[k];
    for (int s = tid; s < S; s += kThreads) {
        const long long m = mlo + s;
        span[s] = (m >= 0 && m < frames) ? frame_at(row, m, ch, enc) : 0.f;
    }
    __syncthreads();

    for (int i = tid; i < nout; i += kThreads) {
        const unsigned t = r0 + (unsigned)i * (unsigned)down;
        const unsigned q = t / (unsigned)up;
        const float* g = tab + (t - q * (unsigned)up) * Jp;
        const float* x = span + q + (J - 1);
        float acc = 0.f;
        for (int j = 0; j < J; ++j) acc = fmaf(x[-j], g[j], acc);
        out[(size_t)blockIdx.y * L_out + n0 + i] = acc;
    }
}

// The planar siblings: one plane per channel instead of their average, out (B, ch, L_out).  Plane c is what the kernels above
// make of a mono payload holding channel c alone - frame_at with one channel IS sample_at, and the tap order and the fmaf chain
// are theirs - so it is bit-identical to them.
__global__ __launch_bounds__(kThreads) void k_decode_planar(const unsigned char* __restrict__ raw, long long row_stride, int frames,
                                                            int ch, int enc, float* __restrict__ out) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= frames) return;
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;
    float* o = out + (size_t)blockIdx.y * ch * frames + n;
    for (int c = 0; c < ch; ++c) o[(size_t)c * frames] = sample_at(row, (long long)n * ch + c, enc);
}

// The table is staged once per workgroup, the span once per channel (the same LDS plan as k_decode_resample: one span).
__global__ __launch_bounds__(kThreads) void k_decode_resample_planar(const unsigned char* __restrict__ raw, long long row_stride,
                                                                     int frames, int ch, int enc, int up, int down,
                                                                     const float* __restrict__ taps, int n_taps, int J, int tile,
                                                                     float* __restrict__ out, int L_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Jp = J | 1;
    float* tab = lds;                        // [up][Jp]
    float* span = lds + (size_t)up * Jp;     // [(up - 1 + (tile - 1) * down) / up + J]
    const int tid = threadIdx.x;
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;

    const long long n0 = (long long)blockIdx.x * tile;
    const long long t0 = n0 * down + (n_taps - 1) / 2;
    const long long q0 = t0 / up;
    const unsigned r0 = (unsigned)(t0 - q0 * up);
    const int nout = (int)(L_out - n0 < tile ? L_out - n0 : tile);
    const int S = (int)((r0 + (unsigned)(nout - 1) * (unsigned)down) / (unsigned)up) + J;
    const long long mlo = q0 - (J - 1);

    for (int p = tid; p < up; p += kThreads) tab[p * Jp + J - 1] = 0.f;
    __syncthreads();
    for (int k = tid; k < n_taps; k += kThreads) tab[(k % up) * Jp + k / up] = taps[k];

    for (int c = 0; c < ch; ++c) {
        if (c) __syncthreads();              // the previous channel's reads of the span
        for (int s = tid; s < S; s += kThreads) {
            const long long m = mlo + s;
            span[s] = (m >= 0 && m < frames) ? sample_at(row, m * ch + c, enc) : 0.f;
        }
        __syncthreads();
        float* o = out + ((size_t)blockIdx.y * ch + c) * L_out + n0;
        for (int i = tid; i < nout; i += kThreads) {
            const unsigned t = r0 + (unsigned)i * (unsigned)down;
            const unsigned q = t / (unsigned)up;
            const float* g = tab + (t - q * (unsigned)up) * Jp;
            const float* x = span + q + (J - 1);
            float acc = 0.f;
            for (int j = 0; j < J; ++j) acc = fmaf(x[-j], g[j], acc);
            o[i] = acc;
        }
    }
}

}  // namespace

size_t lass_resample_table_floats(int up, int n_taps) {
    const int J = (n_taps + up - 1) / up;
    return (size_t)up * (size_t)(J | 1);
}

size_t lass_resample_span_floats(int up, int down, int n_taps, int tile) {
    const int J = (n_taps + up - 1) / up;
    return ((size_t)(up - 1) + (size_t)(tile - 1) * down) / up + J;
}

hipError_t lass_launch_decode_resample_planar(const void* raw, long long row_stride, int B, int frames, int ch, int enc, int up,
                                              int down, const float* taps, int n_taps, float* out, int L_out, hipStream_t stream) {
    if (B <= 0 || B > 65535 || frames <= 0 || L_out <= 0 || up < 1 || down < 1 || ch < 1) return hipErrorInvalidValue;
    const unsigned char* r = static_cast<const unsigned char*>(raw);
    if (up == 1 && down == 1) {
        hipLaunchKernelGGL(k_decode_planar, dim3((frames + kThreads - 1) / kThreads, B), dim3(kThreads), 0, stream, r, row_stride,
                           frames, ch, enc, out);
        return hipGetLastError();
    }
    const int J = (n_taps + up - 1) / up;
    const size_t table = lass_resample_table_floats(up, n_taps);
    if (up > LASS_RESAMPLE_MAX_RATIO || down > LASS_RESAMPLE_MAX_RATIO || n_taps > LASS_RESAMPLE_MAX_TAPS || table > LASS_RESAMPLE_MAX_TABLE)
        return hipErrorInvalidValue;
    // k_decode_resample's plan: the largest tile whose input span fits beside the table
    int tile = kTileMax;
    while (tile > 1 && table + lass_resample_span_floats(up, down, n_taps, tile) > (size_t)kLdsFloats) tile /= 2;
    const size_t lds = (table + lass_resample_span_floats(up, down, n_taps, tile)) * sizeof(float);
    if (lds > (size_t)kLdsFloats * sizeof(float)) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_resample_planar),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFloats * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    const long long nblk = ((long long)L_out + tile - 1) / tile;
    if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_decode_resample_planar, dim3((unsigned)nblk, B), dim3(kThreads), lds, stream, r, row_stride, frames, ch, enc,
                       up, down, taps, n_taps, J, tile, out, L_out);
    return hipGetLastError();
}

hipError_t lass_launch_decode_resample(const void* raw, long long row_stride, int B, int frames, int ch, int enc, int up, int down,
                                       const float* taps, int n_taps, float* out, int L_out, hipStream_t stream) {
    if (B <= 0 || B > 65535 || frames <= 0 || L_out <= 0 || up < 1 || down < 1) return hipErrorInvalidValue;
    const unsigned char* r = static_cast<const unsigned char*>(raw);
    if (up == 1 && down == 1) {
        hipLaunchKernelGGL(k_decode, dim3((frames + kThreads - 1) / kThreads, B), dim3(kThreads), 0, stream, r, row_stride, frames,
                           ch, enc, out);
        return hipGetLastError();
    }
    const int J = (n_taps + up - 1) / up;
    const size_t table = lass_resample_table_floats(up, n_taps);
    if (up > LASS_RESAMPLE_MAX_RATIO || down > LASS_RESAMPLE_MAX_RATIO || n_taps > LASS_RESAMPLE_MAX_TAPS || table > LASS_RESAMPLE_MAX_TABLE)
        return hipErrorInvalidValue;
    // the largest tile whose input span fits beside the table (one output needs J frames: always fits under the caps above)
    int tile = kTileMax;
    auto span_of = [&](int t) { return ((size_t)(up - 1) + (size_t)(t - 1) * down) / up + J; };
    while (tile > 1 && table + span_of(tile) > (size_t)kLdsFloats) tile /= 2;
    const size_t lds = (table + span_of(tile)) * sizeof(float);
    if (lds > (size_t)kLdsFloats * sizeof(float)) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_decode_resample),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFloats * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    const long long nblk = ((long long)L_out + tile - 1) / tile;
    if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_decode_resample, dim3((unsigned)nblk, B), dim3(kThreads), lds, stream, r, row_stride, frames, ch, enc, up,
                       down, taps, n_taps, J, tile, out, L_out);
    return hipGetLastError();
}
