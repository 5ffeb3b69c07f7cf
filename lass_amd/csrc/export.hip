// export.hip - planar float32 at the model rate -> a WAV data chunk at the file's rate in one launch: the polyphase FIR of
// resample.hip (y[n] = sum_m x[m] * h[n*down - m*up + half], zeros outside the plane, the same tap order and fmaf chain, so the
// value before quantisation is bit-identical to lass_decode_resample's for that plane), truncation to frames_out, PCM
// quantisation and channel interleave.  The mirror of resample.hip; DESIGN.md section 16.
//
// One workgroup makes `tile` consecutive output frames of one recording.  Beside resample.hip's table and span (the table staged
// once per workgroup, the span once per channel) it keeps in LDS
//   stage = the tile's encoded bytes, frame-major and interleaved as they go to memory, at the byte offset (first byte & 3), so
//           that LDS and global dwords line up.
// The stage is then written out as contiguous dwords; a 2-byte store is made only where the tile's byte range starts or ends off
// a 4-byte boundary (PCM16 alone, and with an even tile the end of the row alone).
#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTileMax = 2048;          // output frames per workgroup (fewer when table + span + stage would not fit in LDS)
constexpr int kTilePlain = 1024;        // k_encode: 1024 frames x 8 channels x 4 bytes = 32 KiB of stage
constexpr int kLdsFloats = 160 * 256;   // 160 KiB per CU

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

// up == down == 1: quantise and interleave only
__global__ __launch_bounds__(kThreads) void k_encode(const float* __restrict__ planes, long long row_stride, long long plane_stride,
                                                     int ch, int enc, unsigned char* __restrict__ out, long long out_row_stride,
                                                     int frames_out, unsigned* __restrict__ clipped) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    unsigned char* stage0 = reinterpret_cast<unsigned char*>(lds);
    const int tid = threadIdx.x;
    const int bps = sample_bytes(enc);
    const long long n0 = (long long)blockIdx.x * kTilePlain;
    const int nout = (int)(frames_out - n0 < kTilePlain ? frames_out - n0 : kTilePlain);
    const size_t a = (size_t)n0 * ch * bps;
    unsigned char* stage = stage0 + (a & 3);
    const float* x = planes + (size_t)blockIdx.y * row_stride + n0;
    unsigned clips = 0;
    for (int c = 0; c < ch; ++c)
        for (int i = tid; i < nout; i += kThreads) stage_put(stage, i * ch + c, x[(size_t)c * plane_stride + i], enc, &clips);
    __syncthreads();
    store_tile(stage0, out + (size_t)blockIdx.y * out_row_stride, a, (size_t)nout * ch * bps, tid);
    if (clipped && clips) atomicAdd(clipped + blockIdx.y, clips);
}

__global__ __launch_bounds__(kThreads) void k_resample_encode(const float* __restrict__ planes, long long row_stride,
                                                              long long plane_stride, int L_in, int ch, int enc, int up, int down,
                                                              const float* __restrict__ taps, int n_taps, int J, int tile,
                                                              int span_floats, unsigned char* __restrict__ out,
                                                              long long out_row_stride, int frames_out,
                                                              unsigned* __restrict__ clipped) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int Jp = J | 1;
    float* tab = lds;                                     // [up][Jp]
    float* span = lds + (size_t)up * Jp;                  // [span_floats] = [(up - 1 + (tile - 1) * down) / up + J]
    unsigned char* stage0 = reinterpret_cast<unsigned char*>(lds + (((size_t)up * Jp + span_floats + 3) & ~(size_t)3));
    const int tid = threadIdx.x;
    const int bps = sample_bytes(enc);
    const float* rec = planes + (size_t)blockIdx.y * row_stride;

    // 64-bit: n*down passes 2^31 on long recordings (16 -> 44.1 kHz: after 304 s)
    const long long n0 = (long long)blockIdx.x * tile;
    const long long t0 = n0 * down + (n_taps - 1) / 2;
    const long long q0 = t0 / up;
    const unsigned r0 = (unsigned)(t0 - q0 * up);
    const int nout = (int)(frames_out - n0 < tile ? frames_out - n0 : tile);
    const int S = (int)((r0 + (unsigned)(nout - 1) * (unsigned)down) / (unsigned)up) + J;
    const long long mlo = q0 - (J - 1);
    const size_t a = (size_t)n0 * ch * bps;
    unsigned char* stage = stage0 + (a & 3);

    // only the last tap of a phase can lie past the filter's end
    for (int p = tid; p < up; p += kThreads) tab[p * Jp + J - 1] = 0.f;
    __syncthreads();
    for (int k = tid; k < n_taps; k += kThreads) tab[(k % up) * Jp + k / up] = taps[k];

    unsigned clips = 0;
    for (int c = 0; c < ch; ++c) {
        const float* x0 = rec + (size_t)c * plane_stride;
        if (c) __syncthreads();                           // the previous channel's reads of the span
        for (int s = tid; s < S; s += kThreads) {
            const long long m = mlo + s;
            span[s] = (m >= 0 && m < L_in) ? x0[m] : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < nout; i += kThreads) {
            const unsigned t = r0 + (unsigned)i * (unsigned)down;
            const unsigned q = t / (unsigned)up;
            const float* g = tab + (t - q * (unsigned)up) * Jp;
            const float* x = span + q + (J - 1);
            float acc = 0.f;
            for (int j = 0; j < J; ++j) acc = fmaf(x[-j], g[j], acc);
            stage_put(stage, i * ch + c, acc, enc, &clips);
        }
    }
    __syncthreads();
    store_tile(stage0, out + (size_t)blockIdx.y * out_row_stride, a, (size_t)nout * ch * bps, tid);
    if (clipped && clips) atomicAdd(clipped + blockIdx.y, clips);
}

}  // namespace

hipError_t lass_launch_resample_encode(const float* planes, long long row_stride, long long plane_stride, int B, int ch, int L_in,
                                       int up, int down, const float* taps, int n_taps, int enc, void* out, long long out_row_stride,
                                       int frames_out, unsigned* clipped, hipStream_t stream) {
    if (B <= 0 || B > 65535 || ch < 1 || ch > 8 || L_in <= 0 || frames_out <= 0 || up < 1 || down < 1) return hipErrorInvalidValue;
    unsigned char* o = static_cast<unsigned char*>(out);
    const int bps = enc == LASS_WAV_PCM16 ? 2 : 4;
    if (up == 1 && down == 1) {
        const size_t lds = (size_t)kTilePlain * ch * bps + 4;
        hipLaunchKernelGGL(k_encode, dim3((frames_out + kTilePlain - 1) / kTilePlain, B), dim3(kThreads), lds, stream, planes,
                           row_stride, plane_stride, ch, enc, o, out_row_stride, frames_out, clipped);
        return hipGetLastError();
    }
    const int J = (n_taps + up - 1) / up;
    const size_t table = lass_resample_table_floats(up, n_taps);
    if (up > LASS_RESAMPLE_MAX_RATIO || down > LASS_RESAMPLE_MAX_RATIO || n_taps > LASS_RESAMPLE_MAX_TAPS || table > LASS_RESAMPLE_MAX_TABLE)
        return hipErrorInvalidValue;
    // the largest tile whose span and stage fit beside the table (one frame needs J floats of span and at most 9 of stage: it
    // always fits under the caps above); the stage starts on a multiple of four floats
    auto floats_of = [&](int t) {
        const size_t head = (table + lass_resample_span_floats(up, down, n_taps, t) + 3) & ~(size_t)3;
        return head + ((size_t)t * ch * bps + 4 + 3) / 4;
    };
    int tile = kTileMax;
    while (tile > 1 && floats_of(tile) > (size_t)kLdsFloats) tile /= 2;
    const size_t lds = floats_of(tile) * sizeof(float);
    if (lds > (size_t)kLdsFloats * sizeof(float)) return hipErrorInvalidValue;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_resample_encode),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFloats * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    const long long nblk = ((long long)frames_out + tile - 1) / tile;
    if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_resample_encode, dim3((unsigned)nblk, B), dim3(kThreads), lds, stream, planes, row_stride, plane_stride, L_in,
                       ch, enc, up, down, taps, n_taps, J, tile, (int)lass_resample_span_floats(up, down, n_taps, tile), o,
                       out_row_stride, frames_out, clipped);
    return hipGetLastError();
}
