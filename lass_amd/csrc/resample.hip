// resample.hip - WAV payload -> mono float32 at the target rate in one launch: PCM decode, mono down-mix and a polyphase FIR
// (scipy.signal.resample_poly's arithmetic: y[n] = sum_m x[m] * h[n*down - m*up + half], zeros outside the clip).  Stands in for
// librosa.load(path, sr=16000, mono=True) (dcase_evaluator.py:73-74) on files that are not mono at the target rate; DESIGN.md
// section 12 has the filter, the indexing and what is pinned to what.
//
// One workgroup makes `tile` consecutive outputs of one clip with the FIR of polyphase.h (the table, the span and the tap chain
// are there); its span holds the decoded, down-mixed frames of the tile's reach.  Results are bit-identical per clip, whatever the
// batch, the row stride or the tile an output falls in.  No atomics.
//
// The PLANAR instances are the same two kernels without the down-mix: one output plane per channel, for callers that separate
// every channel on its own (export.hip is the way back out).
#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

#include "polyphase.h"
#include "wav_sample.h"     // sample_at: one sample of the payload, by read_wav's rule

// One frame of the clip as read_wav makes it: its samples (sample_at) summed in ascending channel order in f32 and divided by
// their count, correctly rounded (numpy's mean over the channel axis).
__device__ __forceinline__ float frame_at(const unsigned char* __restrict__ row, long long m, int ch, int enc) {
    float s = sample_at(row, m * ch, enc);
    if (ch == 1) return s;
    for (int c = 1; c < ch; ++c) s += sample_at(row, m * ch + c, enc);
    return __fdiv_rn(s, (float)ch);
}

// Plane c of frame m.  PLANAR: channel c as it stands (out holds ch planes); otherwise the down-mix (one plane, c == 0).  frame_at
// with one channel IS sample_at, and the tap order and the fmaf chain are polyphase.h's for both, so a planar plane is
// bit-identical to the mono result of a payload holding that channel alone.
template <bool PLANAR>
__device__ __forceinline__ float plane_at(const unsigned char* __restrict__ row, long long m, int c, int ch, int enc) {
    return PLANAR ? sample_at(row, m * ch + c, enc) : frame_at(row, m, ch, enc);
}

// up == down == 1: decode (+ down-mix) only (a stereo or PCM file already at the target rate)
template <bool PLANAR>
__global__ __launch_bounds__(kThreads) void k_decode(const unsigned char* __restrict__ raw, long long row_stride, int frames,
                                                     int ch, int enc, float* __restrict__ out) {
    const int n = blockIdx.x * kThreads + threadIdx.x;
    if (n >= frames) return;
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;
    const int planes = PLANAR ? ch : 1;
    float* o = out + (size_t)blockIdx.y * planes * frames + n;
    for (int c = 0; c < planes; ++c) o[(size_t)c * frames] = plane_at<PLANAR>(row, n, c, ch, enc);
}

// The table is staged once per workgroup, the span once per plane (one span in LDS whatever the plane count).
template <bool PLANAR>
__global__ __launch_bounds__(kThreads) void k_decode_resample(const unsigned char* __restrict__ raw, long long row_stride,
                                                              int frames, int ch, int enc, int up, int down,
                                                              const float* __restrict__ taps, int n_taps, int J, int tile,
                                                              float* __restrict__ out, int L_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const unsigned char* row = raw + (size_t)blockIdx.y * row_stride;
    const FirTile T = fir_tile(lds, up, down, n_taps, J, tile, L_out);
    fir_table(T, taps, n_taps);
    const int planes = PLANAR ? ch : 1;
    for (int c = 0; c < planes; ++c) {
        if (c) __syncthreads();              // the previous plane's reads of the span
        fir_fill(T, frames, [&](long long m) { return plane_at<PLANAR>(row, m, c, ch, enc); });
        __syncthreads();
        float* o = out + ((size_t)blockIdx.y * planes + c) * L_out + T.n0;
        for (int i = threadIdx.x; i < T.nout; i += kThreads) o[i] = fir_output(T, i);
    }
}

template <bool PLANAR>
hipError_t launch(const PayloadRows& rows, int B, const RationalFilter& F, float* out, int L_out, hipStream_t stream) {
    const unsigned char* raw = static_cast<const unsigned char*>(rows.p);
    const int up = F.up, down = F.down, n_taps = F.n_taps;
    if (up == 1 && down == 1) {
        hipLaunchKernelGGL(k_decode<PLANAR>, dim3((rows.frames + kThreads - 1) / kThreads, B), dim3(kThreads), 0, stream, raw,
                           rows.row_stride_bytes, rows.frames, rows.ch, rows.enc, out);
        return hipGetLastError();
    }
    // the largest tile whose input span fits beside the table (one output needs J frames: always fits under the caps)
    FirPlan P;
    hipError_t e = fir_plan(reinterpret_cast<const void*>(k_decode_resample<PLANAR>), up, down, n_taps, L_out, [&](int t) {
        return lass_resample_table_floats(up, n_taps) + lass_resample_span_floats(up, down, n_taps, t);
    }, &P);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode_resample<PLANAR>, dim3(P.nblk, B), dim3(kThreads), P.lds, stream, raw, rows.row_stride_bytes, rows.frames,
                       rows.ch, rows.enc, up, down, F.taps, n_taps, P.J, P.tile, out, L_out);
    return hipGetLastError();
}

}  // namespace

size_t lass_resample_span_floats(int up, int down, int n_taps, int tile) {
    const int J = (n_taps + up - 1) / up;
    return ((size_t)(up - 1) + (size_t)(tile - 1) * down) / up + J;
}

hipError_t lass_launch_decode_resample(const PayloadRows& raw, int B, const RationalFilter& F, bool planar, float* out, int L_out,
                                       hipStream_t stream) {
    if (B <= 0 || B > 65535 || raw.frames <= 0 || L_out <= 0 || F.up < 1 || F.down < 1 || raw.ch < 1) return hipErrorInvalidValue;
    return planar ? launch<true>(raw, B, F, out, L_out, stream) : launch<false>(raw, B, F, out, L_out, stream);
}
