// stft.hip - STFT front end (fused magnitude/phase + bn0) and iSTFT back end for gfx950.
//
// Replaces (reference: /root/reference):
//   torchlibrosa STFT.forward  (call: models/base.py:84; cfg: models/resunet.py:284-292) - there a Conv1d against a
//       513x1024 windowed DFT matrix (1.05 GMAC/clip); here a radix-4 Stockham FFT in LDS, two real frames per complex
//       transform (n_fft 1024, or 2048 with zero-padded windows for the multi-STFT model).
//   Base.spectrogram_phase     (models/base.py:83-88, eps :91)
//   bn0 / T-pad / F-crop       (models/resunet.py:537-552)
//   torchlibrosa ISTFT.forward (call: models/resunet.py:510) - Hermitian extension, inverse DFT x Hann, overlap-add,
//       division by the window-sum-square envelope, trim: one fused kernel, overlap-add in LDS, no frame scratch.
// All of it is HBM-bound streaming: frames are read as contiguous 4-KB runs of the waveform, spectra are written as
// contiguous 513-float rows.
#include <hip/hip_runtime.h>
#include "kernels.h"

namespace {

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }

// u * exp(-i*theta) (forward) or u * exp(+i*theta) (inverse); w = (cos theta, sin theta)
template <bool INV>
__device__ __forceinline__ float2 ctw(float2 u, float2 w) {
    if (INV) return make_float2(u.x * w.x - u.y * w.y, u.y * w.x + u.x * w.y);
    return make_float2(u.x * w.x + u.y * w.y, u.y * w.x - u.x * w.y);
}

// centre=True: sample n of a clip of L samples under reflect padding of n_fft/2 (< L) at either end
__device__ __forceinline__ int reflect(int n, int L) {
    if (n < 0) n = -n;
    if (n >= L) n = 2 * (L - 1) - n;
    return n;
}

#ifdef LASS_STFT_DBG
// Diagnostic build only (tools/stft_hazard_probe.py): every radix-4 pass of the forward transform of
// stft2_kernel records, per workgroup, [pass][kind][1024] float2 with kind 0 = the four points as READ from LDS, kind 1 = the
// three twiddles as READ from the LDS table (slot 0 unused), kind 2 = the four results as COMPUTED, in front of their LDS
// stores.  A wrong launch then says whether its first wrong value was read (LDS path) or computed (vector ALU).
__device__ float2* g_stft_dbg = nullptr;
#define STFT_DBG_REC(kind, slot, val) \
    if (dbg) dbg[(pass * 3 + (kind)) * N + i + (slot) * (N / 4)] = (val)
#else
#define STFT_DBG_REC(kind, slot, val)
#endif

// N-point complex FFT, forward or inverse, for N in {256, 512, 1024, 2048}: radix-4 Stockham passes plus one radix-2 pass
// when log2 N is odd; 256 threads, each taking (N/4)/256 butterflies per pass (or idling).  tw2k[m] = (cos, sin)(2*pi*m/2048).
template <int N, bool INV>
__device__ __forceinline__ float2* fft_c(float2* a, float2* b, const float2* tw2k, int tid, float2* dbg = nullptr) {
    constexpr int LOG2 = N == 256 ? 8 : N == 512 ? 9 : N == 1024 ? 10 : 11;
    constexpr int NP4 = LOG2 / 2;
    constexpr int TWS = 2048 / N;  // stride into the 2048-entry table
    float2* src = a;
    float2* dst = b;
#pragma unroll
    for (int pass = 0; pass < NP4; ++pass) {
        const int p = 1 << (2 * pass);
#pragma unroll
        for (int i = tid; i < N / 4; i += 256) {
            const int k = i & (p - 1);
            const int j = ((i - k) << 2) + k;
            const int ts = (N / 4 / p) * TWS;
            float2 u0 = src[i], u1 = src[i + N / 4], u2 = src[i + N / 2], u3 = src[i + 3 * N / 4];
            STFT_DBG_REC(0, 0, u0); STFT_DBG_REC(0, 1, u1); STFT_DBG_REC(0, 2, u2); STFT_DBG_REC(0, 3, u3);
            if (pass > 0) {
                const float2 w1 = tw2k[k * ts], w2 = tw2k[2 * k * ts], w3 = tw2k[3 * k * ts];
                STFT_DBG_REC(1, 1, w1); STFT_DBG_REC(1, 2, w2); STFT_DBG_REC(1, 3, w3);
                u1 = ctw<INV>(u1, w1);
                u2 = ctw<INV>(u2, w2);
                u3 = ctw<INV>(u3, w3);
            }
            const float2 a0 = cadd(u0, u2), a1 = csub(u0, u2), a2 = cadd(u1, u3);
            float2 a3 = csub(u1, u3);
            a3 = INV ? make_float2(-a3.y, a3.x) : make_float2(a3.y, -a3.x);  // * (+i) inverse, * (-i) forward
            const float2 r0 = cadd(a0, a2), r1 = cadd(a1, a3), r2 = csub(a0, a2), r3 = csub(a1, a3);
            STFT_DBG_REC(2, 0, r0); STFT_DBG_REC(2, 1, r1); STFT_DBG_REC(2, 2, r2); STFT_DBG_REC(2, 3, r3);
            dst[j] = r0;
            dst[j + p] = r1;
            dst[j + 2 * p] = r2;
            dst[j + 3 * p] = r3;
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
    }
    if (LOG2 & 1) {  // final radix-2 pass, p = N/2
#pragma unroll
        for (int i = tid; i < N / 2; i += 256) {
            const float2 u0 = src[i];
            const float2 u1 = ctw<INV>(src[i + N / 2], tw2k[i * TWS]);
            dst[i] = cadd(u0, u1);
            dst[i + N / 2] = csub(u0, u1);
        }
        __syncthreads();
        float2* t = src; src = dst; dst = t;
    }
    return src;  // natural order
}

struct MultiStftArgs {
    int nwin;
    int n_fft[LASS_MAX_STFT_WINDOWS];
    float* mag[LASS_MAX_STFT_WINDOWS];
    float* cosv[LASS_MAX_STFT_WINDOWS];
    float* sinv[LASS_MAX_STFT_WINDOWS];
};

template <int N>
__device__ __forceinline__ void stft_frame(const float* __restrict__ w, int L, int hop, int t, size_t row,
                                           const float2* TW, float2* A, float2* Bf, float* __restrict__ mag,
                                           float* __restrict__ cosv, float* __restrict__ sinv, int tid) {
    constexpr int TWS = 2048 / N;
    for (int idx = tid; idx < N; idx += 256) {
        const int n = reflect(t * hop + idx - N / 2, L);
        const float wn = 0.5f - 0.5f * TW[idx * TWS].x;  // periodic Hann
        A[idx] = make_float2(w[n] * wn, 0.f);
    }
    __syncthreads();
    const float2* X = fft_c<N, false>(A, Bf, TW, tid);
    for (int f = tid; f <= N / 2; f += 256) {
        const float re = X[f].x, im = X[f].y;
        const float m = sqrtf(re * re + im * im);
        const float den = fmaxf(m, 1e-10f);  // torchlibrosa magphase: the clamp is on |X| (precompute_stfts.py:51)
        mag[row + f] = m;
        cosv[row + f] = re / den;
        sinv[row + f] = im / den;
    }
}

// One launch for all analysis windows (they share the hop, hence T): blockIdx.z selects the window.
__global__ __launch_bounds__(256) void multi_stft_kernel(const float* __restrict__ wav, int L, int T, int hop,
                                                         const float2* __restrict__ tw2k, MultiStftArgs a) {
    __shared__ float2 A[2048], Bf[2048], TW[2048];
    const int t = blockIdx.x, b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    for (int i = tid; i < 2048; i += 256) TW[i] = tw2k[i];
    __syncthreads();
    const int N = a.n_fft[z];
    const float* w = wav + (size_t)b * L;
    const size_t row = ((size_t)b * T + t) * (N / 2 + 1);
    switch (N) {
        case 256: stft_frame<256>(w, L, hop, t, row, TW, A, Bf, a.mag[z], a.cosv[z], a.sinv[z], tid); break;
        case 512: stft_frame<512>(w, L, hop, t, row, TW, A, Bf, a.mag[z], a.cosv[z], a.sinv[z], tid); break;
        case 1024: stft_frame<1024>(w, L, hop, t, row, TW, A, Bf, a.mag[z], a.cosv[z], a.sinv[z], tid); break;
        default: stft_frame<2048>(w, L, hop, t, row, TW, A, Bf, a.mag[z], a.cosv[z], a.sinv[z], tid); break;
    }
}

// ---- clip forms -----------------------------------------------------------------------------------------------------------
// The two ends of the network, stft2_kernel and istft2_kernel below, are each ONE body.  What a launch's clips are is a type,
// resolved when the kernel is instantiated, that answers the few questions in which the forms differ: where clip b's row is,
// how many samples and frames it has, and which of its output samples the iSTFT stores.  Every form therefore runs the same
// arithmetic in the same order, and a clip of any form is bit-identical to that clip run alone through the dense form.
//   DenseClips  (lass_separate): rows L samples apart, every clip L samples and the launch's T frames long.
//   RaggedClips (lass_separate_ragged): the same rows with a length per clip (`lengths`, device int32).  Clips whose lengths
//       fall in one 32-frame bucket share every launch between the two ends: the U-Net sees a (Tpad, n_fft/2) image per clip
//       whatever its length.  What differs per clip is where the reflect padding turns round, how many rows of x0 are real,
//       and what the iSTFT overlap-adds and trims; beyond a clip's frames x0 and the spectra are 0, beyond its samples the
//       waveform is 0.  `lo` is the smallest length of L's bucket: a length outside [lo, L] is clamped into it, so a wrong
//       entry gives a wrong clip, never an access out of range.
//   WindowClips (lass_separate_windows): window b is recording[s_b, s_b + W), a clip that starts at an arbitrary offset of ONE
//       long row, and of its W output samples only [lo_b, hi_b) are stored, at the same offset of one long output row; s_b
//       from `starts` (device int64), (lo_b, hi_b) from `keep` (device int32 pairs, read by the iSTFT alone).  Entries are
//       clamped - s_b into [0, total - W], lo_b into [0, W], hi_b into [lo_b, W] - so a wrong entry gives wrong audio, never
//       an access out of range.
//   FadedWindowClips (lass_separate_windows_faded): WindowClips whose kept range may begin with a fade-in region and end with a
//       fade-out region of up to F samples (`fade`: device int32 flag pairs; `ramp`: device f32 (F), ascending).  A sample of
//       a region is not stored: its product with the ramp weight is ADDED to the output row, where the neighbouring window's
//       complementary region adds the other half of the cross-fade.  The output holds 0 there beforehand, and two adds onto a
//       zero give the same bits in either order, so the result does not depend on which window arrives first.  The regions
//       are cut to the (clamped) kept range and to each other, so both table indices lie in [0, F) whatever the entries say.
//       The forward side has no such form: a faded window reads its input as WindowClips does.
struct Kept { int lo, hi, zend; };  // of a clip's output row the iSTFT stores samples [lo, hi) and writes [hi, zend) as 0

struct DenseClips {
    int L;
    static constexpr bool kShort = false;    // may a clip have fewer frames than the launch's T?
    static constexpr bool kPartial = false;  // may a span of the iSTFT lie wholly outside what its clip stores?
    static constexpr bool kFaded = false;    // are some kept samples added, weighted, instead of stored?
    template <class P> __device__ P* row(P* base, int b) const { return base + (size_t)b * L; }
    __device__ int len(int) const { return L; }
    __device__ int frames(int, int T, int) const { return T; }
    __device__ Kept kept(int, int) const { return {0, L, L}; }
};

struct RaggedClips {
    const int* __restrict__ lengths;
    int lo, L;
    static constexpr bool kShort = true, kPartial = true, kFaded = false;
    template <class P> __device__ P* row(P* base, int b) const { return base + (size_t)b * L; }
    __device__ int len(int b) const {
        const int v = lengths[b];
        return v < lo ? lo : (v > L ? L : v);
    }
    __device__ int frames(int Lb, int, int hop) const { return 1 + Lb / hop; }
    __device__ Kept kept(int, int Lb) const { return {0, Lb, L}; }
};

struct WindowClips {
    const int64_t* __restrict__ starts;
    const int* __restrict__ keep;
    int64_t total;
    int W;
    static constexpr bool kShort = false, kPartial = true, kFaded = false;  // (an empty keep meets no span)
    template <class P> __device__ P* row(P* base, int b) const {
        const int64_t v = starts[b], last = total - W;
        return base + (v < 0 ? 0 : (v > last ? last : v));
    }
    __device__ int len(int) const { return W; }
    __device__ int frames(int, int T, int) const { return T; }
    __device__ Kept kept(int b, int) const {
        int lo = keep[2 * b], hi = keep[2 * b + 1];
        lo = lo < 0 ? 0 : (lo > W ? W : lo);
        hi = hi < lo ? lo : (hi > W ? W : hi);
        return {lo, hi, hi};
    }
};

// of a kept range [lo, hi): [lo, in_end) fades in with ramp[n - lo], [out_begin, hi) fades out with ramp[hi - 1 - n]
struct Fades { int in_end, out_begin; };

struct FadedWindowClips : WindowClips {
    const int* __restrict__ fade;
    const float* __restrict__ ramp;
    int F;  // 1 <= F <= W (the launcher refuses anything else)
    static constexpr bool kFaded = true;
    __device__ Fades fades(int b, const Kept& kp) const {
        const int in_end = fade[2 * b] != 0 ? (kp.hi - kp.lo < F ? kp.hi : kp.lo + F) : kp.lo;
        int out_begin = kp.hi;
        if (fade[2 * b + 1] != 0) out_begin = kp.hi - F < in_end ? in_end : kp.hi - F;
        return {in_end, out_begin};
    }
};

// ---- generic pair-packed transforms (n_fft in {1024, 2048}, window length <= n_fft) ---------------------------------
// A real frame needs only half a complex transform: two frames ride in one complex FFT (frame a in the real part, frame b
// in the imaginary part) and are separated by the Hermitian symmetry of their spectra:
//     Z = FFT(xa + i xb):   Xa[k] = (Z[k] + conj(Z[N-k])) / 2,   Xb[k] = (Z[k] - conj(Z[N-k])) / (2i)
// and the other way round for the inverse.  Twiddles and the periodic Hann window come from the 2048-entry table.
struct Stft2Args {
    int nbr;
    int wlen[LASS_MAX_STFT_WINDOWS];
    float* mag[LASS_MAX_STFT_WINDOWS];
    float* cosv[LASS_MAX_STFT_WINDOWS];
    float* sinv[LASS_MAX_STFT_WINDOWS];
    float* real[LASS_MAX_STFT_WINDOWS];
    float* imag[LASS_MAX_STFT_WINDOWS];
    float* x0[LASS_MAX_STFT_WINDOWS];
    static constexpr bool kMasked = false;
};
// ... of the masked transform (lass_launch_masked_stft): the spectrum of branch 0 is multiplied by the complex mask m_re + i m_im,
// (B, T, N/2+1) as the spectra, before it is stored to real / imag; nothing else is computed.  A type of its own, so that the
// kernels instantiated on Stft2Args keep their argument block and their code.
struct MaskedStft2Args : Stft2Args {
    const float* m_re;
    const float* m_im;
    static constexpr bool kMasked = true;
};

// X * M as torch float32 elementwise ops restate it: four products and two sums, each rounded once.  (The pragma, as in
// export.hip's Mix: the toolchain's __fmul_rn / __fadd_rn are plain * and +, which HIP's default -ffp-contract=fast fuses.)
__device__ __forceinline__ float2 masked_product(float re, float im, float mr, float mi) {
#pragma clang fp contract(off)
    const float a = re * mr, b = im * mi, c = re * mi, d = im * mr;
    return make_float2(a - b, c + d);
}

// Centred, reflect-padded STFT of frames (2*blockIdx.x, 2*blockIdx.x + 1) of clip blockIdx.y for branch blockIdx.z
// (periodic Hann of wlen samples zero-padded to N, centred), fused with magnitude / phase and the network-input prologue
// x0 = bn0(mag) with T zero-padded to Tpad and the Nyquist bin dropped (resunet.py:533-552).  Of a clip of Tb <= T frames,
// rows Tb <= t < Tpad of x0 and rows Tb <= t < T of mag / cos / sin / real / imag are 0 (no such spectrum rows where the form
// gives Tb = T), and nothing of the clip's row is read at or beyond its length.
// MAGPHASE: torchlibrosa magphase (clamp on |X|, precompute_stfts.py:51) instead of base.py:83-88 (clamp on |X|^2).
// Args = MaskedStft2Args: the same transform with a masked epilogue instead - Y = X * M stored to real / imag as
// Y_re = fl(fl(X_re M_re) - fl(X_im M_im)), Y_im = fl(fl(X_re M_im) + fl(X_im M_re)): four products and two sums, each rounded once
// (masked_product), no magnitude, no phase, no x0.  Rows beyond a short clip's frames are zeros as above.
template <int N, bool MAGPHASE, class Clips, class Args = Stft2Args>
__global__ __launch_bounds__(256) void stft2_kernel(const float* __restrict__ wav, Clips clips, int hop, int T, int Tpad,
                                                    const float2* __restrict__ tw2k, Args a,
                                                    const float* __restrict__ s0, const float* __restrict__ h0) {
    __shared__ float2 A[N], Bf[N], TW[2048];
    constexpr int NB = N / 2 + 1, FC = N / 2;
    const int ta = 2 * blockIdx.x, b = blockIdx.y, z = blockIdx.z, tid = threadIdx.x;
    const int Lb = clips.len(b), Tb = clips.frames(Lb, T, hop);
    float* x0 = a.x0[z];
    // rows from `from` of this frame pair lie beyond the clip: zeros in the network input (AFTER bn0) and in the spectra
    const auto zero_rows = [&](int from) {
        for (int t = from; t < ta + 2; ++t) {
            if (x0 && t < Tpad)
                for (int f = tid; f < FC; f += 256) x0[((size_t)b * Tpad + t) * FC + f] = 0.f;
            if (Clips::kShort && t < T) {
                float *mag = a.mag[z], *cosv = a.cosv[z], *sinv = a.sinv[z], *real = a.real[z], *imag = a.imag[z];
                for (int f = tid; f < NB; f += 256) {
                    const size_t row = ((size_t)b * T + t) * NB + f;
                    if (real) real[row] = 0.f;
                    if (imag) imag[row] = 0.f;
                    if (mag) mag[row] = 0.f;
                    if (cosv) cosv[row] = 0.f;
                    if (sinv) sinv[row] = 0.f;
                }
            }
        }
    };
    if (ta >= Tb) {
        zero_rows(ta);
        return;
    }
    for (int i = tid; i < 2048; i += 256) TW[i] = tw2k[i];
    __syncthreads();
    const int wlen = a.wlen[z], woff = (N - wlen) / 2, wstride = 2048 / wlen;
    const float* w = clips.row(wav, b);
    const bool have_b = ta + 1 < Tb;
    for (int idx = tid; idx < N; idx += 256) {
        float2 v = make_float2(0.f, 0.f);
        const int j = idx - woff;
        if (j >= 0 && j < wlen) {
            const float wn = 0.5f - 0.5f * TW[j * wstride].x;  // periodic Hann of wlen
            const int n = ta * hop + idx - N / 2;
            v = make_float2(w[reflect(n, Lb)] * wn, have_b ? w[reflect(n + hop, Lb)] * wn : 0.f);
        }
        A[idx] = v;
    }
    __syncthreads();
#ifdef LASS_STFT_DBG
    float2* dbg = g_stft_dbg ? g_stft_dbg + (size_t)((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 5 * 3 * N : nullptr;
    const float2* Z = fft_c<N, false>(A, Bf, TW, tid, dbg);
#else
    const float2* Z = fft_c<N, false>(A, Bf, TW, tid);
#endif
    float *mag = a.mag[z], *cosv = a.cosv[z], *sinv = a.sinv[z], *real = a.real[z], *imag = a.imag[z];
    for (int f = tid; f < NB; f += 256) {
        const float2 z1 = Z[f], z2 = Z[(N - f) & (N - 1)];
        const float re[2] = {0.5f * (z1.x + z2.x), 0.5f * (z1.y + z2.y)};
        const float im[2] = {0.5f * (z1.y - z2.y), -0.5f * (z1.x - z2.x)};
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !have_b) break;
            const size_t row = ((size_t)b * T + ta + r) * NB + f;
            if constexpr (Args::kMasked) {
                const float2 y = masked_product(re[r], im[r], a.m_re[row], a.m_im[row]);
                real[row] = y.x;
                imag[row] = y.y;
                continue;
            }
            float m, c, s;
            if (MAGPHASE) {
                m = sqrtf(re[r] * re[r] + im[r] * im[r]);
                const float den = fmaxf(m, 1e-10f);
                c = re[r] / den; s = im[r] / den;
            } else {
                m = sqrtf(fmaxf(re[r] * re[r] + im[r] * im[r], 1e-10f));
                c = re[r] / m; s = im[r] / m;
            }
            if (real) real[row] = re[r];
            if (imag) imag[row] = im[r];
            if (mag) mag[row] = m;
            if (cosv) cosv[row] = c;
            if (sinv) sinv[row] = s;
            if (x0 && f < FC) x0[((size_t)b * Tpad + ta + r) * FC + f] = m * s0[f] + h0[f];
        }
    }
    if (!have_b) zero_rows(ta + 1);
}

// Inverse STFT, fused: a workgroup owns SPAN consecutive samples of the (n_fft/2-padded) output, runs the inverse
// transforms of every frame of the clip whose window reaches into that span (two frames per complex transform) and
// overlap-adds them in LDS in ascending frame order, then divides by the window-sum-square envelope of the same frames
// (clamped at 1e-11) and writes the samples the form keeps, n_fft/2 trimmed (zeros where it says so: sums over a padded
// ragged row gain only exact zeros).  No frame scratch in HBM.  A span that meets nothing its clip stores writes its zeros
// and returns before it loads a twiddle: with a second of context either side of a five-second window that is two spans in
// five.
// SPAN is a property of the STFT geometry (its hop): the LDS of a workgroup is A + Bf + TW = 24 * N bytes plus acc + env = 8 bytes
// per span sample, and a span of S samples runs the (S + wlen) / hop frames that reach into it for the S / hop that start in it.
//   hop 160: 16 hops = 2 560 samples - 44 KiB at N = 1024 (three workgroups per CU), 68 KiB at N = 2048 (two).
//   hop 320: kIstftSpanHops320 hops.  8 hops = the same 2 560 samples and 68 KiB: two workgroups per CU, (8 + 6.4) / 8 = 1.8 x
//            redundant transforms.  16 hops = 5 120 samples and 88 KiB: one workgroup per CU, 1.4 x.  Measured on an MI355X at
//            B = 16, L = 320 000 (tools/geometry_bench.py --istft): 8 hops 0.214 ms, 16 hops 0.293 ms -
//            8 ships; the build-time override below exists for that measurement alone.
// The frames of a span are visited in ascending order whatever the span, and a sample's sum never leaves its span: the value of
// a sample does not depend on the clip form, only (through the pairing of frames) on the span constant.
#ifndef LASS_ISTFT_SPAN_HOPS_320
#define LASS_ISTFT_SPAN_HOPS_320 8
#endif
constexpr int kIstftSpanHops320 = LASS_ISTFT_SPAN_HOPS_320;
constexpr int kIstftSpan160 = 16 * LASS_HOP;
constexpr int kIstftSpan320 = kIstftSpanHops320 * 320;
static_assert(kIstftSpanHops320 == 8 || kIstftSpanHops320 == 16, "8 or 16 hops per span at hop 320");

template <int N, int ISTFT_SPAN, class Clips>
__global__ __launch_bounds__(256) void istft2_kernel(const float* __restrict__ real, const float* __restrict__ imag,
                                                     Clips clips, int T, int hop, int wlen,
                                                     const float2* __restrict__ tw2k, float* __restrict__ out) {
    __shared__ float2 A[N], Bf[N], TW[2048];
    __shared__ float acc[ISTFT_SPAN], env[ISTFT_SPAN];
    constexpr int NB = N / 2 + 1;
    const int b = blockIdx.y, tid = threadIdx.x;
    const int m0 = blockIdx.x * ISTFT_SPAN;  // first padded position of this span
    const int Lb = clips.len(b), Tb = clips.frames(Lb, T, hop);
    const Kept kp = clips.kept(b, Lb);
    float* wav = clips.row(out, b);
    if (Clips::kPartial && (m0 - N / 2 >= kp.hi || m0 + ISTFT_SPAN - N / 2 <= kp.lo)) {
        for (int i = tid; i < ISTFT_SPAN; i += 256) {
            const int n = m0 + i - N / 2;
            if (n >= kp.hi && n < kp.zend) wav[n] = 0.f;
        }
        return;
    }
    const int woff = (N - wlen) / 2, wstride = 2048 / wlen;
    for (int i = tid; i < 2048; i += 256) TW[i] = tw2k[i];
    for (int i = tid; i < ISTFT_SPAN; i += 256) { acc[i] = 0.f; env[i] = 0.f; }
    // frames whose window support [t*hop + woff, t*hop + woff + wlen) meets [m0, m0 + SPAN)
    int t_lo = m0 - woff - wlen + 1;
    t_lo = t_lo <= 0 ? 0 : (t_lo + hop - 1) / hop;
    int t_hi = (m0 + ISTFT_SPAN - 1 - woff) / hop;
    if (m0 + ISTFT_SPAN - 1 - woff < 0) t_hi = -1;
    if (t_hi > Tb - 1) t_hi = Tb - 1;
    __syncthreads();
    for (int ta = t_lo; ta <= t_hi; ta += 2) {
        const bool have_b = ta + 1 <= t_hi;
        const size_t rowa = ((size_t)b * T + ta) * NB, rowb = rowa + NB;
        // Z = Xa + i Xb with both spectra Hermitian-extended: bin k > N/2 is the conjugate of bin N-k
        for (int k = tid; k < N; k += 256) {
            const int kk = k <= N / 2 ? k : N - k;
            // bins 0 and N/2 of a real frame's spectrum are real: their imaginary parts are ignored (sin(0) = sin(pi n)
            // = 0 in the reference's inverse-DFT matrix) - and must not leak into the partner frame of the packed pair
            const float sg = (kk == 0 || kk == N / 2) ? 0.f : (k <= N / 2 ? 1.f : -1.f);
            const float ar = real[rowa + kk], ai = sg * imag[rowa + kk];
            const float br = have_b ? real[rowb + kk] : 0.f, bi = have_b ? sg * imag[rowb + kk] : 0.f;
            A[k] = make_float2(ar - bi, ai + br);
        }
        __syncthreads();
        const float2* X = fft_c<N, true>(A, Bf, TW, tid);  // (xa, xb) * N
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            if (r == 1 && !have_b) break;
            const int base = (ta + r) * hop + woff - m0;  // span position of window sample 0
            for (int j = tid; j < wlen; j += 256) {
                const int pos = base + j;
                if (pos >= 0 && pos < ISTFT_SPAN) {
                    const float wn = 0.5f - 0.5f * TW[j * wstride].x;
                    const float2 x = X[woff + j];
                    acc[pos] += (r == 0 ? x.x : x.y) * (wn * (1.0f / N));
                    env[pos] += wn * wn;
                }
            }
            __syncthreads();
        }
    }
    if constexpr (Clips::kFaded) {
        // (the span early-out above stands: both regions lie inside [lo, hi).)  __fmul_rn: nothing contracts into the product
        const Fades fd = clips.fades(b, kp);
        for (int i = tid; i < ISTFT_SPAN; i += 256) {
            const int n = m0 + i - N / 2;
            if (n < kp.lo || n >= kp.hi) continue;
            const float y = acc[i] / fmaxf(env[i], 1e-11f);
            if (n < fd.in_end) atomicAdd(wav + n, __fmul_rn(clips.ramp[n - kp.lo], y));
            else if (n >= fd.out_begin) atomicAdd(wav + n, __fmul_rn(clips.ramp[kp.hi - 1 - n], y));
            else wav[n] = y;
        }
    } else {
        for (int i = tid; i < ISTFT_SPAN; i += 256) {
            const int n = m0 + i - N / 2;
            if (n >= kp.lo && n < kp.hi) wav[n] = acc[i] / fmaxf(env[i], 1e-11f);
            else if (n >= kp.hi && n < kp.zend) wav[n] = 0.f;
        }
    }
}

// The smallest length that shares a 32-frame bucket with L: max(hop * (Tpad - 32), n_fft / 2 + 1).
int ragged_lo(int L, int n_fft, int hop) {
    const int T = 1 + L / hop, Tpad = (T + 31) / 32 * 32;
    const int a = hop * (Tpad - 32), b = n_fft / 2 + 1;
    return a > b ? a : b;
}

// f(clips) with the device-side form of cf: the window form where it has starts, the ragged form where it has lengths.  kFades:
// the faded window form where cf has flags as well - the iSTFT's; what a window stores or adds is no business of the forward
// side, which reads a faded window as WindowClips (and instantiates nothing new).
template <bool kFades, class F>
void with_clips(const ClipForm& cf, int n_fft, int hop, F f) {
    if constexpr (kFades) {
        if (cf.starts && cf.fade) {
            f(FadedWindowClips{{cf.starts, cf.keep, cf.total, cf.L}, cf.fade, cf.ramp, cf.F});
            return;
        }
    }
    if (cf.starts) f(WindowClips{cf.starts, cf.keep, cf.total, cf.L});
    else if (cf.lengths) f(RaggedClips{cf.lengths, ragged_lo(cf.L, n_fft, hop), cf.L});
    else f(DenseClips{cf.L});
}

// mag = cos = 1, sin = 0 over n floats each: the unit spectrum that turns the output head's product into the mask itself
__global__ __launch_bounds__(256) void unit_spectrum_kernel(float* __restrict__ mag, float* __restrict__ cosv, float* __restrict__ sinv,
                                                            size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        mag[i] = 1.f;
        cosv[i] = 1.f;
        sinv[i] = 0.f;
    }
}

bool bad_transform(int n_fft, int wlen) {
    return (n_fft != 1024 && n_fft != 2048) || wlen <= 0 || wlen > n_fft || (2048 % wlen) != 0 || ((n_fft - wlen) & 1);
}

}  // namespace

hipError_t lass_launch_multi_stft(const float* wav, int B, int L, int hop, int nwin, const int* n_fft,
                                  const float2* tw2k, float* const* mag, float* const* cosv, float* const* sinv,
                                  hipStream_t stream) {
    if (B <= 0 || hop <= 0 || nwin <= 0 || nwin > LASS_MAX_STFT_WINDOWS) return hipErrorInvalidValue;
    MultiStftArgs a;
    a.nwin = nwin;
    for (int i = 0; i < nwin; ++i) {
        const int N = n_fft[i];
        if ((N != 256 && N != 512 && N != 1024 && N != 2048) || L <= N / 2 || !mag[i] || !cosv[i] || !sinv[i])
            return hipErrorInvalidValue;
        a.n_fft[i] = N; a.mag[i] = mag[i]; a.cosv[i] = cosv[i]; a.sinv[i] = sinv[i];
    }
    const int T = 1 + L / hop;
    hipLaunchKernelGGL(multi_stft_kernel, dim3(T, B, nwin), dim3(256), 0, stream, wav, L, T, hop, tw2k, a);
    return hipGetLastError();
}

hipError_t lass_launch_stft2(const float* wav, const ClipForm& cf, int n_fft, int hop, int T, int Tpad, int nbr,
                             const StftBranch* br, int magphase_sem, const float* s0, const float* h0,
                             const float2* tw2k, hipStream_t stream) {
    const int B = cf.B, L = cf.L;
    if (B <= 0 || hop <= 0 || nbr <= 0 || nbr > LASS_MAX_STFT_WINDOWS || (n_fft != 1024 && n_fft != 2048) ||
        L <= n_fft / 2 || T != 1 + L / hop)
        return hipErrorInvalidValue;
    if (cf.starts ? (!wav || cf.total < L || Tpad < T) : cf.lengths ? Tpad != (T + 31) / 32 * 32 : Tpad < T)
        return hipErrorInvalidValue;
    Stft2Args a;
    a.nbr = nbr;
    bool any_x0 = false;
    for (int i = 0; i < nbr; ++i) {
        if (bad_transform(n_fft, br[i].wlen)) return hipErrorInvalidValue;
        if (br[i].x0 && (!s0 || !h0)) return hipErrorInvalidValue;
        any_x0 |= br[i].x0 != nullptr;
        a.wlen[i] = br[i].wlen; a.mag[i] = br[i].mag; a.cosv[i] = br[i].cosv; a.sinv[i] = br[i].sinv;
        a.real[i] = br[i].real; a.imag[i] = br[i].imag; a.x0[i] = br[i].x0;
    }
    dim3 grid(((any_x0 ? Tpad : T) + 1) / 2, B, nbr);
    with_clips<false>(cf, n_fft, hop, [&](auto clips) {
        using C = decltype(clips);
        const auto kernel = n_fft == 1024 ? (magphase_sem ? stft2_kernel<1024, true, C> : stft2_kernel<1024, false, C>)
                                          : (magphase_sem ? stft2_kernel<2048, true, C> : stft2_kernel<2048, false, C>);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, wav, clips, hop, T, Tpad, tw2k, a, s0, h0);
    });
    return hipGetLastError();
}

hipError_t lass_launch_masked_stft(const float* wav, const ClipForm& cf, int n_fft, int hop, int T, int wlen, const float* m_re,
                                   const float* m_im, float* y_re, float* y_im, const float2* tw2k, hipStream_t stream) {
    const int B = cf.B, L = cf.L;
    if (!wav || !m_re || !m_im || !y_re || !y_im || B <= 0 || hop <= 0 || L <= n_fft / 2 || T != 1 + L / hop || bad_transform(n_fft, wlen))
        return hipErrorInvalidValue;
    if (cf.starts && cf.total < L) return hipErrorInvalidValue;
    MaskedStft2Args a = {};
    a.nbr = 1;
    a.wlen[0] = wlen; a.real[0] = y_re; a.imag[0] = y_im;
    a.m_re = m_re; a.m_im = m_im;
    dim3 grid((T + 1) / 2, B, 1);
    with_clips<false>(cf, n_fft, hop, [&](auto clips) {
        using C = decltype(clips);
        const auto kernel = n_fft == 1024 ? stft2_kernel<1024, false, C, MaskedStft2Args> : stft2_kernel<2048, false, C, MaskedStft2Args>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, wav, clips, hop, T, T, tw2k, a, (const float*)nullptr, (const float*)nullptr);
    });
    return hipGetLastError();
}

hipError_t lass_launch_unit_spectrum(float* mag, float* cosv, float* sinv, size_t n, hipStream_t stream) {
    if (!mag || !cosv || !sinv || n == 0) return hipErrorInvalidValue;
    const size_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(unit_spectrum_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, stream, mag, cosv, sinv, n);
    return hipGetLastError();
}

hipError_t lass_launch_istft2(const float* real, const float* imag, const ClipForm& cf, int T, int n_fft, int wlen, int hop,
                              const float2* tw2k, float* wav, hipStream_t stream) {
    const int B = cf.B, L = cf.L;
    // the two geometries: hop 160 at either transform size, hop 320 at n_fft 2048
    if (B <= 0 || (hop != LASS_HOP && !(hop == 320 && n_fft == 2048)) || bad_transform(n_fft, wlen)) return hipErrorInvalidValue;
    if (cf.starts || cf.lengths ? (L <= n_fft / 2 || T != 1 + L / hop) : (T <= 0 || L <= 0)) return hipErrorInvalidValue;
    if (cf.starts && (!cf.keep || !wav || cf.total < L)) return hipErrorInvalidValue;
    if (cf.fade && (!cf.starts || !cf.ramp || cf.F < 1 || cf.F > L)) return hipErrorInvalidValue;
    const int span = hop == LASS_HOP ? kIstftSpan160 : kIstftSpan320;
    dim3 grid((n_fft / 2 + L + span - 1) / span, B);
    with_clips<true>(cf, n_fft, hop, [&](auto clips) {
        using C = decltype(clips);
        const auto kernel = n_fft == 1024      ? istft2_kernel<1024, kIstftSpan160, C>
                            : hop == LASS_HOP ? istft2_kernel<2048, kIstftSpan160, C>
                                              : istft2_kernel<2048, kIstftSpan320, C>;
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, real, imag, clips, T, hop, wlen, tw2k, wav);
    });
    return hipGetLastError();
}

#ifdef LASS_STFT_DBG
// diagnostic build: the record buffer of the NEXT stft2_kernel launches on `stream` (nullptr = off)
extern "C" int lass_dbg_stft_buffer(void* buf, hipStream_t stream) {
    float2* pbuf = (float2*)buf;
    return (int)hipMemcpyToSymbolAsync(HIP_SYMBOL(g_stft_dbg), &pbuf, sizeof(pbuf), 0, hipMemcpyHostToDevice, stream);
}
#endif
