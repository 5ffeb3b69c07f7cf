// loudness.hip - the ITU-R BS.1770-4 integrated-loudness meter on planar float32 recordings, and the gain rule of the levelled
// export.  lass_amd/loudness.py is the float64 definition; DESIGN.md section 18.
//
// K-weighting is two biquads in direct form II transposed, i.e. a 4-state affine recurrence s[n+1] = M s[n] + v x[n] that is
// serial in time, on B * C planes (a handful) of millions of samples.  The time axis is cut instead:
//   hop bin  = H = rate/10 consecutive samples of a plane (a 400 ms block is four bins), one WAVE each;
//   lane run = S = H / nl consecutive samples of the bin, one lane each (nl: the largest divisor of H up to 64).
// k_bins<false>: every lane runs its samples from a zero state; lane 0 carries the states over the lane runs with M^S; the bin's
//                zero-state end state goes to memory.
// k_carry:       one thread per plane carries the states over the bins with M^H (both powers are the host's, in float64).
// k_bins<true>:  the same two steps from the bin's true initial state, then every lane reruns its samples from its true state
//                and sums y^2; lane 0 adds the lane sums in lane order.
// k_gate:        one workgroup per recording: block powers from four consecutive bin sums, then the two gates, each one
//                strided sum per thread and one LDS tree.
// k_range:       (lass_loudness_stats alone) one workgroup per recording: short-term powers from thirty consecutive bin sums, the
//                maxima of both kinds of block, EBU Tech 3342's two gates, and the 10th and 95th percentile by an exact radix
//                select on the powers' bit patterns.  DESIGN.md section 19.
// A wave reads its bin into LDS with consecutive lanes on consecutive floats (the lanes' own runs lie S floats apart, which no
// load instruction coalesces); a lane's run sits at pitch S | 1 so the lanes spread over the banks.  State, products and sums
// are float64.  Every chunk boundary is a multiple of H from the plane's first sample and every sum has one order, so a
// recording's numbers do not depend on the batch, its row, the strides or the call; there is no floating-point atomic.
#include <cmath>

#include "../../include/lass_hip.h"
#include "kernels.h"

namespace {

constexpr int kWave = 64;

struct State {
    double s[4];
};

// one sample through both stages; c = b0 b1 b2 a1 a2 of stage 1, then of stage 2
__host__ __device__ __forceinline__ double advance(State& z, const LoudnessFilter& f, double x) {
    const double* c = f.coef;
    const double y1 = c[0] * x + z.s[0];
    z.s[0] = c[1] * x - c[3] * y1 + z.s[1];
    z.s[1] = c[2] * x - c[4] * y1;
    const double y2 = c[5] * y1 + z.s[2];
    z.s[2] = c[6] * y1 - c[8] * y2 + z.s[3];
    z.s[3] = c[7] * y1 - c[9] * y2;
    return y2;
}

__device__ __forceinline__ State carry(const double* m, const State& s, const State& z) {
    State r;
    for (int i = 0; i < 4; ++i) r.s[i] = ((m[4 * i] * s.s[0] + m[4 * i + 1] * s.s[1]) + (m[4 * i + 2] * s.s[2] + m[4 * i + 3] * s.s[3])) + z.s[i];
    return r;
}

__device__ __forceinline__ int clamp_len(const int* lengths, int b, int L) {
    const int n = lengths ? lengths[b] : L;
    return n < 0 ? 0 : (n > L ? L : n);
}

// grid (bins of the longest plane, B * C), one wave per workgroup.  states[plane][bin] = the bin's zero-state end state
// (kFinal false, written) or its true initial state (kFinal true, read); sums[plane][bin] = the bin's sum of y^2 (kFinal true).
template <bool kFinal>
__global__ __launch_bounds__(kWave) void k_bins(const float* __restrict__ planes, long long row_stride, long long plane_stride,
                                                int ch, int L, const int* __restrict__ lengths, int H, int nl, int S, int bins_max,
                                                LoudnessFilter f, State* __restrict__ states, double* __restrict__ sums) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x, bin = blockIdx.x, plane = blockIdx.y;
    const int b = plane / ch, c = plane - b * ch;
    const int bins = clamp_len(lengths, b, L) / H;
    // the last bin's end state carries into nothing
    if (kFinal ? bin >= bins : bin + 1 >= bins) return;
    const int Sp = S | 1;
    float* xs = lds;                                                        // [nl][Sp]
    State* zs = reinterpret_cast<State*>(lds + (((size_t)nl * Sp + 3) & ~(size_t)3));   // [nl]
    double* part = reinterpret_cast<double*>(zs + nl);                      // [nl]
    const float* x = planes + (size_t)b * row_stride + (size_t)c * plane_stride + (size_t)bin * H;
    for (int e = lane; e < H; e += kWave) {
        const int i = e / S;
        xs[i * Sp + (e - i * S)] = x[e];
    }
    __syncthreads();
    const float* mine = xs + lane * Sp;
    State z = {{0.0, 0.0, 0.0, 0.0}};
    if (lane < nl) {
        for (int k = 0; k < S; ++k) advance(z, f, (double)mine[k]);
        zs[lane] = z;
    }
    __syncthreads();
    State* st = states + (size_t)plane * bins_max + bin;
    if (lane == 0) {
        State s = {{0.0, 0.0, 0.0, 0.0}};
        if (kFinal) s = *st;
        for (int i = 0; i < nl; ++i) {                                      // zs[i]: zero-state end -> true initial state
            const State zi = zs[i];
            zs[i] = s;
            s = carry(f.lane_step, s, zi);
        }
        if (!kFinal) *st = s;
    }
    if (!kFinal) return;
    __syncthreads();
    if (lane < nl) {
        z = zs[lane];
        double acc = 0.0;
        for (int k = 0; k < S; ++k) {
            const double y = advance(z, f, (double)mine[k]);
            acc += y * y;
        }
        part[lane] = acc;
    }
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int i = 0; i < nl; ++i) acc += part[i];
        sums[(size_t)plane * bins_max + bin] = acc;
    }
}

// states[plane][bin]: zero-state end states -> true initial states
__global__ void k_carry(int planes, int ch, int L, const int* __restrict__ lengths, int H, int bins_max, LoudnessFilter f,
                        State* __restrict__ states) {
    const int plane = blockIdx.x * blockDim.x + threadIdx.x;
    if (plane >= planes) return;
    const int bins = clamp_len(lengths, plane / ch, L) / H;
    State* st = states + (size_t)plane * bins_max;
    State s = {{0.0, 0.0, 0.0, 0.0}};
    for (int j = 0; j < bins; ++j) {
        if (j + 1 < bins) {          // (the last bin's end state was not written, and carries into nothing)
            const State zj = st[j];
            st[j] = s;
            s = carry(f.bin_step, s, zj);
        } else {
            st[j] = s;
        }
    }
}

constexpr int kGateThreads = 256;

// sum over the workgroup in one fixed tree; every thread gets the result
__device__ __forceinline__ double tree_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kGateThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// one workgroup per recording.  out[b * out_pitch] ... = {integrated loudness, blocks, blocks that pass both gates}
__global__ __launch_bounds__(kGateThreads) void k_gate(const double* __restrict__ sums, int ch, int L, const int* __restrict__ lengths,
                                                       int H, int bins_max, const float* __restrict__ weights,
                                                       double* __restrict__ out, int out_pitch, double* __restrict__ blocks, int nb_max) {
    __shared__ double red[kGateThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int bins = clamp_len(lengths, b, L) / H;
    const int nb = bins >= 4 ? bins - 3 : 0;
    const double T = 4.0 * (double)H;
    auto power = [&](int j) {
        double p = 0.0;
        for (int c = 0; c < ch; ++c) {
            const double* s = sums + ((size_t)b * ch + c) * bins_max + j;
            const double ms = (((s[0] + s[1]) + s[2]) + s[3]) / T;
            p += (weights ? (double)weights[c] : 1.0) * ms;
        }
        return p;
    };
    auto lufs = [](double p) { return -0.691 + 10.0 * log10(p); };
    if (blocks)
        for (int j = tid; j < nb_max; j += kGateThreads) blocks[(size_t)b * nb_max + j] = j < nb ? power(j) : 0.0;
    double sum = 0.0, cnt = 0.0;
    for (int j = tid; j < nb; j += kGateThreads) {
        const double p = power(j);
        if (lufs(p) > -70.0) { sum += p; cnt += 1.0; }
    }
    sum = tree_sum(sum, red);
    cnt = tree_sum(cnt, red);
    double kept = 0.0, loud = -INFINITY;
    if (cnt > 0.0) {
        const double rel = lufs(sum / cnt) - 10.0;
        double sum2 = 0.0, cnt2 = 0.0;
        for (int j = tid; j < nb; j += kGateThreads) {
            const double p = power(j), l = lufs(p);
            if (l > -70.0 && l > rel) { sum2 += p; cnt2 += 1.0; }
        }
        sum2 = tree_sum(sum2, red);
        kept = tree_sum(cnt2, red);
        if (kept > 0.0) loud = lufs(sum2 / kept);
    }
    if (tid == 0) {
        out[(size_t)out_pitch * b] = loud;
        out[(size_t)out_pitch * b + 1] = (double)nb;
        out[(size_t)out_pitch * b + 2] = kept;
    }
}

// ---- EBU R 128 beside the integrated loudness (lass_loudness_stats) --------------------------------------
constexpr int kShortBins = 30;          // a 3 s short-term block in hop bins

// maximum over the workgroup; every thread gets the result (exact whatever the order)
__device__ __forceinline__ double tree_max(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kGateThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x + w] > red[threadIdx.x] ? red[threadIdx.x + w] : red[threadIdx.x];
        __syncthreads();
    }
    return red[0];
}

// The k-th smallest (k from 0) of the n doubles of row v, by their bit patterns (non-negative doubles order as unsigned 64-bit
// integers; a dropped block holds all ones and sorts behind every power): a radix select, most significant byte first, each pass
// one 256-bin histogram of the values that share the bytes found so far.  Integer LDS atomics: exact and order-independent.
__device__ __forceinline__ unsigned long long radix_select(const double* v, int n, unsigned k, unsigned* hist, unsigned long long* found) {
    unsigned long long prefix = 0;
    for (int pass = 7; pass >= 0; --pass) {
        const int shift = 8 * pass;
        const unsigned long long mask = pass == 7 ? 0ull : ~0ull << (shift + 8);
        __syncthreads();
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int j = threadIdx.x; j < n; j += kGateThreads) {
            const unsigned long long bits = (unsigned long long)__double_as_longlong(v[j]);
            if ((bits & mask) == prefix) atomicAdd(hist + (unsigned)((bits >> shift) & 255u), 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned below = 0, d = 0;
            while (d < 255u && k >= below + hist[d]) below += hist[d++];
            found[0] = prefix | ((unsigned long long)d << shift);
            found[1] = k - below;
        }
        __syncthreads();
        prefix = found[0];
        k = (unsigned)found[1];
    }
    return prefix;
}

// one workgroup per recording, after k_gate.  out[b * 10 + 3 ...] = {max momentary, max short-term, LRA, ns, short-term blocks past
// both gates, p10, p95}; st (B, bins_max): the recording's short-term powers, a dropped one replaced by all ones; short_term
// (optional, (B, ns_max)): the powers themselves, 0 past the recording's own count.
__global__ __launch_bounds__(kGateThreads) void k_range(const double* __restrict__ sums, int ch, int L, const int* __restrict__ lengths,
                                                        int H, int bins_max, const float* __restrict__ weights,
                                                        double* __restrict__ out, double* __restrict__ st_all,
                                                        double* __restrict__ short_term, int ns_max) {
    __shared__ double red[kGateThreads];
    __shared__ unsigned hist[kGateThreads];
    __shared__ unsigned long long found[2];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int bins = clamp_len(lengths, b, L) / H;
    const int nb = bins >= 4 ? bins - 3 : 0, ns = bins >= kShortBins ? bins - (kShortBins - 1) : 0;
    double* st = st_all + (size_t)b * bins_max;
    // the channel-weighted mean square of the n bins from bin j on, the bin sums added left to right
    auto power = [&](int j, int n) {
        double p = 0.0;
        for (int c = 0; c < ch; ++c) {
            const double* s = sums + ((size_t)b * ch + c) * bins_max + j;
            double acc = s[0];
            for (int i = 1; i < n; ++i) acc += s[i];
            p += (weights ? (double)weights[c] : 1.0) * (acc / ((double)n * (double)H));
        }
        return p;
    };
    auto lufs = [](double p) { return -0.691 + 10.0 * log10(p); };
    double mom = 0.0, shr = 0.0, sum = 0.0, cnt = 0.0;
    for (int j = tid; j < nb; j += kGateThreads) {
        const double p = power(j, 4);
        mom = p > mom ? p : mom;
    }
    for (int j = tid; j < ns; j += kGateThreads) {           // (thread tid alone touches st[tid + 256 i], here and below)
        const double q = power(j, kShortBins);
        st[j] = q;
        shr = q > shr ? q : shr;
        if (lufs(q) > -70.0) { sum += q; cnt += 1.0; }
    }
    if (short_term)
        for (int j = tid; j < ns_max; j += kGateThreads) short_term[(size_t)b * ns_max + j] = j < ns ? st[j] : 0.0;
    mom = tree_max(mom, red);
    shr = tree_max(shr, red);
    sum = tree_sum(sum, red);
    cnt = tree_sum(cnt, red);
    double kept = 0.0, p10 = 0.0, p95 = 0.0, lra = 0.0;
    if (cnt > 0.0) {                                         // (uniform over the workgroup)
        const double rel = lufs(sum / cnt) - 20.0;
        double cnt2 = 0.0;
        for (int j = tid; j < ns; j += kGateThreads) {
            const double l = lufs(st[j]);
            if (l > -70.0 && l > rel) cnt2 += 1.0;
            else st[j] = __longlong_as_double(-1ll);
        }
        kept = tree_sum(cnt2, red);
        if (kept > 0.0) {
            // floor((n - 1) * 0.10 + 0.5) and the same at 0.95, rounded as the host rounds them (no fused multiply-add)
            const unsigned k10 = (unsigned)floor(__dadd_rn(__dmul_rn(kept - 1.0, 0.10), 0.5));
            const unsigned k95 = (unsigned)floor(__dadd_rn(__dmul_rn(kept - 1.0, 0.95), 0.5));
            p10 = __longlong_as_double((long long)radix_select(st, ns, k10, hist, found));
            p95 = __longlong_as_double((long long)radix_select(st, ns, k95, hist, found));
            lra = 10.0 * log10(p95 / p10);
        }
    }
    if (tid == 0) {
        double* o = out + (size_t)10 * b;
        o[3] = nb ? lufs(mom) : -INFINITY;
        o[4] = ns ? lufs(shr) : -INFINITY;
        o[5] = lra;
        o[6] = (double)ns;
        o[7] = kept;
        o[8] = p10;
        o[9] = p95;
    }
}

__global__ void k_gain(const double* __restrict__ loudness, const float* __restrict__ peak, int B, double target, float ceiling,
                       float* __restrict__ gain, int* __restrict__ limited) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double l = loudness[b];
    float g = 1.0f;
    if (target == target && isfinite(l)) g = (float)pow(10.0, (target - l) / 20.0);
    int bit = 0;
    if (ceiling > 0.0f && peak) {
        const float pk = peak[b];
        if (__fmul_rn(g, pk) > ceiling) {
            bit = 1;
            g = __fdiv_rn(ceiling, pk);
            while (__fmul_rn(g, pk) > ceiling) g = __uint_as_float(__float_as_uint(g) - 1u);    // g > 0 here: one ulp down
        }
    }
    gain[b] = g;
    if (limited) limited[b] = bit;
}

}  // namespace

int lass_loudness_lanes(int hop);

// m <- m^n (4 x 4, row-major), squared and multiplied in long double
static void mat_power(const double* m, long long n, double* out) {
    long double r[16], a[16], t[16];
    for (int i = 0; i < 16; ++i) { r[i] = i % 5 == 0 ? 1.0L : 0.0L; a[i] = m[i]; }
    auto mul = [&](const long double* x, const long double* y, long double* z) {
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                long double v = 0.0L;
                for (int k = 0; k < 4; ++k) v += x[4 * i + k] * y[4 * k + j];
                t[4 * i + j] = v;
            }
        for (int i = 0; i < 16; ++i) z[i] = t[i];
    };
    for (; n > 0; n >>= 1) {
        if (n & 1) mul(r, a, r);
        mul(a, a, a);
    }
    for (int i = 0; i < 16; ++i) out[i] = (double)r[i];
}

bool lass_loudness_filter(const double* coef, int hop, LoudnessFilter* f) {
    for (int i = 0; i < 10; ++i) {
        if (!std::isfinite(coef[i])) return false;
        f->coef[i] = coef[i];
    }
    // both stages' poles strictly inside the unit circle (the stability triangle): the powers of M stay bounded
    for (int s = 0; s < 2; ++s) {
        const double a1 = coef[5 * s + 3], a2 = coef[5 * s + 4];
        if (!(std::fabs(a2) < 1.0 && std::fabs(a1) < 1.0 + a2)) return false;
    }
    double m[16];
    for (int j = 0; j < 4; ++j) {          // column j of M: one silent sample from the unit state e_j
        State e = {{0.0, 0.0, 0.0, 0.0}};
        e.s[j] = 1.0;
        advance(e, *f, 0.0);
        for (int i = 0; i < 4; ++i) m[4 * i + j] = e.s[i];
    }
    mat_power(m, hop / lass_loudness_lanes(hop), f->lane_step);
    mat_power(m, hop, f->bin_step);
    return true;
}

int lass_loudness_lanes(int hop) {
    int nl = hop < kWave ? hop : kWave;
    while (hop % nl) --nl;
    return nl;
}

// The meter up to and including k_gate; out: rows of out_pitch doubles.
static hipError_t launch_meter(const PlaneRows& P, const int* lengths, int hop, const LoudnessFilter& f, const float* weights, double* out,
                               int out_pitch, double* blocks, int nb_max, double* scratch, hipStream_t stream) {
    const int B = P.B, ch = P.ch, L = P.L, bins_max = L / hop;
    if (B <= 0 || ch < 1 || ch > 8 || (long long)B * ch > 65535 || hop < 1 || L < 1) return hipErrorInvalidValue;
    State* states = reinterpret_cast<State*>(scratch);
    double* sums = scratch + (size_t)4 * B * ch * bins_max;
    if (bins_max > 0) {
        const int nl = lass_loudness_lanes(hop), S = hop / nl;
        const size_t lds = (((size_t)nl * (S | 1) + 3) & ~(size_t)3) * sizeof(float) + (size_t)nl * (sizeof(State) + sizeof(double));
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        if (lds > 64 * 1024) {
            for (const void* k : {reinterpret_cast<const void*>(k_bins<false>), reinterpret_cast<const void*>(k_bins<true>)}) {
                hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (e != hipSuccess) return e;
            }
        }
        const dim3 grid(bins_max, B * ch);
        if (bins_max > 1) {
            hipLaunchKernelGGL(k_bins<false>, grid, dim3(kWave), lds, stream, P.p, P.row_stride, P.plane_stride, ch, L, lengths, hop, nl,
                               S, bins_max, f, states, sums);
        }
        hipLaunchKernelGGL(k_carry, dim3((B * ch + kWave - 1) / kWave), dim3(kWave), 0, stream, B * ch, ch, L, lengths, hop, bins_max,
                           f, states);
        hipLaunchKernelGGL(k_bins<true>, grid, dim3(kWave), lds, stream, P.p, P.row_stride, P.plane_stride, ch, L, lengths, hop, nl, S,
                           bins_max, f, states, sums);
    }
    hipLaunchKernelGGL(k_gate, dim3(B), dim3(kGateThreads), 0, stream, sums, ch, L, lengths, hop, bins_max > 0 ? bins_max : 1, weights,
                       out, out_pitch, blocks, nb_max);
    return hipGetLastError();
}

hipError_t lass_launch_loudness(const PlaneRows& P, const int* lengths, int hop, const LoudnessFilter& f, const float* weights, double* out,
                                double* blocks, int nb_max, double* scratch, hipStream_t stream) {
    return launch_meter(P, lengths, hop, f, weights, out, 3, blocks, nb_max, scratch, stream);
}

hipError_t lass_launch_loudness_stats(const PlaneRows& P, const int* lengths, int hop, const LoudnessFilter& f, const float* weights,
                                      double* out, double* blocks, int nb_max, double* short_term, int ns_max, double* scratch,
                                      hipStream_t stream) {
    hipError_t e = launch_meter(P, lengths, hop, f, weights, out, 10, blocks, nb_max, scratch, stream);
    if (e != hipSuccess) return e;
    const int bins_max = P.L / hop;
    const double* sums = scratch + (size_t)4 * P.B * P.ch * bins_max;
    hipLaunchKernelGGL(k_range, dim3(P.B), dim3(kGateThreads), 0, stream, sums, P.ch, P.L, lengths, hop, bins_max > 0 ? bins_max : 1,
                       weights, out, scratch + (size_t)5 * P.B * P.ch * bins_max, short_term, ns_max);
    return hipGetLastError();
}

hipError_t lass_launch_loudness_gain(const double* loudness, const float* peak, int B, double target, float ceiling, float* gain,
                                     int* limited, hipStream_t stream) {
    if (B <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gain, dim3((B + 63) / 64), dim3(64), 0, stream, loudness, peak, B, target, ceiling, gain, limited);
    return hipGetLastError();
}
