// polyphase.h - the polyphase FIR of resample.hip and export.hip (y[n] = sum_m x[m] * h[n*down - m*up + half], zeros outside the
// row), shared by inclusion so that every kernel built on it computes an output with the same instructions in the same order:
// decode (mono and planar) and export agree bit for bit because they ARE one tap chain.  Include inside an anonymous namespace,
// after kernels.h.  DESIGN.md section 12 has the filter and the indexing.
//
// One workgroup makes `tile` consecutive outputs of one row.  With t = n*down + half, output n reads the inputs m0 - j (m0 = t / up,
// j = 0 ... J-1, J = ceil(n_taps / up)) against the taps h[p + j*up] of its phase p = t % up, so the workgroup keeps in LDS
//   tab[p][j] = h[p + j*up] (0 past the filter's end), row pitch J | 1: the lanes of a wave sit on different phases, and an odd
//               pitch spreads their rows over the banks; with up == 1 there is one row, which every lane reads at the same j (a
//               broadcast);
//   span[s]   = input (first input of the tile's reach) + s, zero outside the row.
// Every output is one f32 fmaf chain over j = 0 ... J-1 in that order, whatever the batch, the row stride or the tile it falls in.
// The kernels differ only in how an input is loaded (fir_fill's callable) and where an output goes.
#pragma once

constexpr int kThreads = 256;
constexpr int kTileMax = 2048;          // outputs per workgroup (fewer when the kernel's LDS need would not fit)
constexpr int kLdsFloats = 160 * 256;   // 160 KiB per CU

struct FirTile {
    float* tab;     // [up][Jp]
    float* span;    // [(up - 1 + (tile - 1) * down) / up + J]
    long long n0;   // first output of the tile
    long long mlo;  // the input span[0] holds
    unsigned r0;    // phase of the first output
    int nout, S;    // outputs made, inputs reached
    int J, Jp, up, down;
};

// The tile of workgroup blockIdx.x of a row of L_out outputs.
__device__ __forceinline__ FirTile fir_tile(float* lds, int up, int down, int n_taps, int J, int tile, int L_out) {
    FirTile T;
    T.J = J;
    T.Jp = J | 1;
    T.up = up;
    T.down = down;
    T.tab = lds;
    T.span = lds + (size_t)up * T.Jp;
    // 64-bit: n*down and m*up pass 2^31 on long rows (44.1 <-> 16 kHz: after 304 s)
    T.n0 = (long long)blockIdx.x * tile;
    const long long t0 = T.n0 * down + (n_taps - 1) / 2;
    const long long q0 = t0 / up;
    T.r0 = (unsigned)(t0 - q0 * up);
    T.nout = (int)(L_out - T.n0 < tile ? L_out - T.n0 : tile);
    T.S = (int)((T.r0 + (unsigned)(T.nout - 1) * (unsigned)down) / (unsigned)up) + J;
    T.mlo = q0 - (J - 1);
    return T;
}

// The same for a tile that does not start at blockIdx.x * tile: the `count` outputs from output `first` >= 0 on (a tile with a
// halo, export.hip's true-peak sink).  A sibling and not a generalisation, so that fir_tile's callers compile to what they did.
__device__ __forceinline__ FirTile fir_tile_at(float* lds, int up, int down, int n_taps, int J, long long first, int count) {
    FirTile T;
    T.J = J;
    T.Jp = J | 1;
    T.up = up;
    T.down = down;
    T.tab = lds;
    T.span = lds + (size_t)up * T.Jp;
    T.n0 = first;
    const long long t0 = first * down + (n_taps - 1) / 2;
    const long long q0 = t0 / up;
    T.r0 = (unsigned)(t0 - q0 * up);
    T.nout = count;
    T.S = (int)((T.r0 + (unsigned)(count - 1) * (unsigned)down) / (unsigned)up) + J;
    T.mlo = q0 - (J - 1);
    return T;
}

// tab <- taps.  The caller's first span fill may follow at once; one __syncthreads() after it covers both.
__device__ __forceinline__ void fir_table(const FirTile& T, const float* __restrict__ taps, int n_taps) {
    // only the last tap of a phase can lie past the filter's end
    for (int p = threadIdx.x; p < T.up; p += kThreads) T.tab[p * T.Jp + T.J - 1] = 0.f;
    __syncthreads();
    for (int k = threadIdx.x; k < n_taps; k += kThreads) T.tab[(k % T.up) * T.Jp + k / T.up] = taps[k];
}

// span <- load(m) for the inputs m of the tile's reach that lie in [0, len), zero elsewhere
template <class Load>
__device__ __forceinline__ void fir_fill(const FirTile& T, int len, Load load) {
    for (int s = threadIdx.x; s < T.S; s += kThreads) {
        const long long m = T.mlo + s;
        T.span[s] = (m >= 0 && m < len) ? load(m) : 0.f;
    }
}

// output i of the tile
__device__ __forceinline__ float fir_output(const FirTile& T, int i) {
    const unsigned t = T.r0 + (unsigned)i * (unsigned)T.down;
    const unsigned q = t / (unsigned)T.up;
    const float* g = T.tab + (t - q * (unsigned)T.up) * T.Jp;
    const float* x = T.span + q + (T.J - 1);
    float acc = 0.f;
    for (int j = 0; j < T.J; ++j) acc = fmaf(x[-j], g[j], acc);
    return acc;
}

struct FirPlan {
    int J, tile;
    size_t lds;     // bytes
    unsigned nblk;  // tiles per row
};

// The launch plan of `kernel` for rows of n_out outputs: the largest tile whose LDS need, floats_of(tile) floats (the table, the
// span and whatever else the kernel keeps per tile), fits 160 KiB; one output always fits under the caps.  hipErrorInvalidValue
// for what the caps or the grid cannot hold.
template <class FloatsOf>
hipError_t fir_plan(const void* kernel, int up, int down, int n_taps, int n_out, FloatsOf floats_of, FirPlan* P) {
    if (up > LASS_RESAMPLE_MAX_RATIO || down > LASS_RESAMPLE_MAX_RATIO || n_taps > LASS_RESAMPLE_MAX_TAPS ||
        lass_resample_table_floats(up, n_taps) > LASS_RESAMPLE_MAX_TABLE)
        return hipErrorInvalidValue;
    P->J = (n_taps + up - 1) / up;
    P->tile = kTileMax;
    while (P->tile > 1 && floats_of(P->tile) > (size_t)kLdsFloats) P->tile /= 2;
    P->lds = floats_of(P->tile) * sizeof(float);
    if (P->lds > (size_t)kLdsFloats * sizeof(float)) return hipErrorInvalidValue;
    if (P->lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFloats * (int)sizeof(float));
        if (e != hipSuccess) return e;
    }
    const long long nblk = ((long long)n_out + P->tile - 1) / P->tile;
    if (nblk > 0x7fffffffLL) return hipErrorInvalidValue;
    P->nblk = (unsigned)nblk;
    return hipSuccess;
}
