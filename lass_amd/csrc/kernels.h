// kernels.h - internal launch interfaces between the C-ABI layer (api.hip) and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "audio_args.h"  // the operand structs of the audio file launchers and lass_resample_table_floats (host only, HIP-free)
#include "conv_route.h"  // ConvKind, the shape rules of the f32 conv families and the route of a block, LASS_NFFT & co (host only, HIP-free)

// ---- conv.hip -----------------------------------------------------------------------------------------------------
struct ConvArgs {
    // phase A: K = Cin x TAPS
    const float* in = nullptr;  // (B, Cin, H, W); batch stride in_bs, channel stride H*W
    long in_bs = 0;
    int Cin = 0;
    const float* w = nullptr;  // Wt[Cin][TAPS][Nw]
    int Nw = 0;                // row pitch of the weight matrix (total output channels it holds)
    const float* pro_scale = nullptr;  // [Cin]
    const float* pro_shift = nullptr;  // [B][pro_shift_bs], column = channel
    int pro_shift_bs = 0;
    // phase B: 1x1 shortcut over the raw block input
    const float* in2 = nullptr;
    long in2_bs = 0;
    int Cin2 = 0;
    const float* w2 = nullptr;    // [Cin2][Nw]
    const float* bias = nullptr;  // [Nw]
    const float* res = nullptr;   // (B, N, H, W) residual
    long res_bs = 0;
    const float* epi_scale = nullptr;  // [N]
    const float* epi_shift = nullptr;  // [B][epi_shift_bs]
    int epi_shift_bs = 0;
    float* out = nullptr;
    long out_bs = 0;
    int B = 0, H = 0, W = 0;
    int N = 0;  // output channels computed by this launch (GEMM rows)
    int up_h = 1;  // TCONV: vertical stride (1 or 2); horizontal stride is always 2
    const float* w_wino = nullptr;   // Winograd-domain weights U[16][Cin][Nw] (wino.hip)
    const float* w2_wino = nullptr;  // Winograd-domain shortcut weights [4][Cin2][Nw]
    const float* w_wino4 = nullptr;    // Winograd F(4x4,3x3)-domain weights: LDS images of wino4.hip (36 * Cin * Nw floats)
    const void* w_bf16 = nullptr;    // bf16 weights [Cin/16][tap][2][Nw][8] (conv_bf16.hip)
    const void* w2_bf16 = nullptr;   // bf16 shortcut weights [Cin2/16][1][2][Nw][8]
    const void* w_bf16_lo = nullptr;   // split mode: bf16(w - float(bf16(w))), same layouts; non-null selects the 3-MFMA kernels
    const void* w2_bf16_lo = nullptr;
    // bf16 modes: the block's intermediate (conv1 -> conv2) in the blocked bf16 layout [B][C/8][H][W][8], hi (+ lo) planes
    void* out_bf16 = nullptr;
    void* out_bf16_lo = nullptr;
    const void* in_bf16 = nullptr;
    const void* in_bf16_lo = nullptr;
    // bf16 mode, decoder inputs: the concat (transposed-conv output | encoder skip) is kept as TWO blocked bf16 copies
    // instead of f32 - `raw` for the 1x1 shortcut and `act` = leaky(v*act_scale[c] + act_shift[b][c]) (the consumer's
    // BN+FiLM prologue) for conv1.  Producers write octets [out_oct0, out_oct0 + N/8) of out_noct octets per clip.
    void* out_bf16_act = nullptr;
    const float* act_scale = nullptr;   // indexed by this launch's output channel
    const float* act_shift = nullptr;   // [B][act_shift_bs]
    int act_shift_bs = 0;
    int out_oct0 = 0;
    int out_noct = 0;                   // 0: N / 8
    const void* in2_bf16 = nullptr;     // phase B (1x1 shortcut) input as the blocked bf16 raw copy
    // bf16 mode, encoder chain: the fused avg-pool output as two blocked bf16 copies (raw + activated with the NEXT block's
    // conv1 prologue) instead of f32; replaces pool_out when set
    void* pool_bf16 = nullptr;
    void* pool_bf16_act = nullptr;
    int pool_oct0 = 0;                      // the launch writes octets [pool_oct0, pool_oct0 + N/8) of pool_noct per clip
    int pool_noct = 0;                      // (0: N / 8) - a channel slice of a wider pooled tensor (multi-STFT branches)
    const float* pool_act_scale = nullptr;  // indexed by this launch's output channel
    const float* pool_act_shift = nullptr;  // [B][act_shift_bs]
    const float* pre_w = nullptr;  // pre_conv (1x1, 1 -> 32) weight / bias for the *_PRE kinds
    const float* pre_b = nullptr;
    // fused output head (decoder_block6.conv2 only, N == 32, W == mask_nbins - 1: 512 or 1024 bins, the kernels read W): after_conv (1x1, 32 -> 3, + bias) and the complex
    // ratio mask (resunet.py:570-574,436-519) in the epilogue; the block's own output is then not written at all
    const float* mask_w = nullptr;    // after_conv.weight [3][32]
    const float* mask_b = nullptr;    // after_conv.bias [3]
    const float* mask_mag = nullptr;  // (B, mask_T, 513) mixture magnitude / cos / sin
    const float* mask_cos = nullptr;
    const float* mask_sin = nullptr;
    float* mask_re = nullptr;         // (B, mask_T, 513) separated spectrum
    float* mask_im = nullptr;
    int mask_T = 0;                   // frames (rows y >= mask_T are the T padding: dropped)
    int mask_nbins = LASS_NBINS;      // bins per spectrum row = W + 1 (513; 1025 at n_fft 2048: ResUNet30 at 32 kHz, the multi-STFT model)
    float* pool_out = nullptr;  // fused avg-pool of the output: (B, N, H/pool_h, W/2), batch stride pool_bs
    long pool_bs = 0;            // elements between clips of pool_out; 0 = dense (N * H/pool_h * W/2).  A launch that
                                 // produces a channel slice of a wider pooled tensor passes the wide tensor's stride.
    int pool_h = 2;              // vertical pool factor (1 or 2); horizontal is 2
    // XCD-aware block order (conv.hip, wino.hip, wino4.hip, conv_bf16.hip): launched as a 1-D grid of gx * gy * B workgroups;
    // set by the launcher
    int gx = 0, gy = 0;        // spatial tiles per clip, cout blocks
    int xcd_map = 0;           // 1 (when gx * B is a multiple of 8): the gy cout blocks of one (tile, clip) run on ONE XCD (they
                               // re-read the same input tile), and every XCD walks one contiguous range of tiles
                               // (block_coords, wino_common.h)
};

// Split-K on the 32 x 16 blocks of wino4.hip (conv_route.h: lass_wino4_narrow): the input-channel loop is dealt to n workgroups per
// (block, cout group, clip); each stores its partial of the conv sum, [n][B][N][H][W] dense in part, and a combine launch sums them in split order and applies the epilogue.
// (Not part of ConvArgs: the kernels that take only ConvArgs keep their argument block, and with it their compiled code.)
struct Wino4Split {
    int n = 1;
    float* part = nullptr;
};

// The transformed input image of a layer, formed once by a prep launch instead of by every cout group's workgroups:
// v[clip][block][chunk = cin / 8][36][256] f32, lass_wino4_vpre_floats() of them; null = the kernels transform their own input.
// (Beside ConvArgs for the same reason as Wino4Split.)
struct Wino4VPre {
    float* v = nullptr;
};

// The folded head's shortcut logits, formed where their inputs are produced (conv_route.h: head_sc_fold): Wsc' cat = Wsc'_skip x1 +
// (Wsc'_up o Wt) act(x11), as two sets of planes [B][3][H][W] f32 at decoder_block6's resolution.  encoder_block1.conv2 writes
// `skip` from its epilogue registers, the transposed conv's two cout blocks write `up` (12 more columns), the head adds (skip + up) to its conv
// sum.  (Beside ConvArgs for the same reason as Wino4Split.)
struct HeadScPlanes {
    float* skip = nullptr;
    float* up = nullptr;
    const float* w = nullptr;  // the producer's composed weights (head_fold.h): Wsc'_skip [3][32], or Wt' [Cin][64]; the head reads none
};

// The shape half of the predicates below (conv_route.h) reads a launch as its ConvShape; they add that the pointers are there.
inline ConvShape lass_conv_shape(const ConvArgs& p) {
    ConvShape s;
    s.Cin = p.Cin; s.N = p.N; s.Nw = p.Nw; s.H = p.H; s.W = p.W;
    s.Cin2 = p.Cin2; s.pool = p.pool_out != nullptr; s.pool_h = p.pool_h; s.head = p.mask_re != nullptr;
    return s;
}

hipError_t lass_launch_conv(ConvKind kind, const ConvArgs& p, hipStream_t stream);
// TCONV_ACT (2 x 2, f32 output, two cout blocks) with 12 more columns in the same launch: hs.w = Wt' [Cin][64], whose 12 live
// columns (3 logits x 4 sub-pixels) go to hs.up as three planes at the up-sampled resolution
bool lass_tconv_logits_supported(const ConvArgs& p, const HeadScPlanes& hs);
hipError_t lass_launch_tconv_logits(const ConvArgs& p, const HeadScPlanes& hs, hipStream_t stream);

// ---- wino.hip (Winograd F(2x2,3x3) variant of the 3x3 kinds; W must be a multiple of 32, H even) -------------------
bool lass_wino_supported(const ConvArgs& p);
hipError_t lass_launch_wino(ConvKind kind, const ConvArgs& p, hipStream_t stream);
hipError_t lass_launch_wino_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream);
hipError_t lass_launch_wino_shortcut_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream);

// ---- wino4.hip (Winograd F(4x4,3x3): 36 instead of 64 MFMA multiplies per 16 outputs; W % 32 == 0) ---------------------------
// CONV2_IDENT: conv2 + a residual read from res (which may be `out` itself: every element is read and written by one lane)
bool lass_wino4_supported(ConvKind kind, const ConvArgs& p, const Wino4Split& sk = Wino4Split());
hipError_t lass_launch_wino4(ConvKind kind, const ConvArgs& p, hipStream_t stream, const Wino4Split& sk = Wino4Split(),
                             const Wino4VPre& vp = Wino4VPre());
// V from memory (vp.v set): CONV1_ACT and CONV2_IDENT only, a prep launch in front of the conv launch
bool lass_wino4_vpre_supported(ConvKind kind, const ConvArgs& p, const Wino4Split& sk = Wino4Split());
hipError_t lass_launch_wino4_weights(const float* w, int Cout, int Cin, float* U, hipStream_t stream);  // w (Cout, Cin, 3, 3)
// decoder_block6.conv2 + shortcut + output head on weights composed with after_conv (head_fold.h): w_wino4 / w2 / bias hold the
// composed images (U per 8-channel chunk, Wsc' [Cin2][16], b' [16]); N = Nw = 32 still name the conv that was folded
bool lass_wino4_headfold_supported(const ConvArgs& p);
hipError_t lass_launch_wino4_headfold(const ConvArgs& p, hipStream_t stream);
// ... with the shortcut's logits read from hs.skip / hs.up instead of formed from in2 (which is not read; Cin2 still names it)
bool lass_wino4_headfold_planes_supported(const ConvArgs& p, const HeadScPlanes& hs);
hipError_t lass_launch_wino4_headfold_planes(const ConvArgs& p, const HeadScPlanes& hs, hipStream_t stream);
// CONV2_IDENT_PRE on the 8 x 64 blocks (encoder_block1.conv2) that also writes hs.skip = hs.w x1 from its epilogue
bool lass_wino4_sclogit_supported(const ConvArgs& p, const HeadScPlanes& hs);
hipError_t lass_launch_wino4_sclogit(const ConvArgs& p, const HeadScPlanes& hs, hipStream_t stream);

// ---- wino4_gemm.hip (F(4x4,3x3) as scatter - 36 batched split-bf16 GEMMs - gather: the V-from-memory convs with 128-multiples of
// couts; conv_route.h: ConvRoute::gemm) -------------------------------------------------------------------------------------------
// w3 = the layer's U split into three bf16 pieces, [36][3][Cin / 8][N][8] (lass_launch_wino4_gemm_weights, from the w_wino4 image:
// 216 Cin N bytes); m = the product image M[36][N][tiles of the batch] f32, lass_wino4_gemm_m_floats() of them.  vp.v takes V in GEMM
// layout [36][Cin][tiles]: lass_wino4_vpre_floats() floats, as the prep launch's image.  (Beside ConvArgs for Wino4Split's reason.)
struct Wino4Gemm {
    const void* w3 = nullptr;
    float* m = nullptr;
};
// CONV1_ACT and CONV2_IDENT (res may be `out` itself); three launches: scatter, GEMMs, gather
bool lass_wino4_gemm_supported(ConvKind kind, const ConvArgs& p, const Wino4VPre& vp, const Wino4Gemm& g);
hipError_t lass_launch_wino4_gemm(ConvKind kind, const ConvArgs& p, const Wino4VPre& vp, const Wino4Gemm& g, hipStream_t stream);
hipError_t lass_launch_wino4_gemm_weights(const float* U, int Cout, int Cin, void* dst, hipStream_t stream);

// ---- pw_gemm.hip (f32 pointwise GEMMs with a 128-cout workgroup tile; H*W % 4 == 0, N % 128 == 0, K % 32 == 0) ------------
// CONV2_SHORTCUT: only the 1x1 shortcut, out = bias + Wsc x (in2, Cin2, w2, bias), for conv2 to read back as its residual;
// TCONV_ACT: the kernel == stride transposed conv behind its BN+FiLM+leaky prologue (f32 output only)
// sw.w set: the split-bf16 kernel (six v_mfma_f32_32x32x16_bf16 products of three exact bf16 pieces per operand, f32 accuracy)
// on weights that lass_launch_pw_split_weights formed from the same [K][Nw] f32 matrix: [3][K / 8][Nw][8] bf16, 6 K Nw bytes.
// (Beside ConvArgs for the same reason as Wino4Split.)
struct PwSplitW {
    const void* w = nullptr;
};
bool lass_pw_gemm_supported(ConvKind kind, const ConvArgs& p);
hipError_t lass_launch_pw_gemm(ConvKind kind, const ConvArgs& p, hipStream_t stream, const PwSplitW& sw = PwSplitW());
hipError_t lass_launch_pw_split_weights(const float* w, int K, int Nw, void* dst, hipStream_t stream);

// ---- conv_bf16.hip (bf16-MFMA variant of the 3x3 kinds; W multiple of 32, Cin multiple of 16) ----------------------
bool lass_bf16_supported(const ConvArgs& p);
hipError_t lass_launch_conv_bf16(ConvKind kind, const ConvArgs& p, hipStream_t stream);
hipError_t lass_launch_weights_bf16(const float* w, int Cout, int Cin, int taps, void* dst, int lo, int transposed,
                                    hipStream_t stream);

// ---- conv_bf16_fused.hip (bf16 mode: encoder_block1's ConvBlockRes as one kernel, intermediate in LDS) -------------------
// p = the block's CONV1_ACT_PRE arguments, q = its CONV2_IDENT_PRE arguments with blocked bf16 outputs
bool lass_enc1_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q);
hipError_t lass_launch_enc1_fused_bf16(const ConvArgs& p, const ConvArgs& q, hipStream_t stream);
// ... and decoder_block6's (conv1 64 -> 32 from the activated cat copy, conv2 + 1x1 shortcut over the raw copy + output head)
bool lass_dec6_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q);
hipError_t lass_launch_dec6_fused_bf16(const ConvArgs& p, const ConvArgs& q, hipStream_t stream);

// ... and the same block with decoder_block6's transposed conv computed inside (the up-sampled half of the concat never goes
// to HBM).  u: in_bf16 = the previous decoder's activated blocked-bf16 output (B, 64/8, H/2, W/2, 8), w_bf16 = the transposed
// conv's bf16 weights, w2_bf16 = the composed shortcut weights (lass_launch_compose_up_shortcut -> lass_launch_weights_bf16),
// H, W = the low resolution, Cin = 64
bool lass_dec6u_fused_bf16_supported(const ConvArgs& p, const ConvArgs& q, const ConvArgs& u);
hipError_t lass_launch_dec6u_fused_bf16(const ConvArgs& p, const ConvArgs& q, const ConvArgs& u, hipStream_t stream);
// out[((a*2+bb) * Nsc + n) * Cin + ci] = sum_co wsc[n][co] * wt[ci][co][a][bb]   (f32; wsc (Nsc, Ccat, 1, 1), wt (Cin, Cup, 2, 2))
hipError_t lass_launch_compose_up_shortcut(const float* wsc, const float* wt, int Cin, int Cup, int Ccat, int Nsc, float* out,
                                           hipStream_t stream);

// ---- stft.hip -----------------------------------------------------------------------------------------------------
// Multi-resolution analysis (scripts/precompute_stfts.py:19-58,573-590): nwin centred STFTs (n_fft = win in {256, 512,
// 1024, 2048}, periodic Hann, reflect pad, common hop) of the same waveforms in one launch, torchlibrosa-magphase
// semantics (clamp on |X| at 1e-10).  Outputs (B, T, n_fft/2+1) each, T = 1 + L/hop.  tw2k: 2048 (cos, sin)(2*pi*k/2048).
hipError_t lass_launch_multi_stft(const float* wav, int B, int L, int hop, int nwin, const int* n_fft,
                                  const float2* tw2k, float* const* mag, float* const* cosv, float* const* sinv,
                                  hipStream_t stream);
// Generic pair-packed transforms (stft.hip): n_fft in {1024, 2048}; each branch is a periodic Hann window of `wlen`
// samples (a divisor of 2048, <= n_fft) zero-padded to n_fft and centred.  Outputs per branch where non-null:
// mag/cos/sin/real/imag (B, T, n_fft/2+1) and x0 (B, Tpad, n_fft/2) = bn0(mag), zero rows T..Tpad-1, Nyquist dropped.
// magphase_sem: 0 = base.py:83-88 (clamp on |X|^2), 1 = torchlibrosa magphase (clamp on |X|).
struct StftBranch {
    int wlen = 0;
    float *mag = nullptr, *cosv = nullptr, *sinv = nullptr, *real = nullptr, *imag = nullptr, *x0 = nullptr;
};
// The clips of one launch of the two kernels below (host side; stft.hip turns it into the kernel's form when it instantiates):
//   dense   (lengths == starts == nullptr): clip b is wav[b * L, (b + 1) * L), T = 1 + L / hop frames.
//   ragged  (lengths: device int32 (B), clamped into the 32-frame bucket of L by the kernels): the same rows, Tpad = 32 *
//           ceil(T / 32).  Beyond a clip's own frames x0 and the spectra are 0; beyond its own samples the waveform is 0.
//   windows (starts: device int64 (B); lass_separate_windows): window b is wav[starts[b], starts[b] + L) of ONE row of `total`
//           samples, and of its L output samples only keep[2b] <= n < keep[2b+1] (device int32 (2B), needed by the iSTFT alone)
//           are stored, at out[starts[b] + n].  The kernels clamp starts into [0, total - L], lo into [0, L], hi into [lo, L].
//   faded windows (windows with fade: device int32 (2B) flag pairs, ramp: device f32 (F), 1 <= F <= L;
//           lass_separate_windows_faded): the first min(F, hi - lo) kept samples of a window whose fade[2b] is set, and the last
//           F (cut where they would reach into the former) of one whose fade[2b+1] is set, are multiplied by ramp[n - lo] /
//           ramp[hi - 1 - n] and ADDED to out[starts[b] + n].  Read by the iSTFT alone.
struct ClipForm {
    int B = 0;
    int L = 0;  // samples per row, or per window
    const int* lengths = nullptr;
    const int64_t* starts = nullptr;
    const int* keep = nullptr;
    int64_t total = 0;
    const int* fade = nullptr;
    const float* ramp = nullptr;
    int F = 0;
    // Linked channels (lass_separate_ragged_linked / lass_separate_windows_linked; read by api.hip alone, no kernel sees them):
    // the rows above are the GUIDE's, and `channels` planes laid out as the guide, plane c `c * plane_stride` floats after
    // `planes`, are masked with the guide's mask and written `c * out_plane_stride` floats after the call's output.
    const float* planes = nullptr;
    int64_t plane_stride = 0, out_plane_stride = 0;
    int channels = 0;
};
hipError_t lass_launch_stft2(const float* wav, const ClipForm& cf, int n_fft, int hop, int T, int Tpad, int nbr,
                             const StftBranch* br, int magphase_sem, const float* s0, const float* h0,
                             const float2* tw2k, hipStream_t stream);
// The transform of lass_launch_stft2 (one branch, window `wlen`, the same kernel body: the same bits as its real / imag) with a
// masked epilogue: y = X * (m_re + i m_im), all (B, T, n_fft/2+1), as four products and two sums, each rounded once, no fma:
// y_re = fl(fl(X_re m_re) - fl(X_im m_im)), y_im = fl(fl(X_re m_im) + fl(X_im m_re)).  Rows beyond a ragged clip's frames: 0.
hipError_t lass_launch_masked_stft(const float* wav, const ClipForm& cf, int n_fft, int hop, int T, int wlen, const float* m_re,
                                   const float* m_im, float* y_re, float* y_im, const float2* tw2k, hipStream_t stream);
// mag = cos = 1, sin = 0 over n floats each: with it the output head leaves the complex mask itself in its outputs
hipError_t lass_launch_unit_spectrum(float* mag, float* cosv, float* sinv, size_t n, hipStream_t stream);
// Fused inverse STFT (inverse transforms + overlap-add + envelope + trim in one kernel, no frame scratch).
hipError_t lass_launch_istft2(const float* real, const float* imag, const ClipForm& cf, int T, int n_fft, int wlen, int hop,
                              const float2* tw2k, float* wav, hipStream_t stream);

// ---- misc.hip -----------------------------------------------------------------------------------------------------
// film[b][j] = dot(cond[b], Wf[j]) + bf[j] (+ base[j] if base)   for j < n
hipError_t lass_launch_film(const float* cond, int B, const float* Wf, const float* bf, const float* base, int n,
                            float* out, hipStream_t stream);
// average pool (ph x pw) of (B,C,H,W) with batch stride in_bs -> (B,C,H/ph,W/pw) dense
hipError_t lass_launch_pool(const float* in, long in_bs, int B, int C, int H, int W, int ph, int pw, float* out,
                            hipStream_t stream);
hipError_t lass_launch_mask(const float* x12, const float* wa, const float* ba, const float* mag, const float* cosv,
                            const float* sinv, int B, int T, int Tpad, int fcrop, float* out_real, float* out_imag,
                            hipStream_t stream);
// x0 (B,Tpad,fcrop) = bn0 affine of a precomputed magnitude (B,T,fcrop+1), zero rows T..Tpad-1
hipError_t lass_launch_x0_from_mag(const float* mag, int B, int T, int Tpad, int fcrop, const float* s0,
                                   const float* h0, float* x0, hipStream_t stream);
hipError_t lass_launch_sdr(const float* ref, const float* est, int B, int L, double* stats, hipStream_t stream);
// mixture = source + noise * sqrt(P_source / 10^(snr/10) / P_noise); if max|mixture| > 1 both source and mixture are
// scaled by 0.9/max (dcase_evaluator.py:77-89).  source is updated in place; ws: 4*B doubles of scratch.
hipError_t lass_launch_mix_at_snr(float* source, const float* noise, const float* snr_db, float* mixture, int B, int L,
                                  double* ws, hipStream_t stream);
// SegmentMixer.__call__ (data/waveform_mixers.py:19-62) with the random draws passed in: clip n + its mix_num[n] - 1 successors
// (energy-matched, comp_db[n][i] dB each), the noise sum energy-matched again (+ noise_db[n] dB), declipped to a 0.9 peak.
// ws: 4*B doubles of scratch; max_comp = columns of comp_db (1 ... 7).
hipError_t lass_launch_segment_mix(const float* waveforms, int B, int L, const int* mix_num, const float* comp_db, int max_comp,
                                   const float* noise_db, float* mixture, float* segment, double* ws, hipStream_t stream);
// dst[ci][tap][co] = src[co][ci][tap]
hipError_t lass_launch_relayout_conv(const float* src, int Cout, int Cin, int taps, float* dst, hipStream_t stream);
// scale[c] = g/sqrt(var+eps); base[c] = beta - mean*scale
hipError_t lass_launch_bnfold(const float* g, const float* beta, const float* mean, const float* var, int C, float eps,
                              float* scale, float* base, hipStream_t stream);

// ---- resample.hip, export.hip, limiter.hip, loudness.hip: the audio file kernels ------------------------------------------------
// The operands are audio_args.h's structs.  P: B recordings x ch planes of L floats (PlaneRows; strides in floats).  F: the
// rational filter, out[n] = sum_m x[m] * taps[n*down - m*up + (n_taps-1)/2], up == down == 1: none, taps unused (RationalFilter).
// raw / out / dry: B rows of interleaved frames, enc = LASS_WAV_*, row_stride_bytes apart (PayloadRows); with a dry source the value
// that goes on is v = fl(x + fl(amount[b] * y)), x sample n*ch + c of the dry row (DrySource; NULL: v = y).  O: the (os, 1)
// interpolator of polyphase.h's chain, 20*os + 1 device floats (Oversampler).  The entry points of api.hip have checked the
// arguments (audio_args.h); each launcher keeps a cheap hipErrorInvalidValue guard, and returns it for what its LDS plan cannot hold.
size_t lass_resample_span_floats(int up, int down, int n_taps, int tile);  // the input frames `tile` outputs reach, in LDS
// raw -> out (B, L_out) mono f32: decode, down-mix, F.  planar: out (B, ch, L_out), each plane bit-identical to the mono call on it
hipError_t lass_launch_decode_resample(const PayloadRows& raw, int B, const RationalFilter& F, bool planar, float* out, int L_out,
                                       hipStream_t stream);
// P -> out: F per plane, truncated to out.frames, times gain[b] (B device floats; NULL: none, the same bytes as gain 1), quantised
// as wavio's writers do.  clipped (B counters, may be NULL): += the PCM samples of the row that the clip changed.
hipError_t lass_launch_encode(const PlaneRows& P, const RationalFilter& F, const DrySource* dry, const float* gain, const PayloadRows& out,
                              unsigned* clipped, hipStream_t stream);
// peak[b] = max |v| over the planes of row b and n < frames_out, v what the launcher above quantises without a gain; a NaN is
// skipped.  peak (B floats) is zero-filled here, then raised by integer atomic max on |v|'s bits.
hipError_t lass_launch_sample_peak(const PlaneRows& P, const RationalFilter& F, const DrySource* dry, int frames_out, float* peak,
                                   hipStream_t stream);
// peak[b] = the larger of that and max |z[k]|, k % os != 0, z = y interpolated by O (y = 0 outside its frames_out frames).  os in
// {2, 4}; one launch, the y of a tile and its halo in LDS.  hipErrorInvalidValue where lass_resample_true_peak_fits is false:
bool lass_resample_true_peak_fits(int up, int down, int n_taps, int os);  // a tile of one frame fits the CU's 160 KiB
hipError_t lass_launch_resample_true_peak(const PlaneRows& P, const RationalFilter& F, int frames_out, const Oversampler& O, float* peak,
                                          hipStream_t stream);
// lass_limit's kernel (include/lass_hip.h has the arithmetic): out = fl(fl(g * G) * x) with G the smoothed minimum of the gain that
// holds g x envelope under `ceiling`; one launch, LASS_LIMITER_TILE frames per workgroup.  out: the output planes (written).
// min_gain (1) and frames (0) are filled here, on the stream.
hipError_t lass_launch_limit(const PlaneRows& P, const Oversampler& O, const float* gain, float ceiling, int H, const float* window,
                             const PlaneRows& out, float* curve, float* envelope, long long curve_row_stride, float* min_gain,
                             int* frames, hipStream_t stream);

// K-weighting as the kernels take it: the two biquads (b0 b1 b2 a1 a2 of the shelf, then of the high-pass) and the powers of the
// cascade's 4 x 4 state matrix that carry a state over one lane's samples and over one hop bin, row-major.
struct LoudnessFilter {
    double coef[10];
    double lane_step[16];
    double bin_step[16];
};
int lass_loudness_lanes(int hop);  // lanes of the wave that share a hop bin: the largest divisor of hop up to 64
// f <- coef and the two powers for `hop`; false for a coefficient that is not finite or a pole on or outside the unit circle
bool lass_loudness_filter(const double* coef, int hop, LoudnessFilter* f);
// BS.1770-4 gated loudness of P, lengths[b] <= L samples each (NULL: L; clamped to 0 ... L): out (B,3) = {LUFS or -inf, blocks,
// blocks past both gates}; blocks (B, nb_max), optional: the block powers, 0 past a recording's own count.  scratch: 5 * B * ch *
// (L / hop) doubles.
hipError_t lass_launch_loudness(const PlaneRows& P, const int* lengths, int hop, const LoudnessFilter& f, const float* weights, double* out,
                                double* blocks, int nb_max, double* scratch, hipStream_t stream);
// The same into columns 0 ... 2 of out (B,10) by the same kernels, then one more kernel, one workgroup per recording: columns
// 3 ... 9 = {max momentary LUFS, max short-term LUFS, LRA, ns, short-term blocks past both gates, p10, p95} (EBU Tech 3342 on 3 s
// blocks of 30 bin sums; the two order statistics by an exact radix select).  short_term (B, ns_max), optional: the short-term
// powers, 0 past a recording's own count.  scratch: (5 * ch + 1) * B * (L / hop) doubles.
hipError_t lass_launch_loudness_stats(const PlaneRows& P, const int* lengths, int hop, const LoudnessFilter& f, const float* weights,
                                      double* out, double* blocks, int nb_max, double* short_term, int ns_max, double* scratch,
                                      hipStream_t stream);
// lass_loudness_gain's rule, one thread per row
hipError_t lass_launch_loudness_gain(const double* loudness, const float* peak, int B, double target, float ceiling, float* gain,
                                     int* limited, hipStream_t stream);
