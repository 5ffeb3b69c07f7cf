/*
 * lass_hip.h - C-ABI of liblass_hip.so: the MI355X (gfx950) text-conditioned separation hot path.
 *
 *     mixture (B,L) f32 + condition (B,512) f32  --STFT--> |X|,cos,sin --FiLM ResUNet30--> mask --iSTFT--> (B,L) f32
 *
 * The reference (reedrosenbluth/LASS) is pure Python and has no FFI of its own; this boundary replaces what its
 * evaluator calls two levels down:  `pl_model.ss_model(input_dict)["waveform"]`  (dcase_evaluator.py:99-107), i.e.
 * `ResUNet30.forward` (models/resunet.py:640-653) = `FiLM.forward` (:59-81) + `ResUNet30_Base.forward` (:522-595),
 * plus the numpy metrics `calculate_sdr` / `calculate_sisdr` (utils.py:148-200).  Each entry point below cites the
 * reference code it stands in for.  INTEGRATION.md shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - plain C: pointers + sizes; no torch / C++ types.  All tensor pointers are DEVICE pointers unless said otherwise.
 *   - every function returns 0 on success, <0 on error; `lass_last_error(ctx)` has the message.
 *   - kernels are enqueued on the caller's `stream` (a hipStream_t passed as void*) and never synchronise.
 *   - the caller owns inputs, outputs and the workspace; the context owns re-laid-out weights and constant tables.
 *     `lass_separate` allocates nothing.
 *   - workspaces and scratch buffers need no initialisation, and no result depends on their prior content: every kernel writes
 *     what a later one reads, padding included.  (They may hold anything afterwards.)
 *   - outputs are written in full unless their entry says otherwise.  The entries that say otherwise:
 *       `clipped` of lass_resample_encode / lass_resample_encode_gain: counters the call ADDS to, zero-filled by the caller;
 *       the fade regions of lass_separate_windows_faded / lass_istft_windows_faded: weighted and ADDED to `out`, which holds 0
 *         there before the first window reaches them;
 *       bytes past a row's end in the encoders (lass_resample_encode*, `out_stride` beyond the row's bytes): left alone;
 *       samples outside `keep` in lass_separate_windows / lass_istft_windows and their faded forms: left alone.
 *     tests/test_gpu_poison.py holds both rules, on buffers filled with 0x00, 0xFF (a NaN as f32 and as bf16) and 0x7F (3.39e38).
 *   - one context per (process, device); not re-entrant per context.  Every entry point makes the context's device
 *     current (hipSetDevice) before it launches or allocates, so the caller's current device does not matter.
 *   - there is NO CPU fallback: without a gfx950 device `lass_create` fails.
 */
#ifndef LASS_HIP_H
#define LASS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lass_ctx lass_ctx;

/* error codes */
#define LASS_OK 0
#define LASS_ERR_ARG (-1)      /* bad argument / shape */
#define LASS_ERR_HIP (-2)      /* a HIP runtime call failed */
#define LASS_ERR_STATE (-3)    /* call order (e.g. separate before finalize, missing parameter) */
#define LASS_ERR_WORKSPACE (-4)/* workspace too small */

/* dtypes for lass_set_param */
#define LASS_F32 0
#define LASS_I64 1

/* compute modes for lass_finalize */
#define LASS_COMPUTE_F32 0     /* f32 storage, f32 MFMA contractions (plain f32 FMAs): Winograd F(4x4,3x3) for the 3x3 convs with
                                  >= 64 input channels at >= 32-bin resolutions (LASS_WINO4=0: none), F(2x2,3x3) for the rest */
#define LASS_COMPUTE_BF16 1    /* convolutions contracted on the bf16 MFMA (operands rounded to bf16, f32 accumulate):
                                  BASELINE configs[2].  Inside the workspace the tensors handed from one conv launch to
                                  the next (block intermediates, decoder concats, pooled encoder outputs, transposed-conv
                                  inputs) are stored as blocked bf16 [C/8][H][W][8]; spectra, masks and waveforms stay
                                  f32.  Reduced precision, looser parity. */
#define LASS_COMPUTE_BF16X3 2  /* as BF16 but every operand is split hi+lo (two bf16) and each product formed as
                                  hi*hi + hi*lo + lo*hi on the bf16 MFMA: ~16 mantissa bits per operand.  Block
                                  intermediates are two blocked bf16 planes (hi, lo); everything else stays f32. */

/* Library / ABI version (major*10000 + minor*100 + patch). */
int lass_version(void);

/* Create a context on HIP device `device_id`.  Builds the FFT twiddle / Hann tables.
 * Replaces: ResUNet30.__init__ (resunet.py:621-637) + torchlibrosa STFT/ISTFT construction (:284-302).
 * LIMIT: the context implements ResUNet30(input_channels=1, output_channels=1, condition_size=512) with
 * target_sources_num = 1 - the only configuration the reference ships (config/audiosep_base.yaml:23-30); resunet.py:425-470,
 * 621-637 is written for target_sources_num x output_channels x 3 mask channels, and the Python mirror raises
 * NotImplementedError for anything else (lass_amd/resunet.py). */
int lass_create(lass_ctx** out, int device_id);
/* lass_create at a given STFT geometry (n_fft = window length, hop).  Two pairs are accepted:
 *   (1024, 160): exactly lass_create - the reference's 16 kHz layout (resunet.py:271-276), 513-bin bn0, 512-bin images.
 *   (2048, 320): the same network at 32 kHz - 64 ms windows every 10 ms as before, `base.bn0.*` with 1025 entries, images of
 *                1024 bins, the same K = 3 mask head.  These two numbers are those of upstream AudioSep's released 32 kHz
 *                ResUNet30, from which the reference was trimmed; nothing in the reference states them (it keeps only that
 *                model's RATE = 32000 in chunk_inference, resunet.py:657), so they are the specification here.
 * Any other pair: LASS_ERR_ARG, the message names the two.  Everything below works on such a context with hop and n_fft
 * read as the context's: a clip of L samples has 1 + L/hop frames, a ragged bucket is 32*hop samples wide (10 240 at hop 320),
 * L and window lengths must exceed n_fft/2, all three compute modes.  The weight-free stage calls lass_stft_magphase and
 * lass_istft transform at the context's geometry too.  Per-clip limit at (2048, 320): 64 ch x padded frames x 1024 bins x 4 B
 * below 4 GiB = fewer than 16 384 padded frames, 163 s at 32 kHz (LASS_ERR_ARG beyond, as at the default geometry). */
int lass_create_stft(lass_ctx** out, int device_id, int n_fft, int hop);
/* The STFT geometry of a context (either pointer may be NULL): (1024, 160) or (2048, 320) for ResUNet30, (n_fft, 160) for the
 * multi-STFT model. */
int lass_stft_geometry(const lass_ctx* ctx, int* n_fft, int* hop);
/* Context for the multi-resolution-STFT separator (BASELINE configs[4]; reference intent:
 * models/resunet_with_multistft.py:40-118,137-216 - not runnable as shipped, see DESIGN.md section 9 for the authored
 * spec): `n_windows` periodic-Hann analysis windows (`win_lengths`, e.g. {256, 512, 2048}) at a common n_fft (2048),
 * hop 160; one pre_conv + encoder_block1 per window, pools and skips concatenated on channels, shared trunk; the mask is
 * applied to the `mask_window` branch and the waveform comes from an iSTFT with that window.  Parameter names are the
 * reference module tree's (`base.pre_convs.<w>.*`, `base.encoder_block1s.<w>.conv_block1.*`,
 * `film.encoder_block1s-><w>->conv_block1->beta1.*`, ...).  f32 compute only.  All entry points below work on either
 * kind of context. */
int lass_create_multistft(lass_ctx** out, int device_id, int n_fft, int n_windows, const int* win_lengths,
                          int mask_window);
int lass_destroy(lass_ctx* ctx);

/* Last error message of this context (or of the failed lass_create when ctx == NULL). Never NULL. */
const char* lass_last_error(const lass_ctx* ctx);

/* Upload one tensor of the reference's state_dict (key relative to ss_model, e.g.
 * "base.encoder_block1.conv_block1.conv1.weight", "film.decoder_block3->conv_block2->beta1.bias").
 * `data` may be a host or a device pointer (copied with hipMemcpyDefault); shape/dtype are checked against the
 * architecture.  Unknown keys that a reference checkpoint legitimately carries (base.stft.*, base.istft.*,
 * *.num_batches_tracked, decoder_block*.bn2.*, film.decoder_block*->beta2.*) are accepted and ignored (returns 1).
 * Replaces: nn.Module.load_state_dict as used by utils.load_ss_model (utils.py:356-400). */
int lass_set_param(lass_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim, int dtype);

/* Fold BatchNorm (eval mode, eps 1e-5) into per-channel scale/shift tables, concatenate the 32 live FiLM linears into
 * one matrix, re-lay-out conv weights to [cin][tap][cout].  Fails if a required parameter is missing.
 * Must be called again after any lass_set_param. */
int lass_finalize(lass_ctx* ctx, int compute_mode);

/* Bytes of workspace `lass_separate` needs for B clips of L samples.
 * Limits: B >= 1, L > n_fft/2, and the largest per-clip tensor - decoder_block6's concat, (32 + 32*n_windows) channels x
 * padded frames x n_fft/2 bins, f32 - below 4 GiB: the kernels address one clip's tensors with unsigned 32-bit byte offsets.  ResUNet30: 327 s at 16 kHz, 163 s at 32 kHz with the (2048, 320) geometry (lass_create_stft); multi-STFT model: 40.9 s at 32 kHz.  Longer clips are an LASS_ERR_ARG here and in lass_separate; the reference's own long-form route,
 * chunk_inference (resunet.py:655-714), stays available. */
int lass_workspace_bytes(const lass_ctx* ctx, int B, int L, size_t* bytes);

/* The hot path.  mixture (B,L) f32, condition (B,512) f32 -> out (B,L) f32.
 * Replaces: ResUNet30.forward(input_dict)["waveform"] (resunet.py:640-653) with mixture/out squeezed of their
 * singleton channel axis.
 * Scheduling: the hipGraph that replays a recurring call runs an even batch of >= 8 clips as two independent
 * half-batches on two branches, so that one half's small launches and launch tails overlap the other half's
 * full-size ones (LASS_SPLIT=0: never; =2: eager launches too, the second half on an internal stream forked from /
 * joined to `stream` by events).  Clips are independent: the results are bit-identical to the unsplit run, and `stream`
 * still orders the whole call.  lass_workspace_bytes already accounts for it; lass_workspace_tensor reports
 * LASS_ERR_STATE while the last call of that shape ran split (its workspace holds the half-batch layouts).
 * CAUTION for callers with kernels of their own (gfx950, measured: DESIGN.md section 5b).  While a bf16-mode lass_separate
 * (LASS_COMPUTE_BF16 / _BF16X3: workgroups feeding v_mfma_f32_32x32x16_bf16 from LDS) runs on one stream, a kernel on ANOTHER
 * stream that executes packed-f32 vector instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 - hipcc's SLP vectoriser
 * forms them from float2-shaped code such as complex butterflies) can return wrong values when it shares a compute unit with
 * them: the x half of a packed result in lanes 48-63 came out wrong from right operands, about one launch in two of an FFT
 * kernel, never NaN.  Every kernel of this library is built without packed f32 (-fno-slp-vectorize, audited in the ISA by the
 * test suite).  Kernels the CALLER launches concurrently are the caller's to build the same way (or to keep on the same
 * stream as the bf16 lass_separate); f32-mode contexts are not affected. */
int lass_separate(lass_ctx* ctx, const float* mixture, const float* condition, float* out, int B, int L,
                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- ragged batches: clips of different lengths in one call ------------------------------------------------------ */

/* lass_separate for B clips of different lengths.  mixture and out are (B,L) with rows L samples apart; clip b is
 * mixture[b][0 .. lengths[b]) and the rest of its row is never read.  lengths: DEVICE int32 (B).
 * (160 below is the context's hop: read 320 on a (2048, 320) context of lass_create_stft, whose buckets are 10 240 samples wide.)
 * A clip of Lb samples has 1 + Lb/160 frames, zero-padded after bn0 to a multiple of 32 (resunet.py:543-548): the network sees
 * one (padded frames, n_fft/2) image per clip, and clips whose padded frame counts agree can share every launch.  So every clip
 * must lie in the bucket of L:  max(160*(Tp-32), n_fft/2+1) <= lengths[b] <= L,  Tp = 32*ceil((1 + L/160)/32)  - the interval
 * lass_ragged_bucket returns.  Row b of `out` is then, bit for bit, what lass_separate gives for that clip alone at its own
 * length (f32; in the bf16 modes as close as lass_separate's own batch-size dependence allows), in out[b][0 .. lengths[b]).
 * The zero tail: out[b][lengths[b] .. L) is written as 0.0f.  With zero-padded rows on the input side too, lass_sdr_stats and
 * lass_mix_at_snr work on the padded rows unchanged - their sums gain only exact zeros and the 1/L of their two means cancels.
 * Bucket membership is the CALLER'S to check: the library never reads the array on the host.  The kernels clamp every entry
 * into the interval above, so a wrong length gives a wrong clip and never an access out of range.
 * Everything else is lass_separate's: both kinds of context, all compute modes, lass_workspace_bytes(B, L), the half-batch
 * split (the second half reads lengths + B/2) and graph replay - the key includes the `lengths` POINTER, its contents are
 * read when the graph runs, so a caller that keeps its buffers may rewrite the lengths between calls.
 * NULL lengths: LASS_ERR_ARG. */
int lass_separate_ragged(lass_ctx* ctx, const float* mixture, const int* lengths, const float* condition, float* out,
                         int B, int L, void* workspace, size_t workspace_bytes, void* stream);
/* Host helper, launches nothing: the closed interval [*lo, *hi] of lengths that may share a call whose rows are L samples long
 * on this context (*hi == L).  <0 for L <= n_fft/2.  Either output may be NULL. */
int lass_ragged_bucket(const lass_ctx* ctx, int L, int* lo, int* hi);

/* ---- long recordings: windows of one long row, stitched on the device --------------------------------------------- */

/* lass_separate for B windows of ONE recording.  recording and out are rows of `total` floats; window b is the W-sample clip
 * recording[s_b .. s_b + W) with s_b = starts[b], separated exactly as lass_separate separates that clip alone (reflect padding
 * at the window's own two ends, as the reference does for its chunks).  Of its W output samples only lo_b <= n < hi_b are
 * stored, at out[s_b + n], with (lo_b, hi_b) = (keep[2b], keep[2b+1]).  NO OTHER SAMPLE OF out IS TOUCHED: it keeps its previous
 * value, so consecutive calls on the same `out` stitch a recording of any length in place.  A window with lo_b == hi_b stores
 * nothing (planners pad a group of windows with such rows).
 * starts: DEVICE int64 (B); keep: DEVICE int32 (2B).  The library never reads either array on the host; the kernels clamp
 * instead - s_b into [0, total - W], lo_b into [0, W], hi_b into [lo_b, W] - so a wrong entry gives wrong audio and never an
 * access out of range.  The kept ranges [s_b + lo_b, s_b + hi_b) of one call must be DISJOINT (the two half-batches store from
 * two streams): the caller's duty.  recording and out must not overlap (LASS_ERR_ARG).
 * f32: a kept sample is bit-identical to the gathered window's through lass_separate (any batch size, any position); the bf16
 * modes: as lass_separate at the same B and row positions.
 * Everything else is lass_separate's: both kinds of context, all compute modes, lass_workspace_bytes(B, W), the half-batch
 * split (the second half reads starts + B/2 and keep + 2*(B/2), the same recording and out) and graph replay - the key includes
 * the two POINTERS and total, their contents are read when the graph runs, so a caller that keeps its buffers rewrites the
 * arrays between calls and every group of windows from the third on is one graph launch.
 * LASS_ERR_ARG: a null pointer, B <= 0, W <= n_fft/2, total < W, overlapping recording / out. */
int lass_separate_windows(lass_ctx* ctx, const float* recording, int64_t total, const int64_t* starts, const int* keep,
                          const float* condition /* (B,512) */, float* out /* total floats */, int B, int W,
                          void* workspace, size_t workspace_bytes, void* stream);

/* lass_separate_windows with cross-faded seams.  Everything of lass_separate_windows holds - clamping of starts / keep, both kinds
 * of context, both STFT geometries, all compute modes, lass_workspace_bytes(B, W), the split, graph replay - and the kept range of
 * a window may begin and / or end with a FADE REGION whose samples are not stored but weighted and ADDED to `out`.
 * fade: DEVICE int32 (2B), (fade-in flag, fade-out flag) of window b, any non-zero value meaning set; ramp: DEVICE f32 (F), the
 * fade-in weights in ascending order (the fade-out reads the table backwards).  With (lo, hi) the clamped keep of window b and y
 * its W output samples:
 *   fade-in region,  if fade[2b]   != 0: n in [lo, min(lo + F, hi)),                                 weight ramp[n - lo];
 *   fade-out region, if fade[2b+1] != 0: n in [max(hi - F, end of the fade-in region), hi),          weight ramp[hi - 1 - n].
 * Both table indices lie in [0, F) by construction: a wrong entry gives wrong audio and never an access out of range, and the
 * library never reads either array on the host.  A sample of [lo, hi) in neither region is stored as by lass_separate_windows,
 * bit for bit; a sample of a region contributes the f32 product w * y[n], rounded once, ADDED to out[starts[b] + n] (one
 * hardware f32 atomic add per sample).
 * PRECONDITION: every sample that any window reaches through a fade region holds 0.0f before the first call that reaches it
 * (zero-fill `out` once).  POSTCONDITION: once every window that reaches a sample has run, the sample equals
 * fl(fl(w_a * y_a) + fl(w_b * y_b)) - in any grouping of the windows into calls, at any batch size, on either half-batch, eager
 * or replayed: f32 addition commutes and 0 + a is exact, so two adds onto a zero give the same bits in either order.  (Products
 * below the smallest normal f32 may be flushed to zero by the hardware add.)
 * THE CALLER'S DUTY, across all the calls that stitch one `out`: a plainly stored range overlaps nothing, and a fade region
 * coincides with at most ONE other fade region (the neighbouring window's complementary one).  lass_amd.longform plans and checks
 * such calls.
 * Graph replay: the key gains the fade and ramp POINTERS and F; their contents are read when the graph runs.  The second
 * half-batch reads fade + 2*(B/2).
 * LASS_ERR_ARG, nothing launched: whatever lass_separate_windows refuses, a null fade or ramp, F < 1, F > W. */
int lass_separate_windows_faded(lass_ctx* ctx, const float* recording, int64_t total, const int64_t* starts, const int* keep,
                                const int* fade, const float* ramp, int F, const float* condition /* (B,512) */,
                                float* out /* total floats */, int B, int W, void* workspace, size_t workspace_bytes, void* stream);

/* ---- linked channels: one mask from a guide signal, applied to every channel ------------------------ */

/* A multi-channel recording as ONE separation: a GUIDE signal (the caller's: the mono down-mix, a mid signal, ...) decides the
 * mask, and `channels` PLANES are masked with it.  For each clip or window b the network runs exactly as in the unlinked call on
 * the guide - x0 = bn0(|STFT(guide_b)|), condition[b] - but its output head meets a unit spectrum (mag = 1, cos = 1, sin = 0), so
 * what it leaves in out_real / out_imag is the complex mask M_b itself, (T, n_fft/2+1), Nyquist column 0.  For each channel c:
 *   X = STFT(plane_{c,b})                          the front end's own transform (the bits of lass_stft_magphase's real / imag)
 *   Y_re = fl(fl(X_re M_re) - fl(X_im M_im))       four products and two sums, each rounded once, no fused multiply-add
 *   Y_im = fl(fl(X_re M_im) + fl(X_im M_re))       (rows beyond a ragged clip's own frames are exact zeros)
 *   out_c = the iSTFT of the call's clip form      kept ranges, zero tails and fade regions as in the unlinked call
 * Channel c's input is laid out exactly like the guide - (B, L) rows, or one row of `total` floats - and starts c * plane_stride
 * floats after `planes`; its output is laid out the same way and starts c * out_plane_stride floats after `out`.  A plane's result
 * does not depend on the other planes or on `channels`.  1 <= channels <= LASS_MAX_LINKED_CHANNELS (the export kernels' limit).
 * ResUNet30 contexts at both STFT geometries, all compute modes, lass_workspace_bytes(B, L) as for the unlinked calls; the
 * half-batch split offsets the planes as it offsets the guide, and the graph key gains the planes pointer, the two strides and the
 * channel count.  The mask costs one network pass whatever `channels`; each channel adds one STFT and one iSTFT launch.
 * Workspace taps after a linked call (lass_workspace_tensor): "out_real" / "out_imag" hold M; "mag" / "cos" / "sin" are SCRATCH
 * (the unit spectrum until the head has run, then the last channel's Y_re / Y_im in "mag" / "cos").
 * LASS_ERR_ARG, nothing launched and nothing written: whatever the unlinked call refuses, a null `planes`, channels outside
 * 1 ... 8, a plane stride (either one) shorter than one channel's array (B * L, or total), `out` (any channel's) overlapping the
 * guide or any input plane, a multi-STFT context. */
#define LASS_MAX_LINKED_CHANNELS 8
/* lengths: DEVICE int32 (B) as in lass_separate_ragged, or NULL: every clip is L samples long (the dense form) */
int lass_separate_ragged_linked(lass_ctx* ctx, const float* guide /* (B,L) */, const int* lengths, const float* planes,
                                int64_t plane_stride, int channels, const float* condition /* (B,512) */, float* out,
                                int64_t out_plane_stride, int B, int L, void* workspace, size_t workspace_bytes, void* stream);
/* starts, keep as in lass_separate_windows; fade, ramp, F as in lass_separate_windows_faded, given together, or both NULL (F is
 * then ignored): hard seams.  With fades every output plane must hold 0 in the fade regions beforehand. */
int lass_separate_windows_linked(lass_ctx* ctx, const float* guide /* total floats */, int64_t total, const int64_t* starts,
                                 const int* keep, const int* fade, const float* ramp, int F, const float* planes,
                                 int64_t plane_stride, int channels, const float* condition /* (B,512) */, float* out,
                                 int64_t out_plane_stride, int B, int W, void* workspace, size_t workspace_bytes, void* stream);

/* Graph replay.  The third consecutive lass_separate call with the same pointers and shape is captured into a hipGraph
 * and replayed on the caller's stream from then on (one graph per context; a different combination is captured anew
 * after it, too, has been seen three times in a row).  Nothing else about the call changes; profiled
 * contexts and LASS_GRAPH=0 stay eager.  Returns 1 if replay is enabled, 0 if not; counters are optional outputs. */
int lass_graph_stats(const lass_ctx* ctx, long* captures, long* replays);
/* Turns graph replay off (0: every call launches its kernels eagerly) or back on (cached graphs are replayed again).
 * A measurement switch - bench.py times both forms of the same step - with no effect on results. */
int lass_set_graph_replay(lass_ctx* ctx, int enabled);
/* f32: the 3x3 convs at the 32-frame x 16-bin level run as split-K Winograd F(4x4,3x3) launches with a fixed number of
 * splits (4, whatever the batch: a clip's bits do not depend on its batch).  An internal hook for the tests: splits = 1, 2
 * or 4 forces that number on the stage calls and lass_separate alike (1 = the unsplit kernels), 0 restores the default.  Query lass_workspace_bytes again
 * afterwards: the partial sums live in the workspace. */
int lass_set_wino4_splits(lass_ctx* ctx, int splits);
/* f32: the F(4x4,3x3) layers with many output-channel groups read their transformed input from an image that one prep launch
 * writes (into the workspace), instead of every group's workgroups transforming the same tiles again.  The rule looks at the
 * layer's shape only, never at the batch.  mode 0 = off, 1 = the measured routing (default), 2 = every layer whose kind admits
 * it (tests, A/B).  Query lass_workspace_bytes again afterwards. */
int lass_set_wino4_vprep(lass_ctx* ctx, int mode);
/* f32: lass_separate's last launch (decoder_block6's conv2 + 1x1 shortcut with the output head in its epilogue) runs on weights
 * that lass_finalize composed with after_conv - nothing non-linear sits between the two, so the 3 mask logits are one linear map
 * of the launch's inputs and the block's 32 output channels are never formed.  1 = that route (default), 0 = the unfolded launch
 * (A/B, tests; LASS_HEAD_FOLD at lass_create).  The two differ by f32 rounding only (the last linear layer is re-associated).  The
 * stage calls, LASS_WINO4=0 and the bf16 modes have no folded form and ignore the switch. */
int lass_set_head_fold(lass_ctx* ctx, int enabled);
/* f32, under head_fold = 1, the single-window ResUNet30: that launch reads decoder_block6's concat only to apply the composed 1x1
 * shortcut.  With this route the shortcut's 3 logits are formed where the two halves of the concat are produced - the skip in
 * encoder_block1.conv2's epilogue, the up-sampled half as 12 more columns of decoder_block6's transposed conv - and handed to the
 * head as two sets of planes (B, 3, frames, 512) in the workspace; the head then runs no shortcut phase.  1 = that route
 * (default), 0 = the head forms the shortcut itself (A/B, tests; LASS_HEAD_SC_FOLD at lass_create).  The two differ by f32
 * rounding only.  The multi-STFT model, the stage calls, LASS_WINO4=0, lass_set_head_fold(0) and the bf16 modes ignore the
 * switch.  Query lass_workspace_bytes again afterwards. */
int lass_set_head_sc_fold(lass_ctx* ctx, int enabled);
/* f32: the pointwise GEMMs (the 1x1 shortcuts of the deep blocks, the transposed convs from 128 input channels up) multiply on the
 * bf16 matrix unit at f32 accuracy: each f32 operand is split exactly into three bf16 pieces and six of the nine piece products
 * are summed in f32 in one fixed order (the three dropped ones are ~2^-24 of the product).  1 = that kernel (default), 0 = the
 * f32-MFMA kernel (A/B, tests; LASS_PW_SPLIT at lass_create).  The switch picks the kernel of those launches and nothing else:
 * which layers they are, and every workspace size, stay as they were.  The two differ by f32 rounding only.  Non-finite
 * activations are outside the split's contract.  The bf16 modes run no such launch and ignore the switch. */
int lass_set_pw_split(lass_ctx* ctx, int enabled);
/* f32: the F(4x4,3x3) convs with 384 output channels that read their transformed input from memory (both convs of encoder_block5-6
 * and decoder_block1-2) run as three launches - a scatter that writes the transformed input in GEMM layout, 36 batched GEMMs on the
 * bf16 matrix unit at f32 accuracy (the split of lass_set_pw_split, on weight images lass_finalize keeps: 216 bytes per (cin, cout)
 * pair), and a gather that applies the output transform and the epilogue.  1 = that route (default), 0 = the prep + conv (+ combine)
 * launches (A/B, tests; LASS_WINO4_GEMM at lass_create).  The two differ by f32 rounding only; a clip's result never depends on its
 * batch on either.  The rule looks at the layer's shape only.  The bf16 modes, LASS_WINO4=0, lass_set_wino4_vprep(0) and a forced
 * split factor (lass_set_wino4_splits) never take the route.  Query lass_workspace_bytes again afterwards. */
int lass_set_wino4_gemm(lass_ctx* ctx, int enabled);
/* UNSTABLE, tests only - not part of the supported interface, and may change or go without notice; lass_separate never looks at
 * it.  The stage calls (lass_convblock, lass_encoder_block) keep that image in `v` (`floats` f32 of device memory owned by the
 * caller) instead of a buffer of the context; NULL restores the context's.  A buffer that is too small for a layer, or overlaps
 * its tensors, makes the stage call return LASS_ERR_STATE without launching.  (The tests use it to place the image where the
 * overlap check must refuse it, and to see that a layer's prep launch wrote it.) */
int lass_set_wino4_vprep_buffer(lass_ctx* ctx, float* v, size_t floats);

/* The same path from a PRECOMPUTED analysis of the mixtures, as the reference's multi-STFT wrapper takes it
 * (resunet_with_multistft.py:233-241: input_dict["stft_mixture_mag" / "_cos" / "_sin"][win]; producer:
 * scripts/precompute_stfts.py:19-58 = lass_stft_components): mag[k] (B,T,n_fft/2+1) for each analysis window k in the
 * context's order, cos / sin of the mask window only.  L = target waveform length, T = 1 + L/160. */
int lass_separate_components(lass_ctx* ctx, const float* const* mag, const float* cos_mask, const float* sin_mask,
                             const float* condition, float* out, int B, int L, void* workspace, size_t workspace_bytes,
                             void* stream);

/* ---- stage entry points (used by the parity tests; same kernels lass_separate launches) --------------------- */

/* Centred STFT (n_fft=win=1024, hop 160, reflect pad, periodic Hann; on a lass_create_stft context its (n_fft, hop)) fused with
 * magnitude/phase.  wav (B,L) -> mag, cos, sin (B,T,n_fft/2+1 = 513), T = 1 + L/hop.  Any of mag/cos/sin/real/imag may be NULL.
 * mag = sqrt(max(re^2+im^2, 1e-10)), cos = re/mag, sin = im/mag.
 * Replaces: Base.wav_to_spectrogram_phase (base.py:83-113) + torchlibrosa STFT.forward. */
int lass_stft_magphase(lass_ctx* ctx, const float* wav, int B, int L, float* mag, float* cos_out, float* sin_out,
                       float* real_out, float* imag_out, void* stream);

/* Multi-resolution analysis front end ("next" row f3): n_windows centred STFTs of the same waveforms in one launch
 * (n_fft = win_length in {256,512,1024,2048}, periodic Hann, reflect pad, common hop), each as magnitude / cos / sin
 * with torchlibrosa-magphase semantics (mag = sqrt(re^2+im^2); cos = re/max(mag,1e-10); sin likewise).
 * wav (B,L) -> mag[i], cos_out[i], sin_out[i] (B,T,win_lengths[i]/2+1), T = 1 + L/hop; at most 4 windows.
 * Replaces: calculate_stft_components (scripts/precompute_stfts.py:19-58) looped over stft_win_lengths (:573-590;
 * config stft_win_lengths [256,512,2048], hop 160). */
int lass_multi_stft(lass_ctx* ctx, const float* wav, int B, int L, int hop, int n_windows, const int* win_lengths,
                    float* const* mag, float* const* cos_out, float* const* sin_out, void* stream);

/* `calculate_stft_components(waveform, n_fft, hop, win_length, "hann", True, "reflect")` (scripts/precompute_stfts.py:
 * 19-58) for several win_length at one COMMON n_fft (1024 or 2048; each periodic Hann window zero-padded, centred) in one
 * launch, torchlibrosa-magphase semantics: wav (B,L) -> mag[i], cos_out[i], sin_out[i] (B,T,n_fft/2+1), T = 1 + L/hop.
 * This is the producer of the multi-STFT model's wire format. */
int lass_stft_components(lass_ctx* ctx, const float* wav, int B, int L, int n_fft, int hop, int n_windows,
                         const int* win_lengths, float* const* mag, float* const* cos_out, float* const* sin_out,
                         void* stream);

/* Inverse STFT: real, imag (B,T,513) -> wav (B,L): inverse transforms, overlap-add, division by the window-sum-square
 * envelope and trim fused in one kernel.  frames_ws is unused since 1.1 (no frame scratch exists any more); may be NULL.
 * Replaces: torchlibrosa ISTFT.forward as called at resunet.py:510. */
int lass_istft(lass_ctx* ctx, const float* real, const float* imag, int B, int T, int L, float* wav,
               float* frames_ws, void* stream);
/* The same for n_fft in {1024, 2048} and a synthesis window of win_length <= n_fft (zero-padded, centred), at the context's
 * hop (160; a (2048, 320) context of lass_create_stft: hop 320, n_fft 2048 only):
 * real, imag (B,T,n_fft/2+1) -> wav (B,L).  Replaces: ISTFT(n_fft, hop, win_length) of resunet_with_multistft.py:36-44. */
int lass_istft_nfft(lass_ctx* ctx, const float* real, const float* imag, int B, int T, int L, int n_fft, int win_length,
                    float* wav, void* stream);

/* FiLM + BN folding for a batch of conditions: shift (B, n_shift) where n_shift = lass_film_width(ctx); column
 * layout is given by lass_film_offset().  shift[b, off+c] = bn_beta[c] - mean[c]*s[c] + (W_site cond_b + b_site)[c].
 * Replaces: FiLM.forward (resunet.py:59-81) for the 32 sites whose output is read. */
int lass_film(lass_ctx* ctx, const float* condition, int B, float* shift, void* stream);
int lass_film_width(const lass_ctx* ctx);
/* Column offset of a site ("encoder_block1->conv_block1->beta1", "decoder_block2->beta1", ...) or -1. */
int lass_film_offset(const lass_ctx* ctx, const char* site);
/* Raw FiLM vectors (no BN folding): film (B, n_shift) = W cond + b.  For parity tests against the golden film vectors. */
int lass_film_raw(lass_ctx* ctx, const float* condition, int B, float* film, void* stream);

/* One residual block (resunet.py:147-165) by reference module prefix, e.g. "base.encoder_block2.conv_block1" or
 * "base.decoder_block3.conv_block2".  x (B,Cin,H,W) NCHW f32 -> y (B,Cout,H,W).  shift is the lass_film() output for
 * the same batch.  scratch: B*Cout*H*W floats. */
int lass_convblock(lass_ctx* ctx, const char* prefix, const float* x, int B, int H, int W, const float* shift,
                   float* y, float* scratch, void* stream);

/* One encoder block (resunet.py:186-198) by module name, e.g. "base.encoder_block3": the ConvBlockRes above plus
 * F.avg_pool2d with the block's downsample ((2,2); (1,2) for encoder_block6) - fused into conv2's epilogue exactly as
 * lass_separate does it (its own kernel when H is not divisible).  x (B,Cin,H,W) -> y (B,Cout,H,W) and
 * pool (B,Cout,H/dh,W/2).  "base.conv_block7a" (downsample (1,1) = identity) takes pool == NULL. */
int lass_encoder_block(lass_ctx* ctx, const char* name, const float* x, int B, int H, int W, const float* shift, float* y,
                       float* pool, float* scratch, void* stream);

/* STFT + magnitude/phase + the network-input prologue of ResUNet30_Base.forward (resunet.py:533-552): bn0 over
 * frequency, zero-padding of T to a multiple of 32 AFTER bn0, last bin dropped.  wav (B,L) -> x0 (B,Tpad,512) and,
 * where non-NULL, mag/cos/sin (B,T,513).  pre_conv (:555) is applied inside encoder_block1's staging.
 * Multi-STFT context: x0 is (n_windows,B,Tpad,n_fft/2), one slab per analysis window; mag/cos/sin (B,T,n_fft/2+1) are
 * the mask window's. */
int lass_front_end(lass_ctx* ctx, const float* wav, int B, int L, float* mag, float* cos_out, float* sin_out, float* x0,
                   void* stream);

/* lass_front_end with a length per clip (lengths: DEVICE int32 (B), as in lass_separate_ragged; shapes as for B clips of L
 * samples: T = 1 + L/160, Tpad = 32*ceil(T/32)).  With Tb = 1 + lengths[b]/160: rows t < Tb of clip b are what lass_front_end
 * writes for that clip alone; rows Tb <= t < Tpad of x0 (every analysis window) and rows Tb <= t < T of mag/cos/sin are 0. */
int lass_front_end_ragged(lass_ctx* ctx, const float* wav, const int* lengths, int B, int L, float* mag, float* cos_out,
                          float* sin_out, float* x0, void* stream);
/* lass_istft_nfft with a length per clip: real, imag (B,T,n_fft/2+1) with T = 1 + L/160 -> wav (B,L).  Only frames
 * t < 1 + lengths[b]/160 of clip b are overlap-added; wav[b][0 .. lengths[b]) is what lass_istft_nfft gives for the clip
 * alone, wav[b][lengths[b] .. L) is 0. */
int lass_istft_ragged(lass_ctx* ctx, const float* real, const float* imag, const int* lengths, int B, int T, int L, int n_fft,
                      int win_length, float* wav, void* stream);

/* lass_front_end for the windows recording[starts[b] .. starts[b] + W) of one row of `total` floats (starts: DEVICE int64 (B),
 * clamped as in lass_separate_windows): shapes as for B clips of W samples, row b what lass_front_end writes for the gathered
 * window, bit for bit. */
int lass_front_end_windows(lass_ctx* ctx, const float* recording, int64_t total, const int64_t* starts, int B, int W, float* mag,
                           float* cos_out, float* sin_out, float* x0, void* stream);
/* lass_istft_nfft for windows: real, imag (B,T,n_fft/2+1) with T = 1 + W/160 -> out (total floats).  Of window b only samples
 * keep[2b] <= n < keep[2b+1] are stored, at out[starts[b] + n], each what lass_istft_nfft gives for a clip of W samples; the
 * rest of `out` is not touched.  2 560-sample spans of a window that do not meet its kept range run no transform.  (T = 1 + W/hop
 * with the context's hop, as everywhere.) */
int lass_istft_windows(lass_ctx* ctx, const float* real, const float* imag, const int64_t* starts, const int* keep, int64_t total,
                       int B, int T, int W, int n_fft, int win_length, float* out, void* stream);
/* lass_istft_windows with the fade regions of lass_separate_windows_faded (fade: DEVICE int32 (2B), ramp: DEVICE f32 (F),
 * 1 <= F <= W): samples of a region are weighted and ADDED to `out`, which must hold 0 there beforehand. */
int lass_istft_windows_faded(lass_ctx* ctx, const float* real, const float* imag, const int64_t* starts, const int* keep,
                             const int* fade, const float* ramp, int F, int64_t total, int B, int T, int W, int n_fft,
                             int win_length, float* out, void* stream);

/* The per-channel stage of the linked calls, for callers with a mask of their own: plane (B,L) and the complex mask m_re, m_im
 * (B,T,n_fft/2+1) -> y_re, y_im (B,T,n_fft/2+1), Y = STFT(plane) * M by the rule of lass_separate_ragged_linked, with the context's
 * transform (ResUNet30 contexts only).  lengths: DEVICE int32 (B) or NULL = dense; rows beyond a ragged clip's frames are 0. */
int lass_masked_stft(lass_ctx* ctx, const float* plane, const int* lengths, int B, int L, const float* m_re, const float* m_im,
                     float* y_re, float* y_im, void* stream);
/* ... for the windows recording[starts[b] .. starts[b] + W) of one row of `total` floats (starts clamped as everywhere) */
int lass_masked_stft_windows(lass_ctx* ctx, const float* recording, int64_t total, const int64_t* starts, int B, int W,
                             const float* m_re, const float* m_im, float* y_re, float* y_im, void* stream);

/* Where lass_separate(B, L) leaves a named intermediate inside the caller's workspace (f32 compute mode; in the bf16
 * modes several of these hold blocked bf16 data instead): byte offset, shape (B,C,H,W) and element strides.  Names:
 * "mag" "cos" "sin" "x0" "out_real" "out_imag", "encoder_blockN" (the skip, stored in place inside the decoder's concat
 * buffer), "encoder_blockN.pool", "conv_block7a", "decoder_blockN.up" (transposed-conv half of the concat),
 * "decoder_blockN" (N = 6 is consumed by the fused output head and never written).  For parity tests of the fused
 * stages against the reference's own taps.  Returns LASS_ERR_ARG for an unknown name, and LASS_ERR_STATE when the LAST
 * lass_separate of this (B, L) ran as part-batches (the replayed graph of an even batch >= 8, or LASS_SPLIT=2): the workspace
 * then holds their layouts.  After an eager, unsplit call (the first calls of a key, LASS_GRAPH=0, changing pointers) the taps
 * of any batch size are readable. */
int lass_workspace_tensor(const lass_ctx* ctx, int B, int L, const char* name, size_t* offset, int64_t shape[4],
                          int64_t strides[4]);

/* Transposed conv of a decoder block (resunet.py:254-255): x (B,Cin,h,w) -> y (B,Cout,h*sh,w*sw), with the
 * bn1 + FiLM + leaky-ReLU prologue.  name: "base.decoder_blockN". */
int lass_upconv(lass_ctx* ctx, const char* name, const float* x, int B, int h, int w, const float* shift, float* y,
                void* stream);

/* after_conv (1x1, 32->3, +bias) + complex-mask application (resunet.py:570-574, :469-495):
 * x12 (B,32,Tpad,512), mag/cos/sin (B,T,513) -> out_real, out_imag (B,T,513); bin 512 is exactly 0. */
int lass_mask_apply(lass_ctx* ctx, const float* x12, const float* mag, const float* cos_in, const float* sin_in,
                    int B, int T, int Tpad, float* out_real, float* out_imag, void* stream);

/* Per-clip statistics for SDR / SI-SDR (utils.py:148-200): stats (B,6) f64 =
 * [sum ref^2, sum est^2, sum ref*est, sum (est-ref)^2, sum (a*ref)^2, sum (est-a*ref)^2],
 * a = (eps32 + <ref,est>)/(<ref,ref> + eps32), eps32 = FLT_EPSILON.  dB math is the host's. */
int lass_sdr_stats(lass_ctx* ctx, const float* ref, const float* est, int B, int L, double* stats, void* stream);

/* Evaluator data path ("next" row f1): build B mixtures at given SNRs on the device.
 * source (B,L) in/out, noise (B,L), snr_db (B) -> mixture (B,L):
 *   mixture = source + noise * sqrt(mean(source^2) / 10^(snr/10) / mean(noise^2));
 *   if max|mixture| > 1: source *= 0.9/max and mixture *= 0.9/max   (declipping; source is modified in place).
 * scratch: 4*B doubles.  Replaces: the numpy mixing block of DCASEEvaluator.__call__ (dcase_evaluator.py:77-89). */
int lass_mix_at_snr(lass_ctx* ctx, float* source, const float* noise, const float* snr_db, float* mixture, int B, int L,
                    double* scratch, void* stream);

/* Evaluator load path: B rows of raw WAV payload -> B mono float32 clips at the target rate, in one launch.
 * raw: row b = `frames` interleaved sample frames of `channels` samples at raw + b * row_stride_bytes (little-endian, as
 * in the file's data chunk); encoding LASS_WAV_PCM16 (x/32768), LASS_WAV_PCM32 (round-to-nearest int -> float, then * 2^-31)
 * or LASS_WAV_F32; channels (1 ... 8) are summed in ascending order in float32 and divided by their count, correctly rounded.
 * Then the polyphase FIR of scipy.signal.resample_poly (padtype "constant"):
 *   out[b][n] = sum_m x[b][m] * taps[n*down - m*up + (n_taps-1)/2],   x = 0 outside the clip,   n < L_out = ceil(frames*up/down)
 * accumulated in float32 fmaf, in one fixed tap order per output (bit-identical whatever B, the row stride or the call);
 * indices are 64-bit.  taps: the prototype filter (device, float32, natural order; lass_amd.resample.design_taps builds
 * scipy's default).  up == down == 1 decodes and down-mixes only (taps may then be NULL, n_taps 1).
 * Limits, checked before anything is launched (LASS_ERR_ARG): encoding one of the three, 1 <= channels <= 8,
 * 1 <= up, down <= LASS_RESAMPLE_MAX_RATIO, n_taps odd and <= LASS_RESAMPLE_MAX_TAPS (the prototype filter is a 64 KiB table
 * at most; the kernel keeps it in LDS phase by phase, up * (ceil(n_taps/up) | 1) floats, which must stay within
 * LASS_RESAMPLE_MAX_TABLE floats = half of the CU's 160 KiB - true of every design_taps filter under the tap cap - so that
 * the input span of at least one output always fits beside it), L_out equal to the ceiling above, row_stride_bytes a multiple
 * of 4 and >= frames * channels * bytes per sample, raw 4-byte aligned, B <= 65535.  Stateless; out (B, L_out) is dense.
 * Replaces: librosa.load(path, sr=16000, mono=True) (dcase_evaluator.py:73-74) behind the file read, for the encodings above;
 * librosa resamples with soxr_hq, this is the project's scipy-style filter (parity unpinned against librosa, as on the host). */
#define LASS_WAV_PCM16 0
#define LASS_WAV_PCM32 1
#define LASS_WAV_F32 2
#define LASS_RESAMPLE_MAX_TAPS 16383
#define LASS_RESAMPLE_MAX_TABLE 20480
#define LASS_RESAMPLE_MAX_RATIO 65536
int lass_decode_resample(lass_ctx* ctx, const void* raw, int64_t row_stride_bytes, int B, int frames, int channels, int encoding,
                         int up, int down, const float* taps, int n_taps, float* out, int L_out, void* stream);

/* The same load without the down-mix: out (B, channels, L_out) float32, dense, one plane per channel.  Arguments and limits are
 * lass_decode_resample's.  Plane c of row b is bit-identical to what lass_decode_resample writes for a mono payload holding
 * channel c of that row alone (the same decode rule, tap order and fmaf chain), whatever B, the row stride or the call.  For
 * callers that separate every channel of a recording on its own and keep the channel layout. */
int lass_decode_resample_planar(lass_ctx* ctx, const void* raw, int64_t row_stride_bytes, int B, int frames, int channels,
                                int encoding, int up, int down, const float* taps, int n_taps, float* out, int L_out, void* stream);

/* Export path, the mirror of lass_decode_resample: B recordings as planar float32 at the model rate -> B WAV data chunks at the
 * file's rate, in one launch.  planes: plane c of recording b = L_in floats at planes + b*row_stride + c*plane_stride (strides
 * in floats; channels 1 ... 8).  For every plane
 *   y[n] = sum_m x[m] * taps[n*down - m*up + (n_taps-1)/2],   x = 0 outside the plane,   n < frames_out <= ceil(L_in*up/down)
 * which is lass_decode_resample's formula for a mono LASS_WAV_F32 payload in the same accumulation order: y is bit-identical to
 * what that entry point writes for the plane, whatever B, the strides or the call.  frames_out below the ceiling truncates (a
 * file decoded from F frames comes back at F frames: ceil(ceil(F*u/d)*d/u) >= F).  up == down == 1: no filter (taps may be
 * NULL, n_taps 1).  Then row b = frames_out frames of `channels` interleaved samples at out_bytes + b*out_row_stride_bytes,
 * little-endian, as a WAV data chunk holds them:
 *   LASS_WAV_PCM16  clip(rintf(y * 32768), -32768, 32767), ties to even   (wavio.write_wav_pcm16, for every finite float32)
 *   LASS_WAV_PCM32  rintf(y * 2^31) clipped to [-2^31, 2^31 - 1]          (wavio.write_wav_pcm32)
 *   LASS_WAV_F32    y as is                                               (wavio.write_wav_f32)
 * A NaN encodes as PCM 0.  clipped (optional, device, B unsigned counters zero-filled by the caller): counter b grows by the
 * number of PCM samples of row b that the clip changed (integer atomics: order-independent); LASS_WAV_F32 adds nothing.
 * Limits, checked before anything is launched (LASS_ERR_ARG): those of lass_decode_resample on encoding, channels, up, down,
 * taps, n_taps, the polyphase table and B; L_in >= 1; 1 <= frames_out <= the ceiling above; plane_stride >= L_in and
 * row_stride >= (channels-1)*plane_stride + L_in; out_bytes 4-byte aligned, out_row_stride_bytes a multiple of 4 and
 * >= frames_out * channels * bytes per sample.  Stateless; bytes of a row past its frames_out frames are left alone. */
int lass_resample_encode(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                         int up, int down, const float* taps, int n_taps, int encoding, void* out_bytes,
                         int64_t out_row_stride_bytes, int frames_out, unsigned* clipped, void* stream);

/* ---- levelled export: loudness meter, peak, gain (opt-in; lass_amd.pipeline.separate_files(loudness=, peak_ceiling_db=)) ---- */

/* The ITU-R BS.1770-4 gated integrated loudness of B recordings, on the device.  planes, row_stride, plane_stride, channels:
 * as lass_resample_encode addresses its planes, L floats each; lengths (device, B int32, or NULL: every recording L samples):
 * recording b is the first lengths[b] samples of its planes (values outside 0 ... L are clamped).  hop = rate / 10 samples
 * (100 ms; the rate must be a multiple of 10).  coef (HOST, 10 doubles): the K-weighting biquads for that rate, b0 b1 b2 a1 a2
 * of the high shelf, then of the high-pass, a0 == 1 (lass_amd.loudness.coefficients).  weights (device, `channels` floats, or
 * NULL: all 1): the channel weights G_i.  For every recording:
 *   y_c = the cascade on plane c, direct form II transposed, zero initial state, state and products in float64;
 *   p_j = sum_c G_c * mean(y_c[j*hop .. j*hop + 4*hop)^2),   j < nb = (len - 4*hop) / hop + 1  (0 if len < 4*hop): whole blocks only;
 *   l_j = -0.691 + 10 log10 p_j;  absolute gate l_j > -70;  relative gate l_j > (-0.691 + 10 log10 mean of the abs-gated p) - 10;
 *   out[b] = { -0.691 + 10 log10 (mean of the doubly gated p), or -inf when no block survives;  nb;  surviving blocks }
 * out: (B,3) doubles.  blocks (optional, (B, nb_max) doubles): row b receives p_0 ... p_{nb-1}, then zeros.
 * The recurrence is cut into hop bins (one wave each, its lanes on consecutive sub-runs), carried over the cuts with powers of
 * the cascade's state matrix formed here on the host in float64; every cut is a multiple of hop from the plane's first sample and
 * every sum has one fixed order, so a recording's three numbers and its blocks are bit-identical whatever B, its row, the
 * strides or the call.  No floating-point atomics; nothing is read back.
 * scratch: 5 * B * channels * (L / hop) doubles (device, 8-byte aligned), scratch_bytes its size.
 * Limits, checked before anything is launched (LASS_ERR_ARG): 1 <= channels <= 8, B * channels <= 65535,
 * 1 <= hop <= LASS_LOUDNESS_MAX_HOP, plane_stride >= L, row_stride >= (channels-1)*plane_stride + L, coef finite with both pole
 * pairs inside the unit circle, nb_max >= the blocks of L samples when blocks is given, scratch large enough.  Stateless.
 * Replaces: pyloudnorm.Meter(rate).integrated_loudness (data/waveform_mixers.py:119-120) for the export path; written from the
 * recommendation and pinned by the EBU Tech 3341 tones and the float64 host definition, not by a reference fixture. */
#define LASS_LOUDNESS_MAX_HOP 38400
int lass_loudness(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L,
                  const int* lengths, int hop, const double* coef, const float* weights, double* out, double* blocks, int nb_max,
                  void* scratch, size_t scratch_bytes, void* stream);

/* The sample peak of what lass_resample_encode would quantise: peak[b] (device, B floats, written here) = max |y[n]| over the
 * channels of recording b and n < frames_out, y that entry point's value before quantisation (one kernel body with it: the same
 * formula, tap order and fmaf chain).  Raised by integer atomic max on the bits of |y|: exact and order-independent; a NaN is
 * skipped, an infinity is a peak.  Arguments and limits: lass_resample_encode's up to frames_out, peak 4-byte aligned. */
int lass_resample_peak(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                       int up, int down, const float* taps, int n_taps, int frames_out, float* peak, void* stream);

/* One gain per recording from its loudness and peak (utils.py:293 gives the dB rule; the ceiling is scripts/process_audio.sh's
 * peak normalisation turned into a bound).  loudness (device, B doubles, -inf allowed), peak (device, B floats, may be NULL
 * without a ceiling), target_lufs (NaN: none), ceiling (linear, 0: none) -> gain (device, B floats):
 *   g = (float)10^((target_lufs - loudness[b]) / 20) if a target is given and loudness[b] is finite, else 1;
 *   if a ceiling is given and fl(g * peak[b]) > ceiling:  g = fl(ceiling / peak[b]), then one float32 ulp down while
 *   fl(g * peak[b]) > ceiling.   x -> fl(g * x) is monotone in |x|: no sample of the row, gained, exceeds the ceiling.
 * limited (optional, device, B int32): 1 where the ceiling bit, else 0.  lass_amd.loudness.gain_for is the same rule on the host. */
int lass_loudness_gain(lass_ctx* ctx, const double* loudness, const float* peak, int B, double target_lufs, float ceiling,
                       float* gain, int* limited, void* stream);

/* lass_resample_encode with a gain per recording: every y of recording b becomes fl(gain[b] * y) - one float32 multiplication,
 * rounded once - and is then quantised by lass_resample_encode's rule (gain: device, B floats).  The same kernel body:
 * gain[b] == 1 gives lass_resample_encode's bytes.  The other arguments and limits are that entry point's. */
int lass_resample_encode_gain(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels,
                              int L_in, int up, int down, const float* taps, int n_taps, int encoding, const float* gain,
                              void* out_bytes, int64_t out_row_stride_bytes, int frames_out, unsigned* clipped, void* stream);

/* ---- EBU R 128 delivery: true peak, loudness range and maxima (opt-in; separate_files(peak="true", meter=True)) ---- */

/* The true peak of what lass_resample_encode would quantise: lass_resample_peak with the signal between the samples.  With y_c[n]
 * that entry point's float32 value before quantisation for n < frames_out, and zero outside,
 *   z_c[k] = sum_m y_c[m] * os_taps[k - m*os + 10*os],   k < os * frames_out
 * evaluated as lass_decode_resample evaluates an (up, down) = (os, 1) filter - one float32 fmaf chain over the 21 taps of the
 * output's phase, in that entry point's order - and
 *   peak[b] = max over c of max( max_n |y_c[n]| , max over k % os != 0 of |z_c[k]| ).
 * Phase 0 is the samples themselves and not the filtered samples, so a true peak is never under the sample peak.  peak[b] is
 * bit-identical to composing the public pieces (lass_decode_resample of the float32 plane, cut to frames_out, then of the result
 * at (os, 1)), whatever B, the row, the strides, the tile or the call; raised by integer atomic max on the bits, a NaN skipped.
 * os: 2 or 4 (lass_amd.loudness.oversampling; 1 is lass_resample_peak); os_taps: device, n_os_taps = 20*os + 1 floats, the float32
 * of lass_amd.resample.design_taps(os, 1); peak: device, B floats, written here.  One launch: a workgroup keeps the y of its tile
 * and of the 10 frames on either side of it that the 21 taps reach in LDS; no scratch, no float plane at the file's rate in memory.
 * Arguments and limits otherwise: lass_resample_peak's.  In addition a ratio at which the 21 first-stage frames of one
 * interpolated value no longer fit the CU's LDS beside the filter table (lass_amd.resample.true_peak_fits tells beforehand; far
 * down-sampling ratios such as 1:800) is refused with LASS_ERR_ARG before anything is launched. */
int lass_resample_true_peak(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels,
                            int L_in, int up, int down, const float* taps, int n_taps, int frames_out, int os, const float* os_taps,
                            int n_os_taps, float* peak, void* stream);

/* lass_loudness with the other figures an R 128 delivery is checked against.  Arguments: lass_loudness's, except that out is (B,10)
 * doubles and that short_term (optional, device, (B, ns_max) doubles, ns_max >= the short-term blocks of L samples) receives the
 * short-term powers, zeros past a recording's own count.  With S_c[i] the sum of the squared K-weighted samples of hop bin i,
 *   q_j = sum_c G_c * (S_c[j] + S_c[j+1] + ... + S_c[j+29]) / (30 hop),  j < ns = bins - 29 (0 under 30 bins): 3 s blocks, 100 ms apart.
 * out[b] = { columns 0 ... 2: what lass_loudness writes, bit for bit (the same kernels);
 *            3: maximum momentary loudness, -0.691 + 10 log10 max_j p_j, ungated;   4: maximum short-term loudness, the same of q;
 *            5: loudness range in LU (EBU Tech 3342): absolute gate l > -70, relative gate l > (loudness of the mean of the abs-gated
 *               q) - 20; of the n survivors sorted ascending p10 = v[floor((n-1)*0.10 + 0.5)], p95 = v[floor((n-1)*0.95 + 0.5)],
 *               LRA = 10 log10(p95 / p10);
 *            6: ns;   7: n;   8: p10;   9: p95 (powers) }
 * and -inf, -inf, 0, 0, 0, 0, 0 where there is nothing to measure.  The two order statistics are selected exactly (a radix select
 * on the bit patterns, integer atomics, any count); no floating-point atomics and one order per sum: a recording's ten numbers are
 * bit-identical alone and as any row of any batch.  scratch: (5 * channels + 1) * B * (L / hop) doubles. */
int lass_loudness_stats(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L,
                        const int* lengths, int hop, const double* coef, const float* weights, double* out, double* blocks,
                        int nb_max, double* short_term, int ns_max, void* scratch, size_t scratch_bytes, void* stream);

/* ---- look-ahead limiter of the levelled export (opt-in; separate_files(limiter=True)) ---- */

/* One gain curve per recording, linked across the channels, that holds gain x envelope under the ceiling, so that a ceiling that binds
 * no longer costs the whole recording its loudness.  planes: lass_resample_peak's (B recordings of `channels` planes of L floats at
 * the model rate, strides in floats); gain (device, B floats, finite, >= 0); ceiling (linear, > 0, finite); H: the reach in frames,
 * 1 ... LASS_LIMITER_MAX_H (lass_amd.loudness.reach); window (device, 2H + 1 floats: lass_amd.loudness.limiter_window); os: 1, 2 or 4
 * with os_taps (device, n_os_taps = 20*os + 1 floats, lass_resample_true_peak's) or NULL and 0 at os == 1.  For recording b, in
 * float32 with every operation rounded once:
 *   e[n] = max_c max( |x_c[n]| , max_{p=1..os-1} |z_c[n*os + p]| ),  z_c as lass_resample_true_peak forms it from a plane (one fmaf
 *          chain over the 21 taps of the phase: bit-identical to lass_decode_resample of the plane at (os, 1)); a NaN counts as 0;
 *   r[n] = 1 if a = fl(g * e[n]) <= ceiling, else fl(ceiling / a);
 *   m[n] = min r[k] over |k - n| <= H, 0 <= k < L;
 *   G[n] = sum_{j=-H..H} window[j+H] * m'[n+j] (m' = m inside the row, 1 outside), one fmaf chain in that order onto 0; G[n] = 1
 *          exactly where every m' in reach is 1; then G[n] = min(G[n], r[n]);
 *   out_c[n] = fl( fl(g * G[n]) * x_c[n] ).
 * out: addressed as planes with its own strides; it must not overlap planes (a tile's halo reads what a neighbour would write).
 * Optional outputs: curve and envelope ((B, L) floats, rows curve_row_stride >= L floats apart) receive G and e; min_gain (B floats,
 * written here) the smallest G of the row, lowered by integer atomic min on the bits; frames (B int32, written here) the number of
 * n with m[n] < 1, by integer atomic add.  lass_amd.loudness.limit is the float64 definition.
 * One launch, one workgroup per tile of LASS_LIMITER_TILE frames and recording, no scratch, no floating-point atomics: a tile keeps
 * the plane over tile +- (2H + 10), e over tile +- 2H and m over tile +- H in LDS and makes its neighbours' share again; the
 * minimum is a doubling scheme (O(log H) per frame), and the smoothing chain runs only in waves with some m' < 1 in reach.  A row's
 * outputs are bit-identical whatever B, the row, the strides or the call.  Nothing is read back.
 * Limits, checked before anything is launched (LASS_ERR_ARG): 1 <= B <= 65535, 1 <= channels <= 8, L >= 1, 1 <= H <=
 * LASS_LIMITER_MAX_H, os in {1, 2, 4} with its taps, ceiling > 0 and finite, plane_stride >= L and row_stride >=
 * (channels-1)*plane_stride + L for planes and for out, curve_row_stride >= L with curve or envelope, out disjoint from planes,
 * every pointer 4-byte aligned.  Stateless.  Not ported: the reference has no limiter (scripts/process_audio.sh peak-normalises). */
#define LASS_LIMITER_MAX_H 512
#define LASS_LIMITER_TILE 1024
int lass_limit(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L, int os,
               const float* os_taps, int n_os_taps, const float* gain, float ceiling, int H, const float* window, float* out,
               int64_t out_row_stride, int64_t out_plane_stride, float* curve, float* envelope, int64_t curve_row_stride,
               float* min_gain, int* frames, void* stream);

/* ---- remix export: the original with the target removed, ducked or boosted (opt-in; separate_files(target_gain_db=)) ---- */

/* lass_resample_encode (gain NULL) or lass_resample_encode_gain (gain: device, B floats) of a remix: with y that entry point's
 * float32 value before quantisation for frame n and channel c of recording b (the same kernel body, tile plan, tap order and fmaf
 * chain: bit-identical to lass_decode_resample of the plane), the value that is quantised (after fl(gain[b] * v) with a gain) is
 *   v = fl( x + fl( amount[b] * y ) )
 * - two float32 roundings, never an fma - where x is sample n*channels + c of row b of `dry`, decoded by lass_decode_resample's
 * rule: s / 32768 (LASS_WAV_PCM16), (float)s * 2^-31 (LASS_WAV_PCM32, the conversion rounded to nearest), the float itself
 * (LASS_WAV_F32).  dry: device, B rows of at least frames_out interleaved frames of `channels` samples, dry_row_stride_bytes
 * apart, encoding dry_encoding - independent of the output's `encoding`; amount: device, B floats.  The original is read at the
 * file's rate from its own samples, so everything the model did not touch keeps its full band; only y is band-limited.
 * Identities: amount[b] == 0 and a finite y give v == x, hence a PCM16 payload encoded as PCM16 comes back byte for byte, a float32
 * payload comes back equal as values (x + (+0) turns -0.0 into +0.0), and a PCM32 payload comes back as its float32 rounding; an
 * all-zero float32 dry payload with amount[b] == 1 gives lass_resample_encode's values.
 * Limits, checked before anything is launched (LASS_ERR_ARG): lass_resample_encode's, and dry non-NULL and 4-byte aligned,
 * dry_encoding one of the three, dry_row_stride_bytes a multiple of 4 and >= frames_out * channels * bytes per sample, amount
 * non-NULL (and, as gain, 4-byte aligned).  Stateless, no floating-point atomics: a row's bytes are bit-identical alone and as any
 * row of any batch.  Not ported: the reference writes the separated target only. */
int lass_remix_encode(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                      int up, int down, const float* taps, int n_taps, const void* dry, int64_t dry_row_stride_bytes,
                      int dry_encoding, const float* amount, int encoding, const float* gain, void* out_bytes,
                      int64_t out_row_stride_bytes, int frames_out, unsigned* clipped, void* stream);

/* The sample peak of what lass_remix_encode (without a gain) would quantise: peak[b] = max |v| over the channels of recording b and
 * n < frames_out, v as above - lass_resample_peak with the dry source, by the same integer atomic max; a NaN is skipped.
 * Arguments and limits: lass_remix_encode's up to amount, then lass_resample_peak's. */
int lass_remix_peak(lass_ctx* ctx, const float* planes, int64_t row_stride, int64_t plane_stride, int B, int channels, int L_in,
                    int up, int down, const float* taps, int n_taps, const void* dry, int64_t dry_row_stride_bytes, int dry_encoding,
                    const float* amount, int frames_out, float* peak, void* stream);

/* Training-side data path ("next" row f4, mixer half; also the producer stage of the STFT pre-compute,
 * scripts/precompute_stfts.py:352-681): SegmentMixer.__call__ + dynamic_loudnorm (data/waveform_mixers.py:19-92) on the
 * device.  waveforms (B,L) -> mixture (B,L), segment (B,L).  For clip n:
 *   noise = sum_{i=1}^{mix_num[n]-1} 10^(comp_db[n][i-1]/20) * (x_{(n+i)%B} / clamp(sqrt(E_{(n+i)%B} / max(E_n,1e-10)), 0.02, 50));
 *   noise = 10^(noise_db[n]/20) * (noise / clamp(sqrt(E_noise / max(E_n,1e-10)), 0.02, 50));   E = mean(x^2)
 *   mixture = x_n + noise;  if max|mixture| > 1: segment = x_n * 0.9/max, mixture *= 0.9/max, else segment = x_n.
 * The reference draws mix_num = randint(2, max_mix_num) and the dB values = randint(lower_db, higher_db) with Python's
 * `random`; here they are INPUTS (device arrays: mix_num int32 (B), comp_db f32 (B, max_comp), noise_db f32 (B)), so the
 * host decides the draws (lass_amd.waveform_mixers.SegmentMixer draws them in the reference's order).
 * max_comp = max_mix_num - 1 (1 ... 7); scratch: 4*B doubles; the three waveform buffers must be distinct. */
int lass_segment_mix(lass_ctx* ctx, const float* waveforms, int B, int L, const int* mix_num, const float* comp_db, int max_comp,
                     const float* noise_db, float* mixture, float* segment, double* scratch, void* stream);

/* ---- CLAP text encoder (query embeddings) ----------------------------------------------------------------------- */

/* The text tower of the query encoder: caption token ids -> (N,512) L2-normalised float32 embeddings.
 * Replaces: CLAP_Encoder.get_query_embed(modality="text") (models/clap_encoder.py:78-116) = CLAP.get_text_embedding ->
 * encode_text for text_branch_type "roberta" (CLAP/open_clip/model.py:516-531, 658-665, 732-751): RoBERTa-base
 * (hidden 768, 12 heads, FFN 3072, post-LN, LayerNorm eps 1e-5, exact-erf GELU, pad id 1), pooler tanh(Wp h[:,0] + bp),
 * Linear(768,512) -> ReLU -> Linear(512,512), F.normalize.  f32 throughout, contractions on the f32 MFMA.
 * A separate handle: the separator's lass_ctx is untouched.  Same conventions (return codes, caller's stream, no CPU
 * fallback: without a gfx950 device lass_text_create fails). */
typedef struct lass_text_ctx lass_text_ctx;

int lass_text_create(lass_text_ctx** out, int device_id);
int lass_text_destroy(lass_text_ctx* ctx);
/* Last error of this context (or of the failed lass_text_create when ctx == NULL).  Never NULL. */
const char* lass_text_last_error(const lass_text_ctx* ctx);
/* Upload one f32 tensor (host or device pointer), key relative to the CLAP model: "text_branch.embeddings.*",
 * "text_branch.encoder.layer.<i>.*", "text_branch.pooler.dense.*", "text_projection.{0,2}.*" - the checkpoint's
 * `query_encoder.model.<key>`.  Shapes are checked; any other key is LASS_ERR_ARG.  Vocabulary and position-table
 * sizes are taken from the tensors, the layer count from the layer indices present. */
int lass_text_set_param(lass_text_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim);
/* Checks that every parameter of layers 0 .. L-1 and of the embeddings / pooler / projection is present, fuses each
 * layer's query/key/value weights into one (2304,768) matrix.  Must be called again after any lass_text_set_param. */
int lass_text_finalize(lass_text_ctx* ctx);
/* Encoder layers of a finalized context (0 before lass_text_finalize). */
int lass_text_layers(const lass_text_ctx* ctx);
/* Workspace bytes lass_text_encode needs for N captions padded to S tokens (1 <= S <= 512); anything else is LASS_ERR_ARG
 * with its message in lass_text_last_error. */
int lass_text_workspace_bytes(const lass_text_ctx* ctx, int N, int S, size_t* bytes);
/* input_ids (N,S) int64 DEVICE pointer, attention_mask (N,S) int64 HOST pointer (it decides which rows are computed and
 * sizes every launch, so no device-to-host read is needed) -> out (N,512) f32, and pooler_output (N,768) f32 into
 * `pooler_out` unless NULL.  Only positions with attention_mask != 0 are computed (a packed batch of sum-of-lengths
 * rows); position ids still count over the whole id row, so the result equals the padded computation.  attention_mask[:,0]
 * must be nonzero for every caption.  Ids must lie in [0, vocab) - the caller checks; out-of-range ids are clamped.
 * The mask is staged in pinned memory: a call waits for the previous call's (small) upload before it rewrites it. */
int lass_text_encode(lass_text_ctx* ctx, const int64_t* input_ids, const int64_t* attention_mask, int N, int S,
                     float* out, float* pooler_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CLAP audio encoder (query by example) ------------------------------------------------------------------------ */

/* The audio tower of the query encoder: clips -> (B,512) L2-normalised float32 embeddings.
 * Replaces: CLAP_Encoder.get_query_embed(modality="audio") (models/clap_encoder.py:50-76) for amodel "HTSAT-base" without
 * fusion: resample 32 -> 48 kHz (polyphase 3/2 FIR, torchaudio's published defaults), repeat-pad to 480 000 samples,
 * log-mel (n_fft 1024, hop 480, periodic Hann, reflect; 64 slaney bands 50 .. 14000 Hz; 10 log10(max(p, 1e-10))), bn0,
 * bicubic 1001 -> 1024 frames + fold to 256 x 256 + 4x4 patch embedding, the Swin stages (8 x 8 windows, shifted in odd
 * blocks, relative-position bias, pre-LN, exact-erf GELU, PatchMerging), final LayerNorm, token mean ("embedding"),
 * Linear -> ReLU -> Linear(512), F.normalize (CLAP/open_clip/htsat.py:1012-1149, model.py:566-570, 754-781).
 * f32 throughout, contractions on the f32 MFMA.  Row n of the result is what the reference computes for clip n alone.
 * A separate handle with the conventions of lass_text_*: return codes, caller's stream and workspace, no allocation in
 * the encode calls, no CPU fallback (without a gfx950 device lass_audioq_create fails). */
typedef struct lass_audioq_ctx lass_audioq_ctx;

/* Optional device outputs of the encode calls; a NULL member is not written.  wave48k (B, ceil(1.5 L)) is written by
 * lass_audioq_encode_wave32k only; logmel (B,1001,64) is after bn0; tokens (B,4096,128) after the patch embedding's
 * LayerNorm; stage[i] is stage i's output (after its PatchMerging; the last stage's before the final LayerNorm);
 * embedding (B, 128 * 2^(stages-1)) is the token mean. */
typedef struct lass_audioq_taps {
    float* wave48k;
    float* logmel;
    float* tokens;
    float* stage[4];
    float* embedding;
} lass_audioq_taps;

int lass_audioq_create(lass_audioq_ctx** out, int device_id);
int lass_audioq_destroy(lass_audioq_ctx* ctx);
/* Last error of this context (or of the failed lass_audioq_create when ctx == NULL).  Never NULL. */
const char* lass_audioq_last_error(const lass_audioq_ctx* ctx);
/* Upload one f32 tensor (host or device pointer), key relative to the CLAP model: "audio_branch.bn0.{weight,bias,
 * running_mean,running_var}", "audio_branch.patch_embed.*", "audio_branch.layers.<i>.blocks.<j>.*",
 * "audio_branch.layers.<i>.downsample.*", "audio_branch.norm.*", "audio_projection.{0,2}.*" - the checkpoint's
 * `query_encoder.model.<key>`.  Any other key (the classification heads and the derived buffers included) is
 * LASS_ERR_ARG.  Stage and block counts are taken from the indices present. */
int lass_audioq_set_param(lass_audioq_ctx* ctx, const char* name, const void* data, const int64_t* shape, int ndim);
/* Checks presence and shape of every parameter of the stages found (embedding width 128, doubling per stage), folds bn0,
 * builds the resampler taps, window, twiddles, mel filter and bicubic table.  Call again after any lass_audioq_set_param. */
int lass_audioq_finalize(lass_audioq_ctx* ctx);
/* Stages of a finalized context (0 before lass_audioq_finalize). */
int lass_audioq_stages(const lass_audioq_ctx* ctx);
/* Workspace bytes either encode call needs for B clips. */
int lass_audioq_workspace_bytes(const lass_audioq_ctx* ctx, int B, size_t* bytes);
/* wave (B,L) f32 DEVICE pointer at 48 kHz, 1 <= L <= 480 000; lengths (B) int HOST pointer or NULL (every clip L samples):
 * clip n is wave[n][0 .. lengths[n]) -> out (B,512) f32.  All argument checks run before anything is launched. */
int lass_audioq_encode_wave48k(lass_audioq_ctx* ctx, const float* wave, const int* lengths, int B, int L, float* out,
                               const lass_audioq_taps* taps, void* workspace, size_t workspace_bytes, void* stream);
/* The same from 32 kHz input, 1 <= L <= 320 000 (10 s), with the resampler in front. */
int lass_audioq_encode_wave32k(lass_audioq_ctx* ctx, const float* wave, const int* lengths, int B, int L, float* out,
                               const lass_audioq_taps* taps, void* workspace, size_t workspace_bytes, void* stream);

/* ---- instrumentation ---------------------------------------------------------------------------------------- */

/* When enabled, lass_separate brackets each kernel class with HIP events on `stream` (costs a few us per launch).
 * The event pool (512 pairs, ~12 separations) is created HERE, never inside lass_separate; scopes beyond the pool are
 * not timed, so read (lass_profile_get) or reset at least every few separations while profiling. */
int lass_set_profiling(lass_ctx* ctx, int enabled);
/* After a profiled lass_separate has completed (caller synchronised the stream): number of kernel classes, and for
 * class i its name, accumulated milliseconds and launch count since the last lass_profile_reset. */
int lass_profile_count(const lass_ctx* ctx);
int lass_profile_get(lass_ctx* ctx, int i, const char** name, double* ms, int* launches);
int lass_profile_reset(lass_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* LASS_HIP_H */
