// audio_args.h - the operands of the audio file entry points (lass_decode_resample ... lass_limit, api.hip) as values, and what
// those entries ask of them: each rule ONCE, each entry's checks as one ordered list.  A check returns the refusal's message, ""
// for accepted; the entry turns a message into LASS_ERR_ARG (api.hip, refuse).  A rule is parameterised by what differs between
// the entries and nothing else: the entry's "name: " (w), the operand's name in the message, the name of the length, and whether
// B or B * channels is what the launch grid bounds.  Two refusals read device-side constants and stay with them, made by the entry
// after its list here: lass_resample_true_peak_fits (export.hip's LDS plan) and lass_loudness_filter (loudness.hip).
// The launchers (kernels.h) take the same structs.  Host only and free of HIP, as conv_route.h.  tools/audio_args_table.cpp
// prints a check's message; tests/test_audio_args_cpu.py holds every message to tests/golden/audio_refusals.json, recorded from
// the entries as they were before this header existed.
#pragma once
#include <cmath>
#include <cstdint>
#include <initializer_list>
#include <string>

#include "../../include/lass_hip.h"

// B recordings x ch planes of L floats; strides in floats
struct PlaneRows {
    const float* p;
    long long row_stride, plane_stride;
    int B, ch, L;
};
// y[n] = sum_m x[m] * taps[n*down - m*up + (n_taps-1)/2]; up == down == 1: no filter, taps unused
struct RationalFilter {
    int up, down;
    const float* taps;
    int n_taps;
};
// rows of `frames` interleaved frames of ch samples, enc = LASS_WAV_*, row_stride_bytes apart: the decoder's raw, the encoders'
// out_bytes (written: the one const_cast is the encode launcher's), the remix's dry
struct PayloadRows {
    const void* p;
    long long row_stride_bytes;
    int enc, frames, ch;
};
// v = fl(x + fl(amount[b] * y)), x from rows
struct DrySource {
    PayloadRows rows;
    const float* amount;
};
// polyphase.h's chain at (os, 1): 20 * os + 1 taps
struct Oversampler {
    int os;
    const float* taps;
    int n_taps;
};

// the polyphase table in LDS, in floats
inline size_t lass_resample_table_floats(int up, int n_taps) { return (size_t)up * (size_t)(((n_taps + up - 1) / up) | 1); }
inline long long resampled_frames(long long frames, int up, int down) { return (frames * up + down - 1) / down; }
inline long long payload_row_bytes(const PayloadRows& r) { return (long long)r.frames * r.ch * (r.enc == LASS_WAV_PCM16 ? 2 : 4); }
inline long long plane_row_floats(const PlaneRows& P) { return (long long)(P.ch - 1) * P.plane_stride + P.L; }
inline bool misaligned(std::initializer_list<const void*> ps, uintptr_t n) {
    for (const void* p : ps)
        if (reinterpret_cast<uintptr_t>(p) % n != 0) return true;
    return false;
}

// ---- the rules ----------------------------------------------------------------------------------------------------------------
// the first line of an entry: its required pointers, B (capped where B is a grid dimension), the length where it is named here
inline std::string check_operands(const std::string& w, const char* names, bool present, int B, bool cap_B, const char* L_name, int L) {
    if (present && B >= 1 && (!cap_B || B <= 65535) && (!L_name || L >= 1)) return "";
    return w + names + " non-NULL, " + (cap_B ? "1 <= B <= 65535" : "B >= 1") + (L_name ? std::string(", ") + L_name + " >= 1" : "");
}

// planes_in_grid: B * channels is the grid dimension, not B
inline std::string check_channels(const std::string& w, int ch, int B, bool planes_in_grid) {
    if (ch >= 1 && ch <= 8 && (!planes_in_grid || (long long)B * ch <= 65535)) return "";
    return w + "1 ... 8 channels" + (planes_in_grid ? ", B * channels <= 65535" : "");
}

inline std::string check_encoding(const std::string& w, const char* name, int enc) {
    if (enc == LASS_WAV_PCM16 || enc == LASS_WAV_PCM32 || enc == LASS_WAV_F32) return "";
    return w + name + " must be LASS_WAV_PCM16, LASS_WAV_PCM32 or LASS_WAV_F32";
}

// lass_decode_resample's limits on encoding, channels, the ratio and the filter
inline std::string check_resample(const std::string& w, int enc, int ch, const RationalFilter& F) {
    std::string m = check_encoding(w, "encoding", enc);
    if (m.empty()) m = check_channels(w, ch, 0, false);
    if (!m.empty()) return m;
    if (F.up < 1 || F.down < 1 || F.up > LASS_RESAMPLE_MAX_RATIO || F.down > LASS_RESAMPLE_MAX_RATIO)
        return w + "up and down must lie in 1 ... " + std::to_string(LASS_RESAMPLE_MAX_RATIO);
    if (F.up == 1 && F.down == 1) return "";
    if (!F.taps || F.n_taps < 1 || F.n_taps % 2 == 0) return w + "taps non-NULL, n_taps odd";
    if (F.n_taps > LASS_RESAMPLE_MAX_TAPS)
        return w + std::to_string(F.n_taps) + " taps exceed the cap of " + std::to_string(LASS_RESAMPLE_MAX_TAPS) +
               " (resample on the host)";
    if (lass_resample_table_floats(F.up, F.n_taps) > LASS_RESAMPLE_MAX_TABLE)
        return w + "the polyphase table up * (ceil(n_taps/up) | 1) exceeds " + std::to_string(LASS_RESAMPLE_MAX_TABLE) + " floats";
    return "";
}

inline std::string check_frames_out(const std::string& w, const PlaneRows& P, const RationalFilter& F, int frames_out) {
    const long long ceiling = resampled_frames(P.L, F.up, F.down);
    if (frames_out >= 1 && (long long)frames_out <= ceiling) return "";
    return w + "frames_out must lie in 1 ... ceil(L_in*up/down) = " + std::to_string(ceiling);
}

// pre: "" for the planes, "out_" for lass_limit's output
inline std::string check_plane_layout(const std::string& w, const char* pre, const PlaneRows& P) {
    if (P.plane_stride >= P.L && P.row_stride >= plane_row_floats(P)) return "";
    return w + pre + "plane_stride must hold a plane (" + std::to_string(P.L) + " floats) and " + pre + "row_stride a recording (" +
           std::to_string(plane_row_floats(P)) + " floats)";
}

// stride: the stride's name; holds: what a row is called ("a row", "frames_out frames")
inline std::string check_payload_rows(const std::string& w, const char* stride, const char* holds, const PayloadRows& r) {
    if (r.row_stride_bytes >= payload_row_bytes(r) && r.row_stride_bytes % 4 == 0) return "";
    return w + stride + " must be a multiple of 4 and hold " + holds + " (" + std::to_string(payload_row_bytes(r)) + " bytes)";
}

inline std::string check_aligned4(const std::string& w, const char* names, std::initializer_list<const void*> ps) {
    return misaligned(ps, 4) ? w + names + " must be 4-byte aligned" : "";
}

// the dry source of the two remix entries (rows.frames: frames_out)
inline std::string check_dry(const std::string& w, const DrySource& d) {
    if (!d.rows.p || !d.amount) return w + "dry and amount non-NULL";
    std::string m = check_encoding(w, "dry_encoding", d.rows.enc);
    if (m.empty()) m = check_payload_rows(w, "dry_row_stride_bytes", "frames_out frames", d.rows);
    if (m.empty()) m = check_aligned4(w, "dry and amount", {d.rows.p, d.amount});
    return m;
}

// with_one: os == 1 (no oversampling: taps NULL and 0, or the 21 of a (1, 1) chain) is the entry's to take (lass_limit)
inline std::string check_oversampler(const std::string& w, const Oversampler& o, bool with_one) {
    if (o.os != 2 && o.os != 4 && !(with_one && o.os == 1))
        return w + (with_one ? "os must be 1, 2 or 4" : "os must be 2 or 4 (1 is lass_resample_peak)");
    const std::string want = std::to_string(20 * o.os + 1);
    if (o.os == 1 ? (o.taps ? o.n_taps != 21 : o.n_taps != 0) : (!o.taps || o.n_taps != 20 * o.os + 1))
        return with_one ? w + "os_taps non-NULL with n_os_taps = 20 * os + 1 = " + want + " (or NULL and 0 at os == 1)"
                        : w + "os_taps non-NULL, n_os_taps = 20 * os + 1 = " + want;
    return "";
}

// ---- the entries, each in its order of checks ------------------------------------------------------------------------------------
// lass_decode_resample, lass_decode_resample_planar
inline std::string check_decode(const std::string& w, const PayloadRows& raw, int B, const RationalFilter& F, const float* out, int L_out) {
    std::string m = check_operands(w, "raw, out", raw.p && out, B, true, "frames", raw.frames);
    if (m.empty()) m = check_resample(w, raw.enc, raw.ch, F);
    if (m.empty() && (L_out <= 0 || resampled_frames(raw.frames, F.up, F.down) != (long long)L_out))
        m = w + "L_out must be ceil(frames*up/down) = " + std::to_string(resampled_frames(raw.frames, F.up, F.down));
    if (m.empty()) m = check_payload_rows(w, "row_stride_bytes", "a row", raw);
    if (m.empty()) m = check_aligned4(w, "raw", {raw.p});
    return m;
}

// lass_resample_encode, lass_resample_encode_gain (gain_required), lass_remix_encode (dry; gain optional).  out.frames: frames_out
inline std::string check_encode(const std::string& w, const PlaneRows& P, const RationalFilter& F, const DrySource* dry, const float* gain,
                                bool gain_required, const PayloadRows& out, const unsigned* clipped) {
    if (gain_required && (!gain || misaligned({gain}, 4))) return w + "gain non-NULL, 4-byte aligned";
    std::string m = check_operands(w, "planes, out_bytes", P.p && out.p, P.B, true, "L_in", P.L);
    if (m.empty()) m = check_resample(w, out.enc, P.ch, F);
    if (m.empty()) m = check_frames_out(w, P, F, out.frames);
    if (m.empty()) m = check_plane_layout(w, "", P);
    if (m.empty() && dry) m = check_dry(w, *dry);
    if (m.empty()) m = check_payload_rows(w, "out_row_stride_bytes", "a row", out);
    if (m.empty()) m = check_aligned4(w, "out_bytes", {out.p});
    if (m.empty())
        m = dry ? check_aligned4(w, "planes, gain and clipped", {P.p, gain, clipped})
                : check_aligned4(w, "planes and clipped", {P.p, clipped});
    return m;
}

// lass_resample_peak, lass_remix_peak (dry), lass_resample_true_peak (os; lass_resample_true_peak_fits is the entry's, after this)
inline std::string check_peak(const std::string& w, const PlaneRows& P, const RationalFilter& F, const DrySource* dry, int frames_out,
                              const Oversampler* os, const float* peak) {
    std::string m = check_operands(w, "planes, peak", P.p && peak, P.B, true, "L_in", P.L);
    if (m.empty()) m = check_resample(w, LASS_WAV_F32, P.ch, F);
    if (m.empty()) m = check_frames_out(w, P, F, frames_out);
    if (m.empty()) m = check_plane_layout(w, "", P);
    if (m.empty() && dry) m = check_dry(w, *dry);
    if (m.empty() && os) m = check_oversampler(w, *os, false);
    if (m.empty())
        m = os ? check_aligned4(w, "planes, os_taps and peak", {P.p, os->taps, peak})
               : check_aligned4(w, "planes and peak", {P.p, peak});
    return m;
}

// lass_loudness, lass_loudness_stats (stats: one more double of scratch per recording and hop bin, and the short-term blocks);
// lass_loudness_filter's refusal of coef is the entry's, after this
inline std::string check_meter(const std::string& w, const PlaneRows& P, const int* lengths, int hop, const double* coef,
                               const float* weights, const double* out, const double* blocks, int nb_max, const double* short_term,
                               int ns_max, const void* scratch, size_t scratch_bytes, bool stats) {
    std::string m = check_operands(w, "planes, coef, out", P.p && coef && out, P.B, false, "L", P.L);
    if (m.empty()) m = check_channels(w, P.ch, P.B, true);
    if (m.empty() && (hop < 1 || hop > LASS_LOUDNESS_MAX_HOP))
        m = w + "hop (rate / 10) must lie in 1 ... " + std::to_string(LASS_LOUDNESS_MAX_HOP);
    if (m.empty()) m = check_plane_layout(w, "", P);
    if (!m.empty()) return m;
    const long long bins = P.L / hop, nb = bins >= 4 ? bins - 3 : 0, ns = bins >= 30 ? bins - 29 : 0;
    if (blocks && (long long)nb_max < nb) return w + "nb_max must hold the blocks of L samples (" + std::to_string(nb) + ")";
    const size_t need = ((size_t)5 * P.B * P.ch + (stats ? (size_t)P.B : 0)) * bins * sizeof(double);
    if (need && (!scratch || scratch_bytes < need))
        return w + "scratch must hold " + (stats ? "(5 * channels + 1) * B" : "5 * B * channels") + " * (L / hop) doubles (" +
               std::to_string(need) + " bytes)";
    if (misaligned({P.p, lengths, weights}, 4) || misaligned({out, blocks, scratch}, 8))
        return w + "planes, lengths, weights 4-byte aligned; out, blocks, scratch 8-byte aligned";
    if (stats && short_term && ((long long)ns_max < ns || misaligned({short_term}, 8)))
        return w + "short_term 8-byte aligned, ns_max must hold the short-term blocks of L samples (" + std::to_string(ns) + ")";
    return "";
}

// lass_loudness_gain
inline std::string check_gain_rule(const std::string& w, const double* loudness, const float* peak, int B, double target_lufs,
                                   float ceiling, const float* gain, const int* limited) {
    std::string m = check_operands(w, "loudness, gain", loudness && gain, B, false, nullptr, 0);
    if (!m.empty()) return m;
    if (!(ceiling >= 0.0f) || std::isinf(ceiling)) return w + "ceiling must be finite and >= 0 (0: none)";
    if (ceiling > 0.0f && !peak) return w + "a ceiling needs peak";
    if (std::isinf(target_lufs)) return w + "target_lufs must be finite, or NaN for none";
    if (misaligned({loudness}, 8) || misaligned({peak, gain, limited}, 4))
        return w + "loudness 8-byte aligned; peak, gain, limited 4-byte aligned";
    return "";
}

// lass_limit (out: the output planes, of P's B, ch and L)
inline std::string check_limit(const std::string& w, const PlaneRows& P, const Oversampler& os, const float* gain, float ceiling, int H,
                               const float* window, const PlaneRows& out, const float* curve, const float* envelope,
                               long long curve_row_stride, const float* min_gain, const int* frames) {
    std::string m = check_operands(w, "planes, gain, window, out", P.p && gain && window && out.p, P.B, true, nullptr, 0);
    if (m.empty()) m = check_channels(w, P.ch, P.B, false);
    if (m.empty() && P.L < 1) m = w + "L >= 1";
    if (m.empty() && (H < 1 || H > LASS_LIMITER_MAX_H)) m = w + "H must lie in 1 ... " + std::to_string(LASS_LIMITER_MAX_H);
    if (m.empty()) m = check_oversampler(w, os, true);
    if (m.empty() && (!(ceiling > 0.0f) || std::isinf(ceiling))) m = w + "ceiling must be finite and > 0";
    if (m.empty()) m = check_plane_layout(w, "", P);
    if (m.empty()) m = check_plane_layout(w, "out_", out);
    if (m.empty() && (curve || envelope) && curve_row_stride < P.L)
        m = w + "curve_row_stride must hold a row (" + std::to_string(P.L) + " floats)";
    if (!m.empty()) return m;
    auto end = [](const PlaneRows& R) {
        return reinterpret_cast<uintptr_t>(R.p) +
               ((uintptr_t)(R.B - 1) * (uintptr_t)R.row_stride + (uintptr_t)plane_row_floats(R)) * sizeof(float);
    };
    if (reinterpret_cast<uintptr_t>(P.p) < end(out) && reinterpret_cast<uintptr_t>(out.p) < end(P))
        return w + "out must not overlap planes (a tile's halo reads what a neighbour would write)";
    return check_aligned4(w, "planes, os_taps, gain, window, out, curve, envelope, min_gain and frames",
                          {P.p, os.taps, gain, window, out.p, curve, envelope, min_gain, frames});
}
