// audio_args_table.cpp - what lass_amd/csrc/audio_args.h says to one argument set of an audio file entry point: the refusal's
// message on one line, an empty line for accepted.  The two refusals the header leaves to device-side predicates
// (lass_resample_true_peak_fits, lass_loudness_filter) are not made here.
// Host only: g++ -std=c++17 -Wall -Werror -I lass_amd/csrc tools/audio_args_table.cpp -o tools/bin/audio_args_table
// usage: audio_args_table ENTRY name=value ...
//   ENTRY: lass_decode_resample ... lass_limit; names: the parameters of include/lass_hip.h's declaration (no ctx, no stream), every
//   one of them; pointers as integers (0: NULL), floats as strtod reads them (nan, inf)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "audio_args.h"

namespace {

std::map<std::string, std::string> args;
bool missing = false;

const char* raw(const char* name) {
    auto it = args.find(name);
    if (it == args.end()) {
        fprintf(stderr, "missing %s\n", name);
        missing = true;
        return "0";
    }
    return it->second.c_str();
}
long long I(const char* name) { return strtoll(raw(name), nullptr, 10); }
double F(const char* name) { return strtod(raw(name), nullptr); }
template <class T = void>
const T* P(const char* name) { return reinterpret_cast<const T*>(static_cast<uintptr_t>(strtoull(raw(name), nullptr, 10))); }

PlaneRows planes(const char* L_name) {
    return {P<float>("planes"), I("row_stride"), I("plane_stride"), (int)I("B"), (int)I("channels"), (int)I(L_name)};
}
RationalFilter filter() { return {(int)I("up"), (int)I("down"), P<float>("taps"), (int)I("n_taps")}; }
DrySource dry_source() {
    return {{P("dry"), I("dry_row_stride_bytes"), (int)I("dry_encoding"), (int)I("frames_out"), (int)I("channels")}, P<float>("amount")};
}
Oversampler oversampler() { return {(int)I("os"), P<float>("os_taps"), (int)I("n_os_taps")}; }
PayloadRows out_rows() { return {P("out_bytes"), I("out_row_stride_bytes"), (int)I("encoding"), (int)I("frames_out"), (int)I("channels")}; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s ENTRY name=value ...\n", argv[0]);
        return 2;
    }
    for (int i = 2; i < argc; ++i) {
        const char* eq = strchr(argv[i], '=');
        if (!eq) return 2;
        args[std::string(argv[i], (size_t)(eq - argv[i]))] = eq + 1;
    }
    const std::string e = argv[1], w = e + ": ";
    std::string m;
    if (e == "lass_decode_resample" || e == "lass_decode_resample_planar") {
        m = check_decode(w, {P("raw"), I("row_stride_bytes"), (int)I("encoding"), (int)I("frames"), (int)I("channels")}, (int)I("B"), filter(),
                         P<float>("out"), (int)I("L_out"));
    } else if (e == "lass_resample_encode") {
        m = check_encode(w, planes("L_in"), filter(), nullptr, nullptr, false, out_rows(), P<unsigned>("clipped"));
    } else if (e == "lass_resample_encode_gain") {
        m = check_encode(w, planes("L_in"), filter(), nullptr, P<float>("gain"), true, out_rows(), P<unsigned>("clipped"));
    } else if (e == "lass_remix_encode") {
        const DrySource d = dry_source();
        m = check_encode(w, planes("L_in"), filter(), &d, P<float>("gain"), false, out_rows(), P<unsigned>("clipped"));
    } else if (e == "lass_resample_peak") {
        m = check_peak(w, planes("L_in"), filter(), nullptr, (int)I("frames_out"), nullptr, P<float>("peak"));
    } else if (e == "lass_remix_peak") {
        const DrySource d = dry_source();
        m = check_peak(w, planes("L_in"), filter(), &d, (int)I("frames_out"), nullptr, P<float>("peak"));
    } else if (e == "lass_resample_true_peak") {
        const Oversampler o = oversampler();
        m = check_peak(w, planes("L_in"), filter(), nullptr, (int)I("frames_out"), &o, P<float>("peak"));
    } else if (e == "lass_loudness" || e == "lass_loudness_stats") {
        const bool stats = e == "lass_loudness_stats";
        m = check_meter(w, planes("L"), P<int>("lengths"), (int)I("hop"), P<double>("coef"), P<float>("weights"), P<double>("out"),
                        P<double>("blocks"), (int)I("nb_max"), stats ? P<double>("short_term") : nullptr, stats ? (int)I("ns_max") : 0,
                        P("scratch"), (size_t)I("scratch_bytes"), stats);
    } else if (e == "lass_loudness_gain") {
        m = check_gain_rule(w, P<double>("loudness"), P<float>("peak"), (int)I("B"), F("target_lufs"), (float)F("ceiling"), P<float>("gain"),
                            P<int>("limited"));
    } else if (e == "lass_limit") {
        const PlaneRows p = planes("L");
        m = check_limit(w, p, oversampler(), P<float>("gain"), (float)F("ceiling"), (int)I("H"), P<float>("window"),
                        {P<float>("out"), I("out_row_stride"), I("out_plane_stride"), p.B, p.ch, p.L}, P<float>("curve"), P<float>("envelope"),
                        I("curve_row_stride"), P<float>("min_gain"), P<int>("frames"));
    } else {
        fprintf(stderr, "unknown entry %s\n", argv[1]);
        return 2;
    }
    if (missing) return 2;
    puts(m.c_str());
    return 0;
}
