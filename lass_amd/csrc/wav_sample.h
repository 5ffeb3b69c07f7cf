// wav_sample.h - one sample of a WAV payload row as a float32, shared by inclusion by resample.hip (the decode) and export.hip
// (the dry source of a remix), so that both read a payload by one rule.  Include inside an anonymous namespace, after lass_hip.h.
#pragma once

// Sample idx (frame-major, interleaved) of the row as read_wav makes it: x/32768 (PCM16), round-to-nearest int -> float then
// * 2^-31 (PCM32: equal to read_wav's float64 division rounded once, the scaling being exact), the float itself (float32).
__device__ __forceinline__ float sample_at(const unsigned char* __restrict__ row, long long idx, int enc) {
    if (enc == LASS_WAV_PCM16) return (float)reinterpret_cast<const short*>(row)[idx] * (1.0f / 32768.0f);
    if (enc == LASS_WAV_PCM32) return __int2float_rn(reinterpret_cast<const int*>(row)[idx]) * (1.0f / 2147483648.0f);
    return reinterpret_cast<const float*>(row)[idx];
}
