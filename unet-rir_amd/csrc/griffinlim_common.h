// griffinlim_common.h - what the two forms of the Griffin-Lim reconstruction (griffinlim.hip, fp64 DFTs; griffinlim_fft.hip, fp32 FFTs in
// LDS) must agree on to the bit: the denormalisation constants, librosa's envelope threshold, the counter-based uniform draw of the
// initial phases (the recipe of include/unetrir.h, unetrir_uniform_f32) and the reading of the momentum.
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include "kernels.h"

constexpr double GL_MD = 100.0;               // Normalizer.md (preprocess.py:23)
constexpr double GL_EP = 1e-5;                // 10^(-md/20)    (preprocess.py:24)
constexpr double GL_REF = 128.0;              // amp / 128      (preprocess.py:27)
constexpr double GL_TINY32 = 1.1754943508222875e-38;   // numpy.finfo(float32).tiny: librosa's envelope threshold

#define GL_GOLD64 0x9E3779B97F4A7C15ULL
// "UNIFRM64": separates the phase key from the keys dropout_mask_kernel and normal_kernel derive from the same (seed, step)
#define GL_UNIFORM_TAG 0x554E4946524D3634ULL

// Element i of draw (seed, step) - the recipe of include/unetrir.h (unetrir_uniform_f32)
__device__ __forceinline__ unsigned long long gl_uniform_key(unsigned long long seed, unsigned long long step) {
    return mix64(mix64(seed * GL_GOLD64 + step) ^ GL_UNIFORM_TAG);
}
__device__ __forceinline__ float gl_uniform_at(unsigned long long key, long long i) {
    const unsigned long long r = mix64(key + GL_GOLD64 * (unsigned long long)(i + 1));
    return (float)(unsigned)(r >> 40) * (1.0f / 16777216.0f);          // top 24 bits -> [0, 1)
}

// The ABI carries momentum as a float, but librosa's is a double and 32 iterations carry the 2.4e-9 between 0.99f and 0.99 into
// the waveform at 1e-8...3e-7 of its peak.  The argument is therefore read as the shortest decimal that rounds to the float given
// (0.99f -> 0.99, as numpy prints a float32): the number the caller wrote.
inline double gl_decimal(float v) {
    char buf[40];
    for (int p = 1; p <= 9; ++p) {
        snprintf(buf, sizeof buf, "%.*e", p - 1, (double)v);
        const double d = strtod(buf, nullptr);
        if ((float)d == v) return d;
    }
    return (double)v;
}
