// mfma_types.h - vector types, per-element-type constants and the 32x32 MFMA step shared by the kernels of csrc/ (register-staged
// and LDS-DMA alike).  Internal to csrc/; include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// One 128-byte row of K per LDS stage: KE elements, EPS of them per 16-byte lane slot (Vec: the type a lane loads
// them as).
template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int KE = 32, EPS = 4;
    typedef float4 Vec;
    static __device__ __forceinline__ Vec zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
};
template <> struct Elem<__bf16> {
    static constexpr int KE = 64, EPS = 8;
    typedef uint4 Vec;
    static __device__ __forceinline__ Vec zero() { return make_uint4(0u, 0u, 0u, 0u); }
};

// acc += A . B over the K values of one 16-byte fragment pair.  fp32: four v_mfma_f32_32x32x2_f32 (rows = a, columns = b).
__device__ __forceinline__ void mma4(f32x16& acc, const uint4& a, const uint4& b, float) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}
// bf16: the weight fragment is the A operand, so the accumulator comes out TRANSPOSED (rows/registers = output channel,
// columns/lanes = pixel): a lane then owns 4 consecutive channels per register quad, which pack into 8-byte LDS writes
// for the staged epilogue (2-byte global stores straight from the MFMA layout cost 35-40 % of the kernel).
__device__ __forceinline__ void mma4(f32x16& acc, const uint4& a, const uint4& b, __bf16) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, b), __builtin_bit_cast(bf16x8, a), acc, 0, 0, 0);
}

// two fp32 values rounded to bf16 (nearest even) in one 32-bit word, and the halves of such a word as fp32 (pw1x1.hip, conv2x2.hip:
// the register epilogues that store 16 consecutive channels of a pixel)
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const __bf16 x = (__bf16)a, y = (__bf16)b;
    return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
__device__ __forceinline__ float lo16(unsigned v) { return __builtin_bit_cast(float, v << 16); }
__device__ __forceinline__ float hi16(unsigned v) { return __builtin_bit_cast(float, v & 0xffff0000u); }
