// lds_dma.h - device-only primitives shared by the LDS-DMA kernels (conv3x3g/p/h/r/s/d, upconv3x3g/q, wgrad3x3g/d, stem3x3,
// head_mfma): global memory -> LDS by buffer_load ... lds, fragments out of LDS by inline-asm reads with counted waits, MFMA.
// Internal to csrc/; include after <hip/hip_runtime.h>.
#pragma once
#include <stdint.h>
#include "mfma_types.h"

typedef __attribute__((address_space(3))) void* lptr_t;

// Fragment reads are inline asm so that the compiler does not drain the DMA queue in front of them: it waits vmcnt(0) before
// any LDS load it can see while an LDS-DMA is outstanding.  They return in issue order; LGKM_WAIT(n) lets the youngest n stay
// in flight and pins the instructions around it.
#define DSR128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define TRR(dst, addr, off) asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define LGKM_WAIT(n) do { asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define MMA16(accv, wfrag, pfrag) \
    accv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wfrag), __builtin_bit_cast(bf16x8, pfrag), accv, 0, 0, 0)
#define MMA(accv, wfrag, pfrag) \
    accv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wfrag), __builtin_bit_cast(bf16x8, pfrag), accv, 0, 0, 0)

// An epilogue staging tile is private to a wave: LDS operations of one wave execute in issue order, so its reads see its
// own earlier writes without a workgroup barrier; this only stops the compiler from moving LDS accesses across the point.
#define WAVE_LDS_FENCE() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_wave_barrier(); } while (0)

// A lane that must read zeros (halo outside the image, channels past N) carries this byte offset: past num_records of every
// resource below (the *_applies rules keep them under 0x70000000), so the load returns zeros and a store goes nowhere.
constexpr uint32_t OOB = 0xF0000000u;

// raw buffer resource over `bytes` bytes at `p`: stride 0, bounds-checked against num_records, 32-bit data format
#define raw_rsrc(p, bytes) __builtin_amdgcn_make_buffer_rsrc((void*)(p), (short)0, (bytes), 0x00020000)

// sum over the 16 lanes of a DPP row, every lane gets the total: the xor-butterfly order (1, 2, 4, 8) on single vector
// instructions (quad permutes, then the mirrored half / whole row: after two steps the lanes of a quad hold the same value)
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ float row_sum16(float v) {
    v = dpp_add<0xB1>(v);      // quad_perm [1,0,3,2]
    v = dpp_add<0x4E>(v);      // quad_perm [2,3,0,1]
    v = dpp_add<0x141>(v);     // row_half_mirror
    return dpp_add<0x140>(v);  // row_mirror
}
