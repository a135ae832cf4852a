// igemm_bf16.hip - bf16-storage / fp32-accumulate variant of the implicit-GEMM forward-type kernel (gfx950).
//
// Same tap-table formulation as igemm.hip; activations and the weight work copies are bf16, accumulation is fp32 in
// v_mfma_f32_32x32x16_bf16 (16x the fp32 MFMA rate), bias / BatchNorm parameters stay fp32.
// A = activations [pixel][k], B = weights [n][k], both K-contiguous -> one ds_read_b128 per operand per MFMA (lane l holds
// k = 8*(l>>5) .. +7 of row l&31).  Prologue, stage loader and epilogue are igemm_tile.h's, shared with igemm2_bf16.hip (the
// same kernel for small problems); the K loop - one chunk in flight, one LDS buffer - is this file's own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "igemm_tile.h"

#define BM 128
#define BKH 64            // bf16 k-values per LDS stage (128 B per row, as the fp32 kernel)
#define LDH 72            // padded row length in bf16 elements (144 B = 9 x 16 B)

// ------------------------------------------------------------------------------------------------
// forward-type kernel (Conv2D fwd, Conv2DTranspose fwd, every data gradient)
// ------------------------------------------------------------------------------------------------
template <int BN_, bool UNIFORM>
__device__ __forceinline__ void igemm_fwd_bf16_body(const IgemmArgsH& a, const int block_id, const int n_blocks) {
    constexpr int NSUB = BN_ / 64;
    constexpr int NB = BN_ / 32;
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[(BM + BN_) * LDH];     // A tile, B tile; reused by the epilogue
    __bf16* As = smem_h;
    __bf16* Bs = smem_h + BM * LDH;
    __shared__ uint32_t s_tap[UNETRIR_MAX_TAPS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    if (tid < UNETRIR_MAX_TAPS) s_tap[tid] = a.g.tap[tid];

    const int ntN = (a.g.N + BN_ - 1) / BN_;
    const int id = xcd_remap(block_id, n_blocks);
    const int mt = id / ntN, nt = id - mt * ntN;
    const long long M = (long long)a.g.B * a.g.PH * a.g.PW;
    const long long m0 = (long long)mt * BM;
    const int n0 = nt * BN_;

    const int C = a.g.C, ntaps = a.g.ntaps;
    const int IH = a.g.IH, IW = a.g.IW, ldi = a.g.ldi;
    const int ldw = a.g.wtaps * C;
    const int nch = (ntaps * C + BKH - 1) / BKH;

    const int quad = tid & 7, lrow = tid >> 3;          // 8 threads x 8 bf16 = one 64-wide row; 32 rows per pass
    int kt = UNIFORM ? 0 : (quad * 8) / C;
    int kc = UNIFORM ? 0 : (quad * 8) % C;
    __syncthreads();

    const int plane = a.g.PH * a.g.PW;
    IGEMM_ROW_PROLOGUE(__bf16, 4, NB, long long)

    uint4 ra[4], rb[NB];
    auto load_stage = [&]() { IGEMM_LOAD_STAGE(__bf16, 4, NB, ra, rb) };

    f32x16 acc[2][NSUB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NSUB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_stage();
    const int arow = wm * 64 + (lane & 31), brow = wn * (BN_ / 2) + (lane & 31);
    const int koff = (lane >> 5) * 8;

    for (int ch = 0; ch < nch; ++ch) {
        if (ch) __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<uint4*>(&As[(lrow + 32 * j) * LDH + quad * 8]) = ra[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<uint4*>(&Bs[(lrow + 32 * j) * LDH + quad * 8]) = rb[j];
        __syncthreads();
        if (ch + 1 < nch) {
            kc += BKH;
            while (kc >= C) { kc -= C; ++kt; }
            load_stage();
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8 fa[2], fb[NSUB];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(&As[(arow + 32 * i) * LDH + kk * 16 + koff]);
#pragma unroll
            for (int j = 0; j < NSUB; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(&Bs[(brow + 32 * j) * LDH + kk * 16 + koff]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
    }
    __syncthreads();      // every wave is done with the A/B tiles: the epilogue stages through the same LDS

    IGEMM_BF16_EPILOGUE(64, BN_, long long)
}

template <int BN_, bool UNIFORM>
__global__ __launch_bounds__(256) void igemm_fwd_bf16_kernel(const IgemmArgsH a) {
    igemm_fwd_bf16_body<BN_, UNIFORM>(a, blockIdx.x, gridDim.x);
}

// four launches of the same shape in one grid (blockIdx.y): the output-parity classes of a stride-2 transposed conv
template <int BN_, bool UNIFORM>
__global__ __launch_bounds__(256) void igemm_fwd_bf16_kernel4(const IgemmArgsH4 a4) {
    igemm_fwd_bf16_body<BN_, UNIFORM>(a4.a[blockIdx.y], blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
namespace {
struct GeneralKernels {
    template <int BN_, bool UNIFORM> static constexpr auto k1 = igemm_fwd_bf16_kernel<BN_, UNIFORM>;
    template <int BN_, bool UNIFORM> static constexpr auto k4 = igemm_fwd_bf16_kernel4<BN_, UNIFORM>;
};

// a[0 .. ncls): 1 launch or the 4 output-parity classes of a stride-2 transposed layer
int launch_general(const IgemmArgsH* a, int ncls, hipStream_t s) {
    const long long M = (long long)a[0].g.B * a[0].g.PH * a[0].g.PW;
    if (M <= 0 || a[0].g.N <= 0) return 0;
    if (igemm_bf16_tile_m(M, a[0].g.N, ncls)) return launch_igemm2_fwd_bf16(a, ncls, s);       // small problems: igemm2_bf16.hip
    const long long mt = (M + BM - 1) / BM;
    const bool bn128 = a[0].g.N > 64;
    return launch_tap_table_bf16<GeneralKernels>(a, ncls, bn128, (unsigned)(bn128 ? mt * ((a[0].g.N + 127) / 128) : mt), s);
}
}  // namespace

int launch_igemm_fwd_bf16(const IgemmArgsH& a, hipStream_t s) { return launch_general(&a, 1, s); }
int launch_igemm_fwd_bf16_x4(const IgemmArgsH* a, hipStream_t s) { return launch_general(a, 4, s); }
