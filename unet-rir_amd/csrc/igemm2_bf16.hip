// igemm2_bf16.hip - the tap-table implicit-GEMM forward kernel for SMALL problems (gfx950, bf16 storage, fp32 accumulate).
//
// igemm_bf16.hip serves every layer no patch-staged kernel takes: small grids (the reference's own 36 x 40 / 18 x 20 / 9 x 10
// levels, main_training.py:27), 6 x 6 kernels (the constructor default, dl_models/u_net.py:40-45), stride-2 layers at 16 x 16.  Its
// 128 x 128 tiles with ONE K chunk in flight suit large grids; on a 36 x 40 level there are 360 workgroups for 256 CUs, each
// alone on its CU, and every one of its 18 K chunks pays a full global-memory round trip: 46 us for 13.6 GFLOP (0.3 PFLOP/s).
// Same arithmetic here (v_mfma_f32_32x32x16_bf16 over the same K order: identical bits), re-shaped for few pixels:
//   * 64-pixel tiles (BM = 64) when 128-pixel tiles would not even give every CU one workgroup: four times the workgroups, 37 KB
//     of LDS each, so three to four share a CU and cover each other's memory latency;
//   * TWO K chunks in flight per workgroup: the registers of chunk c + 1 go to the second LDS buffer while chunk c is computed,
//     and are re-loaded for chunk c + 3 at once - one barrier per chunk instead of two, loads issued two chunks ahead;
//   * 32-bit pixel arithmetic in the prologue (the 64-bit divisions of the general kernel cost ~1 us of a 10 us launch);
//   * the same epilogue: bias, optional addend, 16-byte stores through an LDS staging tile, fused column statistics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "igemm_tile.h"

#define BKH 64
#define LDH 72

namespace {

template <int BM_, int BN_, bool UNIFORM>
__device__ __forceinline__ void igemm2_body(const IgemmArgsH& a, const int block_id, const int n_blocks) {
    constexpr int MI = BM_ / 64;                          // 32-pixel blocks per wave (waves 2 x 2: BM_/2 pixels x BN_/2 channels each)
    constexpr int NSUB = BN_ / 64;
    constexpr int NA = BM_ / 32, NB = BN_ / 32;           // loader passes (32 rows per pass)
    constexpr int STAGE = (BM_ + BN_) * LDH;
    __shared__ __attribute__((aligned(16))) __bf16 smem_h[2 * STAGE];     // two (A tile, B tile) buffers; reused by the epilogue
    __shared__ uint32_t s_tap[UNETRIR_MAX_TAPS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    if (tid < UNETRIR_MAX_TAPS) s_tap[tid] = a.g.tap[tid];

    const int ntN = (a.g.N + BN_ - 1) / BN_;
    const int id = xcd_remap(block_id, n_blocks);
    const int mt = id / ntN, nt = id - mt * ntN;
    const unsigned plane = (unsigned)a.g.PH * (unsigned)a.g.PW;
    const unsigned M = (unsigned)a.g.B * plane;           // < 2^31 (checked by the launcher)
    const unsigned m0 = (unsigned)mt * BM_;
    const int n0 = nt * BN_;

    const int C = a.g.C, ntaps = a.g.ntaps;
    const int IH = a.g.IH, IW = a.g.IW, ldi = a.g.ldi;
    const int ldw = a.g.wtaps * C;
    const int nch = (ntaps * C + BKH - 1) / BKH;

    const int quad = tid & 7, lrow = tid >> 3;            // 8 threads x 8 bf16 = one 64-wide row; 32 rows per pass
    int kt = UNIFORM ? 0 : (quad * 8) / C;
    int kc = UNIFORM ? 0 : (quad * 8) % C;
    __syncthreads();

    IGEMM_ROW_PROLOGUE(__bf16, NA, NB, unsigned)

    uint4 ra[2][NA], rb[2][NB];
    // loads the NEXT chunk in K order (chunks are requested strictly in order 0, 1, 2, ...) into register set `set`
    auto load_stage = [&](auto set_c) {
        constexpr int set = decltype(set_c)::value;
        IGEMM_LOAD_STAGE(__bf16, NA, NB, ra[set], rb[set])
        kc += BKH;
        while (kc >= C) { kc -= C; ++kt; }
    };
    auto to_lds = [&](auto set_c, auto buf_c) {
        constexpr int set = decltype(set_c)::value, buf = decltype(buf_c)::value;
        __bf16* As = smem_h + buf * STAGE;
        __bf16* Bs = As + BM_ * LDH;
#pragma unroll
        for (int j = 0; j < NA; ++j) *reinterpret_cast<uint4*>(&As[(lrow + 32 * j) * LDH + quad * 8]) = ra[set][j];
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<uint4*>(&Bs[(lrow + 32 * j) * LDH + quad * 8]) = rb[set][j];
    };

    f32x16 acc[MI][NSUB];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NSUB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int arow = wm * (BM_ / 2) + (lane & 31), brow = wn * (BN_ / 2) + (lane & 31);
    const int koff = (lane >> 5) * 8;

    // prologue: chunks 0 and 1 requested; chunk 0 into LDS buffer 0, its registers re-loaded for chunk 2
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    load_stage(I0{});
    if (nch > 1) load_stage(I1{});
    to_lds(I0{}, I0{});
    if (nch > 2) load_stage(I0{});
    __syncthreads();
    // one K chunk; CUR (compile time: the register sets must not be indexed at run time) = parity of the chunk = its LDS buffer
    auto step = [&](int ch, auto cur_c) {
        constexpr int CUR = decltype(cur_c)::value;
        if (ch + 1 < nch) {                               // chunk ch + 1: registers -> the other buffer; then its registers take chunk ch + 3
            to_lds(std::integral_constant<int, CUR ^ 1>{}, std::integral_constant<int, CUR ^ 1>{});
            if (ch + 3 < nch) load_stage(std::integral_constant<int, CUR ^ 1>{});
        }
        const __bf16* As = smem_h + CUR * STAGE;
        const __bf16* Bs = As + BM_ * LDH;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            bf16x8 fa[MI], fb[NSUB];
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(&As[(arow + 32 * i) * LDH + kk * 16 + koff]);
#pragma unroll
            for (int j = 0; j < NSUB; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(&Bs[(brow + 32 * j) * LDH + kk * 16 + koff]);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
        __syncthreads();                                  // buffer CUR^1 is complete, buffer CUR is free
    };
    for (int ch = 0; ch < nch; ch += 2) {
        step(ch, std::integral_constant<int, 0>{});
        if (ch + 1 < nch) step(ch + 1, std::integral_constant<int, 1>{});
    }

    IGEMM_BF16_EPILOGUE((BM_ / 2), BN_, unsigned)          // step() ended with a barrier
}

template <int BM_, int BN_, bool UNIFORM>
__global__ __launch_bounds__(256) void igemm2_fwd_bf16_kernel(const IgemmArgsH a) {
    igemm2_body<BM_, BN_, UNIFORM>(a, blockIdx.x, gridDim.x);
}

template <int BM_, int BN_, bool UNIFORM>
__global__ __launch_bounds__(256) void igemm2_fwd_bf16_kernel4(const IgemmArgsH4 a4) {
    igemm2_body<BM_, BN_, UNIFORM>(a4.a[blockIdx.y], blockIdx.x, gridDim.x);
}

struct SmallKernels {
    template <int BN_, bool UNIFORM> static constexpr auto k1 = igemm2_fwd_bf16_kernel<64, BN_, UNIFORM>;
    template <int BN_, bool UNIFORM> static constexpr auto k4 = igemm2_fwd_bf16_kernel4<64, BN_, UNIFORM>;
};

}  // namespace

// Pixel-tile height of the tap-table launch for an iteration grid of M pixels and N output channels, ncls launches sharing the
// grid; 0 = the general kernel (igemm_bf16.hip, 128-pixel tiles).  Measured at batch 32 (scripts/micro_igemm.py, round 3): below
// one 128 x 128 workgroup per CU the 64-pixel tiles win (256 -> 256 @ 18 x 20: 47 -> 38 us, 512 -> 512 @ 9 x 10: 79 -> 51,
// 256 -> 512 stride 2 @ 18 x 20: 44 -> 27); from 360 workgroups on (36 x 40 levels, 16 x 16 with 1024 channels) the general
// kernel's five resident workgroups per CU beat two chunks in flight (35 against 46 us).
int igemm_bf16_tile_m(long long M, int N, int ncls) {
    if (!unetrir_cfg().igemm2 || M <= 0 || M >= (1ll << 31)) return 0;
    const long long wg128 = ((M + 127) / 128) * ((N + 127) / 128) * ncls;
    return wg128 < 256 ? 64 : 0;
}

// a[0 .. ncls): 1 launch or the 4 output-parity classes of a stride-2 transposed layer (same shape, one grid).
// Only for problems for which igemm_bf16_tile_m returned 64 (launch_igemm_fwd_bf16 asks first): 64-pixel tiles, M < 2^31.
int launch_igemm2_fwd_bf16(const IgemmArgsH* a, int ncls, hipStream_t s) {
    const long long M = (long long)a[0].g.B * a[0].g.PH * a[0].g.PW;
    if (M <= 0 || a[0].g.N <= 0) return 0;
    const long long mt = (M + 63) / 64;
    // channel tile: 128 when N > 64 and the 64-pixel x 128-channel tiles still fill the chip twice, else 64
    const bool bn128 = a[0].g.N > 64 && mt * ((a[0].g.N + 127) / 128) * ncls >= 2 * 256;
    const unsigned nwg = (unsigned)(mt * (bn128 ? (a[0].g.N + 127) / 128 : (a[0].g.N + 63) / 64));
    return launch_tap_table_bf16<SmallKernels>(a, ncls, bn128, nwg, s);
}
