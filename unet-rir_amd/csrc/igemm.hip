// igemm.hip - implicit-GEMM convolution kernels for gfx950 (MI355X), fp32 MFMA.
//
// One forward-type kernel covers Conv2D (stride 1|2), Conv2DTranspose (as 4 output-parity
// sub-convolutions) and every data gradient; one weight-gradient kernel covers every dW.
// Both are driven by a small tap table (TF padding='same' geometry is resolved on the host
// in api.hip), replace what TensorFlow dispatches to cuDNN for dl_models/u_net.py:269-276,
// :297-304, :366, :248, :262 and their tape.gradient counterparts (main_training.py:267).
//
// Math: v_mfma_f32_32x32x2_f32 (exact fp32 fma chain, 64 FLOP/clk/SIMD).  A = activations
// (rows = pixels), B = weights (cols = output channels), so the accumulator has the output
// channel on the lane and the NHWC store is 128 contiguous bytes per (row, half-wave).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "igemm_tile.h"

#define BM 128          // pixels per tile
#define BK 32           // k (tap, channel) values per LDS stage
#define LDS_LD 36       // padded row length (floats): 9 x 16 B, odd -> conflict-free ds_read_b128

// ------------------------------------------------------------------------------------------------
// forward-type kernel:  out[opix(p)][n] = bias[n] + addend + sum_t sum_c in[ipix(p,t)][c] * w[n][widx_t][c]
// ------------------------------------------------------------------------------------------------
template <int BN_, bool UNIFORM>
__global__ __launch_bounds__(256) void igemm_fwd_kernel(const IgemmArgs a) {
    constexpr int NSUB = BN_ / 64;        // 32-wide N sub-tiles per wave (waves are 2 x 2)
    constexpr int NB = BN_ / 32;          // B-tile rows loaded per thread
    __shared__ __attribute__((aligned(16))) float As[BM * LDS_LD];
    __shared__ __attribute__((aligned(16))) float Bs[BN_ * LDS_LD];
    __shared__ uint32_t s_tap[UNETRIR_MAX_TAPS];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    if (tid < UNETRIR_MAX_TAPS) s_tap[tid] = a.g.tap[tid];

    const int ntN = (a.g.N + BN_ - 1) / BN_;
    const int nwg = gridDim.x;
    const int id = xcd_remap(blockIdx.x, nwg);
    const int mt = id / ntN, nt = id - mt * ntN;
    const long long M = (long long)a.g.B * a.g.PH * a.g.PW;
    const long long m0 = (long long)mt * BM;
    const int n0 = nt * BN_;

    const int C = a.g.C, ntaps = a.g.ntaps;
    const int IH = a.g.IH, IW = a.g.IW, ldi = a.g.ldi;
    const int ldw = a.g.wtaps * C;
    const int Ktot = ntaps * C;
    int nch = (Ktot + BK - 1) / BK;
    int ch0 = 0;
    if (a.ksplit > 1) {      // split-K (small pixel counts, e.g. the Dense layer): this block owns chunks [ch0, nch)
        const int per = (nch + a.ksplit - 1) / a.ksplit;
        ch0 = blockIdx.y * per;
        nch = min(nch, ch0 + per);
    }

    // loader mapping: 8 threads cover the 32 k-values of one row; 32 rows per pass
    const int quad = tid & 7, lrow = tid >> 3;
    // (tap, channel) of the k-quad being staged.  UNIFORM (C % 32 == 0): a stage never straddles a tap, so the
    // tap index and the channel base are wave-uniform scalars and only quad*4 is per lane.
    int kt = (ch0 * BK + (UNIFORM ? 0 : quad * 4)) / C;
    int kc = (ch0 * BK + (UNIFORM ? 0 : quad * 4)) % C;

    __syncthreads();   // s_tap visible

    const int plane = a.g.PH * a.g.PW;
    IGEMM_ROW_PROLOGUE(float, 4, NB, long long)

    float4 ra[4], rb[NB];
    auto load_stage = [&]() { IGEMM_LOAD_STAGE(float, 4, NB, ra, rb) };

    f32x16 acc[2][NSUB];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NSUB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    load_stage();
    const int arow = wm * 64 + (lane & 31), brow = wn * (BN_ / 2) + (lane & 31);
    const int koff = (lane >> 5) * 4;

    for (int ch = ch0; ch < nch; ++ch) {
        if (ch != ch0) __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&As[(lrow + 32 * j) * LDS_LD + quad * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < NB; ++j) *reinterpret_cast<float4*>(&Bs[(lrow + 32 * j) * LDS_LD + quad * 4]) = rb[j];
        __syncthreads();
        if (ch + 1 < nch) {
            kc += BK;
            while (kc >= C) { kc -= C; ++kt; }
            load_stage();
        }
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            float4 fa[2], fb[NSUB];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const float4*>(&As[(arow + 32 * i) * LDS_LD + kk * 8 + koff]);
#pragma unroll
            for (int j = 0; j < NSUB; ++j) fb[j] = *reinterpret_cast<const float4*>(&Bs[(brow + 32 * j) * LDS_LD + kk * 8 + koff]);
            // k-major order: consecutive MFMAs hit different accumulators (dependent latency == issue interval)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].x, fb[j].x, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].y, fb[j].y, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].z, fb[j].z, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NSUB; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i].w, fb[j].w, acc[i][j], 0, 0, 0);
        }
    }

    if (a.ksplit > 1) {      // raw partial sums; bias / reduction happen in splitk_rows_reduce_kernel
        float* part = a.part + (size_t)blockIdx.y * M * a.g.N;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const long long p = m0 + wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (p >= M) continue;
#pragma unroll
                for (int j = 0; j < NSUB; ++j) {
                    const int n = n0 + wn * (BN_ / 2) + 32 * j + (lane & 31);
                    if (n < a.g.N) part[p * a.g.N + n] = acc[i][j][r];
                }
            }
        return;
    }
    // ---- epilogue: accumulator (col = lane&31 -> n, row = (r&3)+8*(r>>2)+4*(lane>>5) -> pixel)
    const bool simple = (a.g.SO == 1 && a.g.ooy == 0 && a.g.oox == 0 && a.g.OH == a.g.PH && a.g.OW == a.g.PW);
    float bias[NSUB];
    int ncol[NSUB];
#pragma unroll
    for (int j = 0; j < NSUB; ++j) {
        ncol[j] = n0 + wn * (BN_ / 2) + 32 * j + (lane & 31);
        bias[j] = (a.bias != nullptr && ncol[j] < a.g.N) ? a.bias[ncol[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = wm * 64 + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
            const long long p = m0 + row;
            if (p >= M) continue;
            long long opix;
            if (simple) {
                opix = p;
            } else {
                const int n = (int)(p / plane);
                const int rem = (int)(p - (long long)n * plane);
                const int py = rem / a.g.PW, px = rem - py * a.g.PW;
                const int oy = py * a.g.SO + a.g.ooy, ox = px * a.g.SO + a.g.oox;
                if (oy >= a.g.OH || ox >= a.g.OW) continue;
                opix = ((long long)n * a.g.OH + oy) * a.g.OW + ox;
            }
#pragma unroll
            for (int j = 0; j < NSUB; ++j) {
                if (ncol[j] < a.g.N) {
                    float v = acc[i][j][r] + bias[j];
                    if (a.addend != nullptr) v += a.addend[opix * a.ldadd + ncol[j]];
                    a.out[opix * a.g.ldo + ncol[j]] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// weight-gradient kernel: part[s][n][widx_t*C + c] = sum_{p in slice s} dy[p][n] * x[ipix(p,t)][c]
// GEMM rows = output channels n, cols = flattened (tap, channel), K = pixels (split over blockIdx.y)
// ------------------------------------------------------------------------------------------------
#define WG_COLS 128
#define WG_PIX 32
#define WG_LDX (WG_COLS + 4)

// operand loads in the storage type of the activations: fp32, or bf16 widened on the way in (the k x k weight gradients of bf16
// graphs that have no bf16 kernel of their own - kernels = 6, the reference's constructor default, dl_models/u_net.py:40-45 - run
// here: fp32 MFMA arithmetic on exactly the stored values)
template <typename T> __device__ __forceinline__ float4 wg_ld4(const void* base, size_t elem_off);
template <> __device__ __forceinline__ float4 wg_ld4<float>(const void* base, size_t elem_off) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(base) + elem_off);
}
template <> __device__ __forceinline__ float4 wg_ld4<__bf16>(const void* base, size_t elem_off) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const __bf16*>(base) + elem_off);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}

template <int BR_, typename T = float>   // rows (output channels) per tile: 64 or 128
__global__ __launch_bounds__(256) void igemm_wgrad_kernel(const WgradArgs a) {
    constexpr int MSUB = BR_ / 64;        // BR_=128: waves 2x2 of 64x64; BR_=64: waves 2x2 of 32x64
    constexpr int LDD = BR_ + 4;
    constexpr int DQ = BR_ / 4;           // dy quads per pixel row
    constexpr int DPASS = (WG_PIX * DQ) / 256;
    constexpr int DROWS = 256 / DQ;
    __shared__ __attribute__((aligned(16))) float Ds[WG_PIX * LDD];
    __shared__ __attribute__((aligned(16))) float Xs[WG_PIX * WG_LDX];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;

    const int C = a.g.C;
    const int Kc = a.g.ntaps * C;                 // valid columns
    const int ntC = (Kc + WG_COLS - 1) / WG_COLS;
    const int id = blockIdx.x;
    const int rt = id / ntC, ct = id - rt * ntC;  // column tile fastest: shares the dy panel in L2
    const int n0 = rt * BR_, j0 = ct * WG_COLS;
    const long long M = (long long)a.g.B * a.g.PH * a.g.PW;
    const long long chunk_per = a.chunks_per_split;
    const long long pk0 = (long long)blockIdx.y * chunk_per * WG_PIX;
    long long pk1 = pk0 + chunk_per * WG_PIX;
    if (pk1 > M) pk1 = M;

    // X loader: this thread always loads the same 4 columns -> fixed (tap, channel)
    const int xq = tid & 31, xr = tid >> 5;      // 32 quads per row, 8 rows per pass
    const int col = j0 + xq * 4;
    const bool colok = col < Kc;
    const int t = colok ? col / C : 0, c = colok ? col - (col / C) * C : 0;
    const uint32_t e = a.g.tap[t];
    const int dy = (int)(int8_t)(e & 0xff), dx = (int)(int8_t)((e >> 8) & 0xff);
    const int plane = a.g.PH * a.g.PW;
    const int IH = a.g.IH, IW = a.g.IW, SI = a.g.SI;

    const int dq = tid % DQ, dr = tid / DQ;
    const bool nok = (n0 + dq * 4) < a.g.N;

    float4 rx[4], rd[DPASS];
    auto load_stage = [&](long long pk) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long long p = pk + xr + 8 * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (colok && p < pk1) {
                const int n = (int)(p / plane);
                const int rem = (int)(p - (long long)n * plane);
                const int py = rem / a.g.PW, px = rem - py * a.g.PW;
                const int iy = py * SI + dy, ix = px * SI + dx;
                if ((unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW)
                    v = wg_ld4<T>(a.x, ((size_t)((long long)n * IH + iy) * IW + ix) * a.g.ldi + c);
            }
            rx[j] = v;
        }
#pragma unroll
        for (int j = 0; j < DPASS; ++j) {
            const long long p = pk + dr + DROWS * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nok && p < pk1) v = wg_ld4<T>(a.dy, (size_t)p * a.lddy + n0 + dq * 4);
            rd[j] = v;
        }
    };

    f32x16 acc[MSUB][2];
#pragma unroll
    for (int i = 0; i < MSUB; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int arow = wm * (BR_ / 2) + (lane & 31);   // output-channel row inside the tile
    const int bcol = wn * 64 + (lane & 31);
    const int kh = lane >> 5;

    if (pk0 < pk1) load_stage(pk0);
    for (long long pk = pk0; pk < pk1; pk += WG_PIX) {
        if (pk != pk0) __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(&Xs[(xr + 8 * j) * WG_LDX + xq * 4]) = rx[j];
#pragma unroll
        for (int j = 0; j < DPASS; ++j) *reinterpret_cast<float4*>(&Ds[(dr + DROWS * j) * LDD + dq * 4]) = rd[j];
        __syncthreads();
        if (pk + WG_PIX < pk1) load_stage(pk + WG_PIX);
#pragma unroll
        for (int s = 0; s < WG_PIX / 2; ++s) {
            float fa[MSUB], fb[2];
#pragma unroll
            for (int i = 0; i < MSUB; ++i) fa[i] = Ds[(2 * s + kh) * LDD + arow + 32 * i];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = Xs[(2 * s + kh) * WG_LDX + bcol + 32 * j];
#pragma unroll
            for (int i = 0; i < MSUB; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
    }

    // ---- epilogue: rows (registers) = output channel, cols (lanes) = flattened (tap, channel)
    float* part = a.part + (size_t)blockIdx.y * a.g.N * ((size_t)a.g.wtaps * C);
    const size_t ldp = (size_t)a.g.wtaps * C;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int cc = j0 + wn * 64 + 32 * j + (lane & 31);
        if (cc >= Kc) continue;
        const int tt = cc / C, c2 = cc - tt * C;
        const size_t ocol = (size_t)((a.g.tap[tt] >> 16) & 0xff) * C + c2;
#pragma unroll
        for (int i = 0; i < MSUB; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wm * (BR_ / 2) + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < a.g.N) part[(size_t)n * ldp + ocol] = acc[i][j][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
int launch_igemm_fwd(const IgemmArgs& a, hipStream_t s) {
    const long long M = (long long)a.g.B * a.g.PH * a.g.PW;
    if (M <= 0 || a.g.N <= 0) return 0;
    const long long mt = (M + BM - 1) / BM;
    const bool uniform = (a.g.C % BK) == 0;
    const unsigned ks = a.ksplit > 1 ? (unsigned)a.ksplit : 1u;
    if (a.g.N > 64) {
        const long long nwg = mt * ((a.g.N + 127) / 128);
        if (uniform) hipLaunchKernelGGL((igemm_fwd_kernel<128, true>), dim3((unsigned)nwg, ks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((igemm_fwd_kernel<128, false>), dim3((unsigned)nwg, ks), dim3(256), 0, s, a);
    } else {
        if (uniform) hipLaunchKernelGGL((igemm_fwd_kernel<64, true>), dim3((unsigned)mt, ks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((igemm_fwd_kernel<64, false>), dim3((unsigned)mt, ks), dim3(256), 0, s, a);
    }
    return (int)hipGetLastError();
}

int wgrad_plan(const IgemmGeom& g, int* nsplit, long long* chunks_per_split) {
    const long long M = (long long)g.B * g.PH * g.PW;
    const long long nchunks = (M + WG_PIX - 1) / WG_PIX;
    const int br = g.N > 64 ? 128 : 64;
    const long long tiles = (long long)((g.N + br - 1) / br) * ((g.ntaps * g.C + WG_COLS - 1) / WG_COLS);
    long long want = (1024 + tiles - 1) / tiles;          // aim at >= 1024 workgroups
    long long maxs = (nchunks + 7) / 8;                   // at least 8 chunks (256 pixels) per slice
    if (maxs < 1) maxs = 1;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    long long per = (nchunks + want - 1) / want;
    long long ns = (nchunks + per - 1) / per;
    *nsplit = (int)ns;
    *chunks_per_split = per;
    return 0;
}

int launch_igemm_wgrad(const WgradArgs& a, int nsplit, hipStream_t s, int bf16_operands) {
    const int br = a.g.N > 64 ? 128 : 64;
    const unsigned tiles = (unsigned)(((a.g.N + br - 1) / br) * ((a.g.ntaps * a.g.C + WG_COLS - 1) / WG_COLS));
    if (bf16_operands) {      // a.x / a.dy point at bf16 tensors
        if (br == 128) hipLaunchKernelGGL((igemm_wgrad_kernel<128, __bf16>), dim3(tiles, nsplit), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((igemm_wgrad_kernel<64, __bf16>), dim3(tiles, nsplit), dim3(256), 0, s, a);
    } else if (br == 128) hipLaunchKernelGGL(igemm_wgrad_kernel<128>, dim3(tiles, nsplit), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(igemm_wgrad_kernel<64>, dim3(tiles, nsplit), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
