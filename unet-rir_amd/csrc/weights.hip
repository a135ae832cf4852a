// weights.hip - layout changes of the weight tensors (gfx950): the fp32 transpose [N][T][C] -> [C][T][N] and the bf16 work copies
// of the fp32 masters (same orientation with channel pad, transposed, and conv3x3d's packed order), one layer or all layers of a
// model per launch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "mfma_types.h"

// [N][T][C] -> [C][T][N] through a 32x33 LDS tile per tap
__global__ void transpose_weight_kernel(const float* __restrict__ w, float* __restrict__ wt, int N, int T, int C) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: 8 rows per pass
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, c = c0 + tx;
        tile[r][tx] = (n < N && c < C) ? w[((size_t)n * T + t) * C + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, n = n0 + tx;
        if (n < N && c < C) wt[((size_t)c * T + t) * N + n] = tile[tx][r];
    }
}

// ------------------------------------------------------------------------------------------------
// weight work copies: fp32 master [N][T][C] -> bf16 [N][T][Cp] (same orientation, channel pad) and bf16 [C][T][Np]
// ------------------------------------------------------------------------------------------------
__global__ void cast_weight_kernel(const float* __restrict__ w, __bf16* __restrict__ o, int N, int T, int C, int Cp) {
    const size_t total = (size_t)N * T * Cp;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % Cp);
        const size_t nt = i / Cp;
        o[i] = (c < C) ? (__bf16)w[nt * C + c] : (__bf16)0.f;
    }
}

__global__ void transpose_cast_weight_kernel(const float* __restrict__ w, __bf16* __restrict__ wt, int N, int T, int C, int Np) {
    __shared__ float tile[32][33];
    const int t = blockIdx.z;
    const int c0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int n = n0 + r, c = c0 + tx;
        tile[r][tx] = (n < N && c < C) ? w[((size_t)n * T + t) * C + c] : 0.f;
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int c = c0 + r, n = n0 + tx;
        if (n < Np && c < C) wt[((size_t)c * T + t) * Np + n] = (__bf16)tile[tx][r];
    }
}

// All layers of a model in two launches: desc[l] describes one fp32 master [N][T][C] and its two bf16 work copies
// (blockIdx.y = layer).  Same element order as cast_weight_kernel / transpose_cast_weight_kernel.
// layers the fused kernel below takes: both copies wanted, no channel padding, 64 x 64 tiles fit exactly
__device__ __forceinline__ bool cast_fused_applies(const unetrir_cast_desc& d) {
    return d.same && d.transposed && d.C == d.Cp && d.N == d.Np && (d.C & 63) == 0 && (d.N & 63) == 0 &&
           ((((uintptr_t)d.w) & 15) | (((uintptr_t)d.same) & 7) | (((uintptr_t)d.transposed) & 7)) == 0;
}

// Both work copies from ONE read of the master: a 64 (n) x 64 (c) tile of tap t is loaded with 16-byte accesses, rounded,
// stored as it lies ([N][T][C]) and, through a padded LDS tile, transposed ([C][T][N]); every global store row is 128 bytes.
__global__ __launch_bounds__(256) void cast_both_batched_kernel(const unetrir_cast_desc* __restrict__ desc) {
    __shared__ __bf16 tile[64][66];                       // 132-byte rows: the column gathers below hit 16 banks
    const unetrir_cast_desc d = desc[blockIdx.y];
    if (!cast_fused_applies(d)) return;
    __bf16* __restrict__ same = (__bf16*)d.same;
    __bf16* __restrict__ wt = (__bf16*)d.transposed;
    __bf16* __restrict__ pk = d.T == 9 ? (__bf16*)d.packed_s2 : nullptr;      // third copy in conv3x3d's DMA order (include/unetrir.h)
    const int ntx = d.C >> 6, nty = d.N >> 6;
    const int ntiles = ntx * nty * d.T;
    const int lr = threadIdx.x >> 4, lc = (threadIdx.x & 15) * 4;
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int t = tl / (ntx * nty);
        const int rem = tl - t * (ntx * nty);
        const int c0 = (rem % ntx) << 6, n0 = (rem / ntx) << 6;
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int r = ps * 16 + lr;
            const size_t off = ((size_t)(n0 + r) * d.T + t) * d.C + c0 + lc;
            const float4 v = *reinterpret_cast<const float4*>(d.w + off);
            bf16x4 h;
            h[0] = (__bf16)v.x; h[1] = (__bf16)v.y; h[2] = (__bf16)v.z; h[3] = (__bf16)v.w;
            *reinterpret_cast<bf16x4*>(same + off) = h;
            if (pk) {
                const int n = n0 + r, c = c0 + lc;
                const int m = n & 31, rho = (m & 16) | ((m & 8) >> 1) | ((m & 4) << 1) | (m & 3);       // row of the MFMA block that holds channel m
                const size_t po = ((((size_t)(n >> 7) * (d.C >> 4) + (c >> 4)) * 36 + t * 4 + ((n >> 5) & 3)) * 64 + rho + 32 * ((c >> 3) & 1)) * 8 + (c & 7);
                *reinterpret_cast<bf16x4*>(pk + po) = h;
            }
            tile[r][lc + 0] = h[0]; tile[r][lc + 1] = h[1]; tile[r][lc + 2] = h[2]; tile[r][lc + 3] = h[3];
        }
        __syncthreads();
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
            const int c = ps * 16 + lr;
            bf16x4 h;
            h[0] = tile[lc + 0][c]; h[1] = tile[lc + 1][c]; h[2] = tile[lc + 2][c]; h[3] = tile[lc + 3][c];
            *reinterpret_cast<bf16x4*>(wt + ((size_t)(c0 + c) * d.T + t) * d.N + n0 + lc) = h;
        }
    }
}

__global__ __launch_bounds__(256) void cast_weights_batched_kernel(const unetrir_cast_desc* __restrict__ desc) {
    const unetrir_cast_desc d = desc[blockIdx.y];
    if (cast_fused_applies(d)) return;
    if (d.packed_s2 && d.T == 9 && (d.C & 15) == 0) {     // packed copy for conv3x3d where the fused kernel does not run (with or without `same`)
        __bf16* pk = (__bf16*)d.packed_s2;
        const size_t tot = (size_t)d.N * 9 * d.C;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < tot; i += (size_t)gridDim.x * 256) {
            const int c = (int)(i % d.C);
            const size_t nt_ = i / d.C;
            const int t = (int)(nt_ % 9), n = (int)(nt_ / 9);
            const int m = n & 31, rho = (m & 16) | ((m & 8) >> 1) | ((m & 4) << 1) | (m & 3);
            const size_t po = ((((size_t)(n >> 7) * (d.C >> 4) + (c >> 4)) * 36 + t * 4 + ((n >> 5) & 3)) * 64 + rho + 32 * ((c >> 3) & 1)) * 8 + (c & 7);
            pk[po] = (__bf16)d.w[i];
        }
    }
    if (!d.same) return;
    __bf16* o = (__bf16*)d.same;
    const size_t total = (size_t)d.N * d.T * d.Cp;
    if (d.C == d.Cp && (total & 7) == 0 && (((uintptr_t)d.w | (uintptr_t)o) & 15) == 0) {     // flat copy, 8 elements per thread
        const size_t n8 = total >> 3;
        for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
            const float4 a = *reinterpret_cast<const float4*>(d.w + i * 8), b = *reinterpret_cast<const float4*>(d.w + i * 8 + 4);
            bf16x8 v;
            v[0] = (__bf16)a.x; v[1] = (__bf16)a.y; v[2] = (__bf16)a.z; v[3] = (__bf16)a.w;
            v[4] = (__bf16)b.x; v[5] = (__bf16)b.y; v[6] = (__bf16)b.z; v[7] = (__bf16)b.w;
            *reinterpret_cast<bf16x8*>(o + i * 8) = v;
        }
        return;
    }
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % d.Cp);
        const size_t nt = i / d.Cp;
        o[i] = (c < d.C) ? (__bf16)d.w[nt * d.C + c] : (__bf16)0.f;
    }
}

__global__ __launch_bounds__(256) void transpose_cast_weights_batched_kernel(const unetrir_cast_desc* __restrict__ desc) {
    __shared__ float tile[32][33];
    const unetrir_cast_desc d = desc[blockIdx.y];
    if (!d.transposed || cast_fused_applies(d)) return;
    __bf16* wt = (__bf16*)d.transposed;
    const int ntx = (d.C + 31) / 32, nty = (d.Np + 31) / 32;
    const int ntiles = ntx * nty * d.T;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int tl = blockIdx.x; tl < ntiles; tl += gridDim.x) {
        const int t = tl / (ntx * nty);
        const int rem = tl - t * (ntx * nty);
        const int c0 = (rem % ntx) * 32, n0 = (rem / ntx) * 32;
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int n = n0 + r, c = c0 + tx;
            tile[r][tx] = (n < d.N && c < d.C) ? d.w[((size_t)n * d.T + t) * d.C + c] : 0.f;
        }
        __syncthreads();
        for (int r = ty; r < 32; r += 8) {
            const int c = c0 + r, n = n0 + tx;
            if (n < d.Np && c < d.C) wt[((size_t)c * d.T + t) * d.Np + n] = (__bf16)tile[tx][r];
        }
    }
}

int launch_transpose_weight(const float* w, float* wt, int N, int T, int C, hipStream_t s) {
    dim3 grid((C + 31) / 32, (N + 31) / 32, T);
    hipLaunchKernelGGL(transpose_weight_kernel, grid, dim3(256), 0, s, w, wt, N, T, C);
    return (int)hipGetLastError();
}

int launch_cast_weight(const float* w, void* o, int N, int T, int C, int Cp, hipStream_t s) {
    const size_t total = (size_t)N * T * Cp;
    unsigned nb = (unsigned)((total + 255) / 256);
    if (nb > 8192) nb = 8192;
    hipLaunchKernelGGL(cast_weight_kernel, dim3(nb), dim3(256), 0, s, w, (__bf16*)o, N, T, C, Cp);
    return (int)hipGetLastError();
}

int launch_transpose_cast_weight(const float* w, void* wt, int N, int T, int C, int Np, hipStream_t s) {
    dim3 grid((C + 31) / 32, (Np + 31) / 32, T);
    hipLaunchKernelGGL(transpose_cast_weight_kernel, grid, dim3(256), 0, s, w, (__bf16*)wt, N, T, C, Np);
    return (int)hipGetLastError();
}

int launch_cast_weights_batched(const unetrir_cast_desc* desc_dev, int n_layers, hipStream_t s) {
    hipLaunchKernelGGL(cast_both_batched_kernel, dim3(256, n_layers), dim3(256), 0, s, desc_dev);
    hipLaunchKernelGGL(cast_weights_batched_kernel, dim3(256, n_layers), dim3(256), 0, s, desc_dev);
    hipLaunchKernelGGL(transpose_cast_weights_batched_kernel, dim3(256, n_layers), dim3(256), 0, s, desc_dev);
    return (int)hipGetLastError();
}
