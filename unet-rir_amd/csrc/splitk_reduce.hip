// splitk_reduce.hip - fixed-order reductions of split-K partial slabs (gfx950): the weight-gradient slabs (narrow, wide and
// several reductions in one launch) and the row slabs of the Dense kernels.  No atomics: every output is summed in one order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

// out[i] = sum_s part[s][i] + reg * w[i].  Block = 64 float4 outputs (one full wave: 1 KB contiguous per load) x G split
// groups (waves): group g sums slabs g, g+G, ... in order with 8 independent loads in flight, then the G group sums are
// added in fixed order -> bit-reproducible.  G follows the split count so that no wave idles when there are few slabs.
template <int G>
__device__ __forceinline__ void splitk_reduce_body(float4 (*red)[64], const unsigned block, const float* __restrict__ part, int nsplit, size_t n,
                                                   float* __restrict__ out, float reg, const float* __restrict__ w) {
    const int lane = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const bool busy = grp < G;                     // the batched kernel runs 8 waves whatever G is: the others only meet the barrier
    const size_t i4 = ((size_t)block * 64 + lane) * 4;
    const bool full = i4 + 3 < n;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (busy && full) {
        const float* p = part + i4;
        int k = grp;
        for (; k + 7 * G < nsplit; k += 8 * G) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(k + u * G) * n);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        for (; k < nsplit; k += G) {
            const float4 v = *reinterpret_cast<const float4*>(p + (size_t)k * n);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    } else if (busy && i4 < n) {
        float* sp = &s.x;
        for (int k = grp; k < nsplit; k += G)
            for (size_t i = i4; i < n; ++i) sp[i - i4] += part[(size_t)k * n + i];
    }
    if (G > 1) {
        if (busy) red[grp][lane] = s;
        __syncthreads();
        if (grp != 0) return;
#pragma unroll
        for (int g = 1; g < G; ++g) {
            const float4 v = red[g][lane];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    if (!busy || i4 >= n) return;
    if (full) {
        if (reg != 0.f) {
            const float4 v = *reinterpret_cast<const float4*>(w + i4);
            s.x += reg * v.x; s.y += reg * v.y; s.z += reg * v.z; s.w += reg * v.w;
        }
        *reinterpret_cast<float4*>(out + i4) = s;
    } else {
        const float* sp = &s.x;
        for (size_t i = i4; i < n; ++i) out[i] = sp[i - i4] + (reg != 0.f ? reg * w[i] : 0.f);
    }
}
template <int G>
__global__ __launch_bounds__(64 * G) void splitk_reduce_kernel(const float* __restrict__ part, int nsplit, size_t n,
                                                               float* __restrict__ out, float reg, const float* __restrict__ w) {
    __shared__ float4 red[G][64];
    splitk_reduce_body<G>(red, blockIdx.x, part, nsplit, n, out, reg, w);
}

// y[p][n] = bias[n] + sum_s part[s][p][n]   (fixed order)
__global__ void splitk_rows_reduce_kernel(const float* __restrict__ part, int nsplit, long long M, int N,
                                          const float* __restrict__ bias, float* __restrict__ y, int ldy) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * N) return;
    const long long p = i / N;
    const int n = (int)(i - p * N);
    float s = bias ? bias[n] : 0.f;
    const size_t mn = (size_t)M * N;
    int k = 0;
    for (; k + 7 < nsplit; k += 8) {             // 8 independent loads in flight, added in slab order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(k + u) * mn + i];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; k < nsplit; ++k) s += part[(size_t)k * mn + i];
    y[p * ldy + n] = s;
}

int launch_splitk_rows_reduce(const float* part, int nsplit, long long M, int N, const float* bias, float* y, int ldy, hipStream_t s) {
    const long long tot = M * N;
    hipLaunchKernelGGL(splitk_rows_reduce_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, part, nsplit, M, N, bias, y, ldy);
    return (int)hipGetLastError();
}

// Few outputs, many slabs (the 1x1 and small 3x3 weight gradients of the residual graphs: 1 K .. 64 K floats from up to 512
// slabs): the kernel above would run a handful of workgroups that each walk 64 slabs one after the other.  Here a workgroup
// owns 16 float4 columns and 32 slab groups: group g sums slabs g, g + 32, ... (8 loads in flight), the 32 group sums are added
// in a fixed order.  16 lanes x 16 bytes = one 256-byte piece of a slab per group and step.
__device__ __forceinline__ void splitk_reduce_wide_body(float4 (*red)[16], const unsigned block, const float* __restrict__ part, int nsplit, size_t n,
                                                        float* __restrict__ out, float reg, const float* __restrict__ w) {
    const int lane = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const size_t i4 = ((size_t)block * 16 + lane) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i4 < n) {                                   // n % 4 == 0 (checked by the launcher)
        const float* p = part + i4;
        int k = grp;
        for (; k + 7 * 32 < nsplit; k += 8 * 32) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(k + u * 32) * n);
#pragma unroll
            for (int u = 0; u < 8; ++u) { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
        for (; k < nsplit; k += 32) {
            const float4 v = *reinterpret_cast<const float4*>(p + (size_t)k * n);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[grp][lane] = s;
    __syncthreads();
    if (grp != 0 || i4 >= n) return;
#pragma unroll
    for (int g = 1; g < 32; ++g) {
        const float4 v = red[g][lane];
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    if (reg != 0.f) {
        const float4 v = *reinterpret_cast<const float4*>(w + i4);
        s.x += reg * v.x; s.y += reg * v.y; s.z += reg * v.z; s.w += reg * v.w;
    }
    *reinterpret_cast<float4*>(out + i4) = s;
}
__global__ __launch_bounds__(512) void splitk_reduce_wide_kernel(const float* __restrict__ part, int nsplit, size_t n,
                                                                 float* __restrict__ out, float reg, const float* __restrict__ w) {
    __shared__ float4 red[32][16];
    splitk_reduce_wide_body(red, blockIdx.x, part, nsplit, n, out, reg, w);
}

// ---- several reductions in ONE launch (round 4).  A weight gradient's fixed-order reduction is 5-20 us of which most is the launch
// itself (37.7 MB of slabs at 1.9 TB/s; 1-64 K outputs at their launch floor), and a train step has 23 (configs[1]) to 57 (configs[4])
// of them.  The weight-gradient entry points can leave their slabs in the caller's workspace and hand back a descriptor instead
// (unetrir_*_wgrad_partials_*); unetrir_splitk_reduce_batched then reduces up to 16 of them per launch.  Every output element is summed
// by the same code over the same slab order as in the single launch (same group count, wide or narrow form per reduction): bit-identical.
#define REDUCE_BATCH 16
struct ReduceBatchArgs {
    unetrir_reduce_desc d[REDUCE_BATCH];
    unsigned first_block[REDUCE_BATCH + 1];       // workgroup range of reduction i: [first_block[i], first_block[i + 1])
    unsigned char kind[REDUCE_BATCH];             // 0: the wide form; 8 / 4 / 2 / 1: the narrow form with that many slab groups
    int n;
};
__global__ __launch_bounds__(512) void splitk_reduce_batched_kernel(const ReduceBatchArgs a) {
    __shared__ float4 red[8 * 64];                 // [8][64] (narrow, 8 slab groups) or [32][16] (wide)
    int i = 0;
    while (i + 1 < a.n && blockIdx.x >= a.first_block[i + 1]) ++i;
    const unetrir_reduce_desc& d = a.d[i];
    const unsigned blk = blockIdx.x - a.first_block[i];
    float4 (*r64)[64] = reinterpret_cast<float4 (*)[64]>(red);
    switch (a.kind[i]) {                           // uniform per workgroup
        case 0: splitk_reduce_wide_body(reinterpret_cast<float4 (*)[16]>(red), blk, d.part, d.nsplit, d.n, d.out, d.reg, d.w); break;
        case 8: splitk_reduce_body<8>(r64, blk, d.part, d.nsplit, d.n, d.out, d.reg, d.w); break;
        case 4: splitk_reduce_body<4>(r64, blk, d.part, d.nsplit, d.n, d.out, d.reg, d.w); break;
        case 2: splitk_reduce_body<2>(r64, blk, d.part, d.nsplit, d.n, d.out, d.reg, d.w); break;
        default: splitk_reduce_body<1>(r64, blk, d.part, d.nsplit, d.n, d.out, d.reg, d.w); break;
    }
}

// The form of one reduction: 0 = the wide kernel, else the narrow one with that many slab groups (8 / 4 / 2 / 1).  The single launch
// and the batched one both take it from here: the same groups sum the same slabs in the same order - bit-identical.
static int reduce_kind(int nsplit, size_t n, const float* part, const float* out, const float* w) {
    const size_t n4 = (n + 3) / 4;
    if ((n & 3) == 0 && nsplit >= 32 && (n4 + 63) / 64 < 128 && (((uintptr_t)part | (uintptr_t)out | (uintptr_t)w) & 15) == 0) return 0;
    return nsplit >= 8 ? 8 : nsplit >= 4 ? 4 : nsplit >= 2 ? 2 : 1;
}

extern "C" int unetrir_splitk_reduce_batched(const unetrir_reduce_desc* desc, int n, unetrir_stream_t stream) {
    if (n < 0 || (n > 0 && !desc)) return UNETRIR_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    ReduceBatchArgs a;
    a.n = 0;
    a.first_block[0] = 0;
    auto flush = [&]() -> int {
        if (a.n == 0) return 0;
        if (a.n == 1) {          // nothing to batch: the single launch
            const unetrir_reduce_desc& d = a.d[0];
            a.n = 0;
            return launch_splitk_reduce(d.part, d.nsplit, d.n, d.out, d.reg, d.w, s);
        }
        hipLaunchKernelGGL(splitk_reduce_batched_kernel, dim3(a.first_block[a.n]), dim3(512), 0, s, a);
        a.n = 0;
        return (int)hipGetLastError();
    };
    for (int i = 0; i < n; ++i) {
        const unetrir_reduce_desc& d = desc[i];
        if (d.nsplit == 0) continue;                            // the weight gradient went straight into dw: nothing to reduce
        if (!d.part || !d.out || d.nsplit < 0 || d.n == 0 || (d.reg != 0.f && !d.w)) return UNETRIR_EINVAL;
        const int kind = reduce_kind(d.nsplit, d.n, d.part, d.out, d.w);
        const size_t n4 = (d.n + 3) / 4;
        const size_t blocks = kind == 0 ? (n4 + 15) / 16 : (n4 + 63) / 64;
        if (blocks > 0x3fffffffu) return UNETRIR_EINVAL;
        if (a.n == REDUCE_BATCH || (size_t)a.first_block[a.n] + blocks > 0x7fffffffu) { const int e = flush(); if (e) return e; a.first_block[0] = 0; }
        a.d[a.n] = d;
        a.kind[a.n] = (unsigned char)kind;
        a.first_block[a.n + 1] = a.first_block[a.n] + (unsigned)blocks;
        ++a.n;
    }
    return flush();
}

int launch_splitk_reduce(const float* part, int nsplit, size_t n, float* out, float reg, const float* w, hipStream_t s) {
    const size_t n4 = (n + 3) / 4;
    const dim3 grid((unsigned)((n4 + 63) / 64));
    // (round 3: taking larger outputs too - up to 4096 narrow workgroups - moves single launches by +-8 us and the step by nothing)
    switch (reduce_kind(nsplit, n, part, out, w)) {
        case 0: hipLaunchKernelGGL(splitk_reduce_wide_kernel, dim3((unsigned)((n4 + 15) / 16)), dim3(512), 0, s, part, nsplit, n, out, reg, w); break;
        case 8: hipLaunchKernelGGL(splitk_reduce_kernel<8>, grid, dim3(512), 0, s, part, nsplit, n, out, reg, w); break;
        case 4: hipLaunchKernelGGL(splitk_reduce_kernel<4>, grid, dim3(256), 0, s, part, nsplit, n, out, reg, w); break;
        case 2: hipLaunchKernelGGL(splitk_reduce_kernel<2>, grid, dim3(128), 0, s, part, nsplit, n, out, reg, w); break;
        default: hipLaunchKernelGGL(splitk_reduce_kernel<1>, grid, dim3(64), 0, s, part, nsplit, n, out, reg, w); break;
    }
    return (int)hipGetLastError();
}
