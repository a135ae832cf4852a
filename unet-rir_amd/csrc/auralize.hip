// auralize.hip - render dry audio through impulse responses: y_b = h_b * x_b, direct form on the fp32 matrix cores (gfx950).
//
//     y_b[n] = sum_{k=0}^{K-1} h_b[k] x_b[n - k]          0 <= n < L <= N + K - 1,   x_b[m] = 0 outside 0 <= m < N
//
// h fp32 [B][K] (the waveforms PostProcess / GriffinLim return), x fp32 [N] shared by all rows (dry_stride = 0: one source heard at B
// microphone positions) or [B][dry_stride >= N], y fp32 [B][L].
//
// Formulation.  Substitute u = k - i.  The 1024 consecutive outputs n0 + 32 j + i (i, j in [0, 32)) of one row are a 32 x 32 GEMM tile
//
//     Y[i][j] = sum_u A[i][u] S[u][j]        A[i][u] = h[u + i]  (zero outside [0, K))        S[u][j] = x[n0 + 32 j - u]
//
// over u in [-32, K - 1]: A is a Hankel view of h, S a sliding view of x, and neither is formed anywhere - a lane of
// v_mfma_f32_32x32x2_f32 holds A[i = lane & 31][u0 + (lane >> 5)] and S[u0 + (lane >> 5)][j = lane & 31], each ONE ds_read_b32 out of an
// LDS copy of h resp. of the x window (both zero-padded at the ends).  The A fragment does not depend on n0, so a wave keeps AU_TILES
// tiles (4096 consecutive outputs) per fragment: 5 LDS reads per 4 MFMAs.  Wasted work is the 32 (+ at most 7) extra values of u.
//
// LDS.  A workgroup (4 waves) owns AU_OUT = 16384 consecutive outputs of one row.  It stages ONCE the x window those outputs can
// reach, x[n0 - U + 1 ... n0 + AU_OUT] with U = UT - 32 and UT = K + 32 rounded up to 8 (the number of u values walked), at index
// q + (q >> 5): one pad word per 32, so that the 32 lanes of a read group, 32 samples apart, fall into 32 different banks.  h is staged
// in chunks of AU_CH = 1024 values of u (+ 31 for the Hankel rows) into two buffers; the chunks are walked in ascending order and the
// loads of chunk c + 1 are issued to registers before the products of chunk c, and written to the other buffer after them.
//     K = 16384:  ((16384 + 16384) * 33/32 + 1 + 2 * 1056) * 4  =  143 620 bytes of the 160 KB;   K = 9600:  115 636 bytes.
//
// Order.  Every MFMA adds its two products to the accumulator as an fp32 fma chain in ascending u, and the accumulator of an output
// starts at +0, so
//     y[n] = fma(h[K-1], x[n-K+1], ... fma(h[1], x[n-1], fma(h[0], x[n], +0)) ...)        (terms outside x are exact zeros)
// whatever n0, B, L, the row's place in the batch and the layout of x: no atomics, no workspace, one store per output.  The tile grid
// is anchored at n = 0.  Inputs are taken to be finite (a zero of the padding times an infinity is a NaN up to 39 samples away).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "kernels.h"
#include "mfma_types.h"

namespace {

constexpr int AU_THREADS = 256;
constexpr int AU_WAVES = AU_THREADS / 64;
constexpr int AU_TILES = 4;                             // 32 x 32 accumulator tiles per wave
constexpr int AU_WOUT = AU_TILES * 1024;                // outputs per wave
constexpr int AU_OUT = AU_WAVES * AU_WOUT;              // outputs per workgroup
constexpr int AU_CH = 1024;                             // values of u per staged chunk of h
constexpr int AU_HB = AU_CH + 32;                       // floats per h buffer: the chunk plus the 31 further taps of the Hankel rows
constexpr int AU_HR = (AU_HB + AU_THREADS - 1) / AU_THREADS;
constexpr int AU_XR = 8;                                // window samples a lane loads before it writes them to LDS
constexpr int AU_MAXK = 16384;

__host__ __device__ constexpr int au_ut(int K) { return (K + 32 + 7) & ~7; }          // values of u walked: -32 ... UT - 33
__host__ __device__ constexpr int au_xpad(int q) { return q + (q >> 5); }             // index of window sample q in LDS

// h[u0 + e] for e = tid + 256 r, zero outside [0, K): the next chunk's buffer image, held in registers
__device__ __forceinline__ void au_load_h(float (&hr)[AU_HR], const float* __restrict__ h, int K, int u0, int tid) {
#pragma unroll
    for (int r = 0; r < AU_HR; ++r) {
        const int k = u0 + tid + AU_THREADS * r;
        hr[r] = (k >= 0 && k < K) ? h[k] : 0.f;
    }
}
__device__ __forceinline__ void au_store_h(const float (&hr)[AU_HR], float* hb, int tid) {
#pragma unroll
    for (int r = 0; r < AU_HR; ++r) {
        const int e = tid + AU_THREADS * r;
        if (e < AU_HB) hb[e] = hr[r];
    }
}

// The operands of AU_G consecutive MFMA steps of a lane: a[d] = A[i][u0 + 2 (s + d) + kh] = hl[2 (s + d)], b[d][t] = S[.][j] of tile t =
// window sample q0 - 2 (s + d) (+ 32 j, folded into xl, + 1024 t: 1056 words on)
constexpr int AU_G = 2;
struct AuFrag {
    float a[AU_G], b[AU_G][AU_TILES];
};
__device__ __forceinline__ void au_read(AuFrag& f, const float* hl, const float* xl, int q0, int s) {
#pragma unroll
    for (int d = 0; d < AU_G; ++d) {
        f.a[d] = hl[2 * (s + d)];
        const float* xp = xl + au_xpad(q0 - 2 * (s + d));
#pragma unroll
        for (int t = 0; t < AU_TILES; ++t) f.b[d][t] = xp[1056 * t];
    }
}

__device__ __forceinline__ void au_mma(f32x16 (&acc)[AU_TILES], const AuFrag& f) {
#pragma unroll
    for (int d = 0; d < AU_G; ++d)
#pragma unroll
        for (int t = 0; t < AU_TILES; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(f.a[d], f.b[d][t], acc[t], 0, 0, 0);
}

__global__ __launch_bounds__(AU_THREADS) void auralize_kernel(const float* __restrict__ rir, const float* __restrict__ dry,
                                                              float* __restrict__ out, int K, int N, long long dry_stride, int L,
                                                              int nblk) {
    extern __shared__ __attribute__((aligned(16))) float au_smem[];
    float* hs = au_smem;                                // [2][AU_HB]
    float* xs = au_smem + 2 * AU_HB;                    // the padded x window
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ij = lane & 31, kh = lane >> 5;
    const int b = blockIdx.x / nblk;
    const long long n0 = (long long)(blockIdx.x - b * nblk) * AU_OUT;
    const float* __restrict__ h = rir + (size_t)b * K;
    const float* __restrict__ x = dry + (long long)b * dry_stride;
    float* __restrict__ y = out + (size_t)b * L;
    const int UT = au_ut(K), U = UT - 32, nch = (UT + AU_CH - 1) / AU_CH;
    // the waves of this workgroup that own an output, and the window those reach: sample q is x[n0 - U + 1 + q]
    const long long left = (long long)L - n0;
    const int nact = left >= AU_OUT ? AU_WAVES : (int)((left + AU_WOUT - 1) / AU_WOUT);
    const int xlen = nact * AU_WOUT + U;
    const long long wb = n0 - U + 1;

    float hr[AU_HR];
    au_load_h(hr, h, K, -32, tid);
    for (int qb = tid; qb < xlen; qb += AU_XR * AU_THREADS) {            // AU_XR loads in flight per lane, then their LDS writes
        float v[AU_XR];
#pragma unroll
        for (int r = 0; r < AU_XR; ++r) {
            const int q = qb + AU_THREADS * r;
            const long long m = wb + q;
            v[r] = (q < xlen && m >= 0 && m < N) ? x[m] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < AU_XR; ++r) {
            const int q = qb + AU_THREADS * r;
            if (q < xlen) xs[au_xpad(q)] = v[r];
        }
    }
    au_store_h(hr, hs, tid);
    __syncthreads();

    f32x16 acc[AU_TILES];
#pragma unroll
    for (int t = 0; t < AU_TILES; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const bool active = wave < nact;
    const float* xl = xs + 33 * ij;                     // column j = ij of every tile: 32 j samples on, 33 j words
    for (int c = 0; c < nch; ++c) {
        const int u0 = -32 + c * AU_CH;
        if (c + 1 < nch) au_load_h(hr, h, K, u0 + AU_CH, tid);            // in flight during the products below
        if (active) {
            const int steps = (UT - c * AU_CH < AU_CH ? UT - c * AU_CH : AU_CH) >> 1;       // a multiple of 4
            const float* hl = hs + (c & 1) * AU_HB + kh + ij;                               // A[i][u0 + 2 s + kh] = hl[2 s]
            // S[u][j] of tile t = window sample (U - 1 - u) + 32 j + 1024 t + 4096 wave
            const int q0 = U - 1 - u0 - kh + AU_WOUT * wave;
            // groups of AU_G steps, the fragments of the next group read from LDS before the MFMAs of this one (one wave per SIMD: nothing
            // else hides the read latency; the scheduling barriers keep the compiler from sinking the reads to their uses); steps is a
            // multiple of 2 AU_G, and the last pair re-reads a group instead of branching
            AuFrag f0, f1;
            au_read(f0, hl, xl, q0, 0);
            for (int s = 0; s < steps; s += 2 * AU_G) {
                au_read(f1, hl, xl, q0, s + AU_G);
                __builtin_amdgcn_sched_barrier(0);
                au_mma(acc, f0);
                __builtin_amdgcn_sched_barrier(0);
                au_read(f0, hl, xl, q0, s + 2 * AU_G < steps ? s + 2 * AU_G : s);
                __builtin_amdgcn_sched_barrier(0);
                au_mma(acc, f1);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (c + 1 < nch) au_store_h(hr, hs + ((c + 1) & 1) * AU_HB, tid);   // last read two chunks ago, before the barrier of chunk c - 1
        __syncthreads();
    }

    if (!active) return;
    // C/D layout: column j on the lane, row i = (r & 3) + 8 (r >> 2) + 4 kh in register r: four consecutive outputs per register quad
#pragma unroll
    for (int t = 0; t < AU_TILES; ++t) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const long long n = n0 + AU_WOUT * wave + 1024 * t + 32 * ij + 8 * g + 4 * kh;
            if (n >= L) continue;
            float* p = y + n;
            if (n + 3 < L && ((uintptr_t)p & 15) == 0) {
                *reinterpret_cast<float4*>(p) = make_float4(acc[t][4 * g], acc[t][4 * g + 1], acc[t][4 * g + 2], acc[t][4 * g + 3]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (n + e < L) p[e] = acc[t][4 * g + e];
            }
        }
    }
}

size_t au_smem_bytes(int K) { return (size_t)(2 * AU_HB + au_xpad(AU_OUT + au_ut(K) - 32) + 1) * sizeof(float); }

}  // namespace

extern "C" {

int unetrir_auralize_supported(int K) { return K >= 1 && K <= AU_MAXK ? 1 : 0; }

int unetrir_auralize_f32(const float* rir, const float* dry, float* out, int B, int K, int N, long long dry_stride, int L,
                         unetrir_stream_t stream) {
    if (!rir || !dry || !out || B < 1 || K < 1 || N < 1 || !unetrir_auralize_supported(K)) return UNETRIR_EINVAL;
    if (L < 1 || (long long)L > (long long)N + K - 1) return UNETRIR_EINVAL;
    if (dry_stride != 0 && dry_stride < N) return UNETRIR_EINVAL;
    const long long nblk = ((long long)L + AU_OUT - 1) / AU_OUT;
    if (nblk * B > 0x7fffffffLL) return UNETRIR_EINVAL;
    const size_t smem = au_smem_bytes(K);
    if (smem > (64 << 10)) {
        // Dynamic LDS above 64 KB has to be asked for, per device: asked once, for the most any K needs, and remembered in an
        // append-only flag per device (a race sets it twice: harmless).  A property of the function, not a stream operation.
        static std::atomic<bool> asked[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return UNETRIR_EINVAL;
        if (!asked[dev].load(std::memory_order_acquire)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&auralize_kernel),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)au_smem_bytes(AU_MAXK));
            if (e != hipSuccess) return (int)e;
            asked[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL(auralize_kernel, dim3((unsigned)(nblk * B)), dim3(AU_THREADS), smem, (hipStream_t)stream, rir, dry, out, K, N,
                       dry_stride, L, (int)nblk);
    return (int)hipGetLastError();
}

}  // extern "C"
