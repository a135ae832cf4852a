// vq.hip - the VectorQuantizer layer of dl_models/vqvae.py:42-98: nearest-code search, straight-through output and the
// commitment + codebook loss in one forward launch; the input gradient and the codebook's segmented-sum gradient in two backward
// launches.  fp32 in both storage modes, plain HIP C++, no float atomics anywhere; the contracts are in include/unetrir.h.
#include "kernels.h"

#define VQ_T 256
#define VQ_MAXG 1024           // most workgroups of the forward launch = most fp64 partials in ws
#define VQ_WS_HEAD 16          // bytes in front of the partials: the arrival counter (left zero by every launch)

// One thread per vector.  The codebook E [D][K] is staged once per workgroup as Es [K][D] (a code's D numbers are consecutive:
// every lane of a wave reads the SAME 16 bytes at a time, a broadcast), n_k = ||E_k||^2 once per workgroup.
//   s_k   = fma chain over d = 0 .. D-1 from 0:  s = fmaf(x_d, E_dk, s)
//   n_k   = fma chain over d = 0 .. D-1 from 0:  n = fmaf(E_dk, E_dk, n)
//   dist_k = fmaf(-2, s_k, n_k)                  the row-constant ||x||^2 of vqvae.py:90-94 is dropped
//   idx   = the lowest k whose dist_k is smallest (codes visited in ascending k, replaced on a strictly smaller distance)
// Four codes are in flight at a time (four independent chains: the order inside each chain is the one above).
// M: the number of 16-byte pieces of a vector held in registers; D / 4 <= M.
template <int M>
__global__ __launch_bounds__(VQ_T) void vq_fwd_kernel(const float* __restrict__ x, int nvec, int vpp, int ld, int D,
                                                      const float* __restrict__ E, int K, float scale, int* __restrict__ idx,
                                                      float* __restrict__ y, int ld_y, float* __restrict__ vq_out,
                                                      unsigned* __restrict__ counter, unsigned long long* __restrict__ part) {
    extern __shared__ float4 vq_smem[];
    float* Es = reinterpret_cast<float*>(vq_smem);                 // [K][D]
    float* En = Es + (size_t)K * D;                                // [K]
    double* red = reinterpret_cast<double*>(En + K);               // [VQ_T]; K * (D + 1) * 4 is a multiple of 16
    __shared__ int is_last;
    const int t = threadIdx.x, D4 = D >> 2;
    for (int e = t; e < K * D; e += VQ_T) {          // by destination: consecutive lanes, consecutive LDS words (no bank conflict);
        const int k = e / D, d = e - k * D;           // the transposed reads come from L2, once per workgroup
        Es[e] = E[(size_t)d * K + k];
    }
    __syncthreads();
    for (int k = t; k < K; k += VQ_T) {
        float n = 0.0f;
        for (int d = 0; d < D; ++d) n = fmaf(Es[k * D + d], Es[k * D + d], n);
        En[k] = n;
    }
    __syncthreads();
    const float4* Es4 = reinterpret_cast<const float4*>(Es);
    const float4* En4 = reinterpret_cast<const float4*>(En);
    double acc = 0.0;
    for (long long v = (long long)blockIdx.x * VQ_T + t; v < nvec; v += (long long)gridDim.x * VQ_T) {
        const int p = (int)v / vpp, j = (int)v - p * vpp;
        const float* xp = x + (long long)p * ld + j * D;
        float4 xr[M];
#pragma unroll
        for (int c = 0; c < M; ++c)
            if (c < D4) xr[c] = *reinterpret_cast<const float4*>(xp + 4 * c);
        float best = __builtin_inff();
        int bi = 0;
        for (int k0 = 0; k0 < K; k0 += 4) {
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
            const float4* e0 = Es4 + (size_t)k0 * D4;
#pragma unroll
            for (int c = 0; c < M; ++c) {
                if (c < D4) {
                    const float4 a = e0[c], b = e0[D4 + c], g = e0[2 * D4 + c], h = e0[3 * D4 + c], xv = xr[c];
                    s0 = fmaf(xv.x, a.x, s0); s1 = fmaf(xv.x, b.x, s1); s2 = fmaf(xv.x, g.x, s2); s3 = fmaf(xv.x, h.x, s3);
                    s0 = fmaf(xv.y, a.y, s0); s1 = fmaf(xv.y, b.y, s1); s2 = fmaf(xv.y, g.y, s2); s3 = fmaf(xv.y, h.y, s3);
                    s0 = fmaf(xv.z, a.z, s0); s1 = fmaf(xv.z, b.z, s1); s2 = fmaf(xv.z, g.z, s2); s3 = fmaf(xv.z, h.z, s3);
                    s0 = fmaf(xv.w, a.w, s0); s1 = fmaf(xv.w, b.w, s1); s2 = fmaf(xv.w, g.w, s2); s3 = fmaf(xv.w, h.w, s3);
                }
            }
            const float4 n = En4[k0 >> 2];
            const float d0 = fmaf(-2.0f, s0, n.x), d1 = fmaf(-2.0f, s1, n.y), d2 = fmaf(-2.0f, s2, n.z), d3 = fmaf(-2.0f, s3, n.w);
            if (d0 < best) { best = d0; bi = k0; }
            if (d1 < best) { best = d1; bi = k0 + 1; }
            if (d2 < best) { best = d2; bi = k0 + 2; }
            if (d3 < best) { best = d3; bi = k0 + 3; }
        }
        idx[v] = bi;
        // quantized = E[:, idx]; y = x + (quantized - x) (vqvae.py:84: two roundings, not quantized); S += (quantized - x)^2
        float* yp = y + (long long)p * ld_y + j * D;
        const float4* q4 = Es4 + (size_t)bi * D4;
#pragma unroll
        for (int c = 0; c < M; ++c) {
            if (c < D4) {
                const float4 q = q4[c], xv = xr[c];
                float4 df, o;
                df.x = q.x - xv.x; df.y = q.y - xv.y; df.z = q.z - xv.z; df.w = q.w - xv.w;
                o.x = xv.x + df.x; o.y = xv.y + df.y; o.z = xv.z + df.z; o.w = xv.w + df.w;
                *reinterpret_cast<float4*>(yp + 4 * c) = o;
                acc += (double)(df.x * df.x);
                acc += (double)(df.y * df.y);
                acc += (double)(df.z * df.z);
                acc += (double)(df.w * df.w);
            }
        }
    }
    // the workgroup's partial: a fixed tree over its threads
    red[t] = acc;
    __syncthreads();
    for (int s = VQ_T / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    // hand the partial over; the workgroup whose arrival is the last one - told by the value its add returned - combines them.
    // Partials travel as agent-scope 8-byte stores and loads, bracketed by an agent-scope release on the storing lane and an
    // acquire in the combining workgroup: each XCD has an L2 of its own.
    if (t == 0) {
        __hip_atomic_store(part + blockIdx.x, (unsigned long long)__double_as_longlong(red[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned arrived = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        is_last = arrived == gridDim.x - 1;
    }
    __syncthreads();
    if (!is_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    // S = the partials in a fixed order that depends on the grid alone: thread t adds those of workgroups t, t + 256, t + 512,
    // t + 768 in that order, then the same tree
    double s = 0.0;
    for (int b = t; b < (int)gridDim.x; b += VQ_T)
        s += __longlong_as_double((long long)__hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    red[t] = s;
    __syncthreads();
    for (int h = VQ_T / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) {
        const float raw = (float)red[0];
        vq_out[1] = raw;                  // S = sum (quantized - x)^2 over all rows * C elements
        vq_out[0] = scale * raw;          // r (1 + beta) S / N: beta commitment_loss + codebook_loss over the replicas (vqvae.py:79-81)
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch finds zero
    }
}

// dx = dy + cdx (x - E[:, idx]), cdx = r beta 2 / N: fmaf(cdx, x - q, dy), two roundings.  An index outside [0, K) is clamped
// into the range (nothing outside the codebook is read).
__global__ void vq_bwd_dx_kernel(const float* __restrict__ x, int nvec, int vpp, int ld, int D, const int* __restrict__ idx,
                                 const float* __restrict__ E, int K, const float* __restrict__ dy, int ld_dy, float cdx,
                                 float* __restrict__ dx, int ld_dx) {
    const int D4 = D >> 2;
    const long long n4 = (long long)nvec * D4;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < n4; u += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(u / D4), c = (int)(u - (long long)v * D4) << 2;
        const int p = v / vpp, j = v - p * vpp;
        int k = idx[v];
        k = k < 0 ? 0 : (k >= K ? K - 1 : k);
        const long long col = (long long)j * D + c;
        const float4 xv = *reinterpret_cast<const float4*>(x + (long long)p * ld + col);
        const float4 g = *reinterpret_cast<const float4*>(dy + (long long)p * ld_dy + col);
        const float* e = E + (size_t)c * K + k;
        float4 o;
        o.x = fmaf(cdx, xv.x - e[0], g.x);
        o.y = fmaf(cdx, xv.y - e[K], g.y);
        o.z = fmaf(cdx, xv.z - e[2 * (size_t)K], g.z);
        o.w = fmaf(cdx, xv.w - e[3 * (size_t)K], g.w);
        *reinterpret_cast<float4*>(dx + (long long)p * ld_dx + col) = o;
    }
}

// dE[:, k] = cde * sum over the vectors i with idx_i == k of (E[:, k] - x_i), cde = 2 r / N: one workgroup per code, lane d of
// each of its four waves owns dimension d (D <= 64).  Wave w scans the vectors [w 64 + 256 m, w 64 + 256 m + 64), m = 0, 1, ...:
// every lane compares one index, the wave visits the matches in ascending vector order and adds fl(E_dk - x_id) to its lane's
// fp32 partial; dE = cde * (((p_0 + p_1) + p_2) + p_3).  The order depends on the indices alone - no atomics, nothing that depends
// on which wave finishes first - and a code nobody chose gets cde * 0 = 0.
__global__ __launch_bounds__(VQ_T) void vq_bwd_de_kernel(const float* __restrict__ x, int nvec, int vpp, int ld, int D,
                                                         const int* __restrict__ idx, const float* __restrict__ E, int K, float cde,
                                                         float* __restrict__ dE) {
    __shared__ float red[VQ_T];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, k = blockIdx.x;
    const float q = lane < D ? E[(size_t)lane * K + k] : 0.0f;
    float acc = 0.0f;
    for (long long base0 = (long long)w * 64; base0 < nvec; base0 += 4 * VQ_T) {
        int id[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long v = base0 + (long long)u * VQ_T + lane;
            id[u] = v < nvec ? idx[v] : -1;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned long long m = __ballot(id[u] == k);
            const int base = (int)(base0 + (long long)u * VQ_T);         // matches exist only below nvec < 2^31
            while (m) {
                const int vv = base + (__ffsll((unsigned long long)m) - 1);
                m &= m - 1;
                if (lane < D) {
                    const int p = vv / vpp, j = vv - p * vpp;
                    acc += q - x[(long long)p * ld + (long long)j * D + lane];
                }
            }
        }
    }
    red[t] = acc;
    __syncthreads();
    if (t < D) dE[(size_t)t * K + k] = cde * (((red[t] + red[64 + t]) + red[128 + t]) + red[192 + t]);
}

static inline bool vq_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }

// the geometry rules of include/unetrir.h; on success *nvec = rows * C / D
static bool vq_bad_geom(long long rows, int ld, int C, int D, int K, int* nvec) {
    if (rows <= 0 || D < 4 || D > 64 || (D & 3) || K < 4 || K > 512 || (K & 3) || C <= 0 || C % D || ld < C || (ld & 3)) return true;
    const long long n = rows * (long long)(C / D);
    if (n > 0x7FFFFFFFLL || rows * (long long)ld > 0x7FFFFFFFFFFLL) return true;
    *nvec = (int)n;
    return false;
}

template <int M>
static int vq_fwd_launch(dim3 grid, size_t smem, hipStream_t stream, const float* x, int nvec, int vpp, int ld, int D, const float* E,
                         int K, float scale, int* idx, float* y, int ld_y, float* vq_out, unsigned* counter, unsigned long long* part) {
    if (smem > (64 << 10)) {          // dynamic LDS above 64 KB has to be asked for, per device: asked on every such call (no state kept)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&vq_fwd_kernel<M>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(vq_fwd_kernel<M>, grid, dim3(VQ_T), smem, stream, x, nvec, vpp, ld, D, E, K, scale, idx, y, ld_y, vq_out, counter, part);
    return (int)hipGetLastError();
}

extern "C" {

size_t unetrir_vq_ws_bytes(void) { return VQ_WS_HEAD + (size_t)VQ_MAXG * sizeof(double); }

int unetrir_vq_fwd_f32(const float* x, long long rows, int ld, int C, int D, const float* E, int K, float beta, float r, int32_t* idx,
                       float* y, int ld_y, float* vq_out, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    int nvec = 0;
    if (!x || !E || !idx || !y || !vq_out || !ws || vq_bad_geom(rows, ld, C, D, K, &nvec) || ld_y < C || (ld_y & 3)) return UNETRIR_EINVAL;
    if (ws_bytes < unetrir_vq_ws_bytes() || vq_misaligned(x) || vq_misaligned(y) || vq_misaligned(ws)) return UNETRIR_EINVAL;
    const int G = (nvec + VQ_T - 1) / VQ_T < VQ_MAXG ? (nvec + VQ_T - 1) / VQ_T : VQ_MAXG;
    const size_t smem = (size_t)K * (D + 1) * sizeof(float) + VQ_T * sizeof(double);
    const float scale = (float)((double)r * (1.0 + (double)beta) / ((double)rows * C));
    unsigned* counter = static_cast<unsigned*>(ws);
    unsigned long long* part = reinterpret_cast<unsigned long long*>(static_cast<char*>(ws) + VQ_WS_HEAD);
    const int D4 = D >> 2, vpp = C / D;
    hipStream_t s = (hipStream_t)stream;
#define VQ_GO(M) vq_fwd_launch<M>(dim3(G), smem, s, x, nvec, vpp, ld, D, E, K, scale, idx, y, ld_y, vq_out, counter, part)
    if (D4 <= 1) return VQ_GO(1);
    if (D4 <= 2) return VQ_GO(2);
    if (D4 <= 4) return VQ_GO(4);
    if (D4 <= 8) return VQ_GO(8);
    return VQ_GO(16);
#undef VQ_GO
}

int unetrir_vq_bwd_f32(const float* x, long long rows, int ld, int C, int D, const int32_t* idx, const float* E, int K, const float* dy,
                       int ld_dy, float beta, float r, float* dx, int ld_dx, float* dE, unetrir_stream_t stream) {
    int nvec = 0;
    if (!x || !idx || !E || !dy || !dx || !dE || vq_bad_geom(rows, ld, C, D, K, &nvec) || ld_dy < C || (ld_dy & 3) || ld_dx < C || (ld_dx & 3))
        return UNETRIR_EINVAL;
    if (vq_misaligned(x) || vq_misaligned(dy) || vq_misaligned(dx)) return UNETRIR_EINVAL;
    const double N = (double)rows * C;
    const float cdx = (float)(2.0 * (double)r * (double)beta / N), cde = (float)(2.0 * (double)r / N);
    const long long n4 = (long long)nvec * (D >> 2);
    const long long blocks = (n4 + VQ_T - 1) / VQ_T;
    hipLaunchKernelGGL(vq_bwd_dx_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(VQ_T), 0, (hipStream_t)stream, x, nvec, C / D,
                       ld, D, idx, E, K, dy, ld_dy, cdx, dx, ld_dx);
    hipLaunchKernelGGL(vq_bwd_de_kernel, dim3(K), dim3(VQ_T), 0, (hipStream_t)stream, x, nvec, C / D, ld, D, idx, E, K, cde, dE);
    return (int)hipGetLastError();
}

}  // extern "C"
