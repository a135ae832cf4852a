// lamb.hip - tfa.optimizers.LAMB(learning_rate) of trainer.py:37-38: Adam's moments, the bias-corrected update u, and per VARIABLE
// the trust ratio r = ||w|| / ||u|| that scales the step.  Three launches over any range of whole variables, whatever their number:
//   pass 1  (one workgroup per chunk)     m, v updated in place; fp64 partial sums of w^2 and u^2 of the chunk -> ws
//   ratio   (one workgroup per variable)  the variable's partials combined in an order that depends on its chunk count alone -> r
//   pass 2  (one workgroup per chunk)     u recomputed from the stored m, v and the old w by the SAME device function; w -= lr r u
// A chunk is LAMB_CHUNK consecutive elements of ONE variable, numbered from the variable's own first element, so a variable's
// reduction order - and with it every bit of the result - is the same whether a launch covers the whole buffer or one bucket.
// Plain HIP C++, no atomics; the contracts are in include/unetrir.h.
#include "kernels.h"

#define LAMB_T 256
#define LAMB_CHUNK 4096            // floats: four 16-byte groups per thread, two in flight at a time (as adam_kernel)

struct LambHyper { float lr, b1, b2, eps, wd, c1, c2, gs; };

static inline long long lamb_chunks_of(long long count) { return (count + LAMB_CHUNK - 1) / LAMB_CHUNK; }

// Device form (HIP-graph replay): the step count comes from state[0] and lr, the betas, eps and grad_scale from cfg (what
// unetrir_step_advance reads); one thread forms the two corrections in fp64 by the expression the host uses for the launched form.
__device__ __forceinline__ LambHyper lamb_hyper(LambHyper h, const unsigned long long* __restrict__ state, const float* __restrict__ cfg) {
    if (!state) return h;
    __shared__ LambHyper sh;
    if (threadIdx.x == 0) {
        const double t = (double)state[0];
        sh.lr = cfg[0]; sh.b1 = cfg[1]; sh.b2 = cfg[2]; sh.eps = cfg[3]; sh.gs = cfg[4]; sh.wd = h.wd;
        sh.c1 = (float)(1.0 - pow((double)cfg[1], t));
        sh.c2 = (float)(1.0 - pow((double)cfg[2], t));
    }
    __syncthreads();
    return sh;
}

// u = m^ / (sqrt(v^) + eps) [+ weight_decay w]: every operation rounded on its own (no contraction), so that pass 1 (the norm) and
// pass 2 (the step) hold the same bits.
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambHyper& h, bool decay) {
#pragma clang fp contract(off)
    const float mh = m / h.c1, vh = v / h.c2;
    float u = mh / (sqrtf(vh) + h.eps);
    if (decay) u = u + h.wd * w;
    return u;
}

// sum over the workgroup in a fixed order: a shuffle tree inside each wave, the four waves' sums in wave order; valid in thread 0
__device__ __forceinline__ void lamb_block_sum(double& a, double& b, double (*red)[2]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[wv][0] = a; red[wv][1] = b; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < LAMB_T / 64; ++k) { a += red[k][0]; b += red[k][1]; }
}

// the workgroup's chunk: variable, and the chunk's element range [e0, e1) inside it
struct LambChunk { long long base, e0, e1; int seg, flags; };
__device__ __forceinline__ LambChunk lamb_chunk(const unetrir_lamb_seg* __restrict__ segs, const int* __restrict__ chunk_seg, int chunk) {
    LambChunk c;
    c.seg = chunk_seg[chunk];
    const unetrir_lamb_seg s = segs[c.seg];
    c.base = s.offset; c.flags = s.flags;
    c.e0 = (long long)(chunk - s.chunk0) * LAMB_CHUNK;
    c.e1 = c.e0 + LAMB_CHUNK < s.count ? c.e0 + LAMB_CHUNK : s.count;
    return c;
}

__global__ __launch_bounds__(LAMB_T) void lamb_moments_kernel(const float* __restrict__ theta, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, const unetrir_lamb_seg* __restrict__ segs,
                                                              const int* __restrict__ chunk_seg, int chunk_lo, LambHyper hy,
                                                              const unsigned long long* __restrict__ state, const float* __restrict__ cfg,
                                                              double* __restrict__ part) {
    __shared__ double red[LAMB_T / 64][2];
    const LambHyper h = lamb_hyper(hy, state, cfg);
    const int chunk = chunk_lo + blockIdx.x;
    const LambChunk c = lamb_chunk(segs, chunk_seg, chunk);
    const bool decay = (c.flags & UNETRIR_LAMB_DECAY) != 0 && h.wd != 0.f;
    double sw = 0.0, su = 0.0;
    // elements past the variable's real count (the alignment tail of its slot) are carried through unchanged and add nothing
    for (int it = 0; it < 2; ++it) {
        const long long ea = c.e0 + 4ll * (threadIdx.x + 2 * it * LAMB_T), eb = ea + 4ll * LAMB_T;
        const bool one = ea < c.e1, two = eb < c.e1;
        float4 t[2], gg[2], mm[2], vv[2];
        if (one) {
            t[0] = *reinterpret_cast<const float4*>(theta + c.base + ea); gg[0] = *reinterpret_cast<const float4*>(g + c.base + ea);
            mm[0] = *reinterpret_cast<const float4*>(m + c.base + ea); vv[0] = *reinterpret_cast<const float4*>(v + c.base + ea);
        }
        if (two) {
            t[1] = *reinterpret_cast<const float4*>(theta + c.base + eb); gg[1] = *reinterpret_cast<const float4*>(g + c.base + eb);
            mm[1] = *reinterpret_cast<const float4*>(m + c.base + eb); vv[1] = *reinterpret_cast<const float4*>(v + c.base + eb);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!(u ? two : one)) break;
            const long long e = u ? eb : ea;
            const float* tp = &t[u].x; const float* gp = &gg[u].x; float* mp = &mm[u].x; float* vp = &vv[u].x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e + k < c.e1) {
                    const float gk = gp[k] * h.gs;
                    mp[k] = h.b1 * mp[k] + (1.f - h.b1) * gk;
                    vp[k] = h.b2 * vp[k] + (1.f - h.b2) * gk * gk;
                    const float uk = lamb_u(mp[k], vp[k], tp[k], h, decay);
                    sw += (double)tp[k] * (double)tp[k];
                    su += (double)uk * (double)uk;
                }
            }
            *reinterpret_cast<float4*>(m + c.base + e) = mm[u];
            *reinterpret_cast<float4*>(v + c.base + e) = vv[u];
        }
    }
    lamb_block_sum(sw, su, red);
    if (threadIdx.x == 0) { part[2ll * chunk] = sw; part[2ll * chunk + 1] = su; }
}

// r = ||w|| / ||u|| of variable seg_lo + blockIdx.x: thread t adds chunks t, t + 256, ... in ascending order, then the fixed tree
__global__ __launch_bounds__(LAMB_T) void lamb_ratio_kernel(const unetrir_lamb_seg* __restrict__ segs, int seg_lo, const double* __restrict__ part,
                                                            float* __restrict__ ratio) {
    __shared__ double red[LAMB_T / 64][2];
    const int s = seg_lo + blockIdx.x;
    const unetrir_lamb_seg sg = segs[s];
    const long long nch = (sg.count + LAMB_CHUNK - 1) / LAMB_CHUNK;
    double sw = 0.0, su = 0.0;
    for (long long k = threadIdx.x; k < nch; k += LAMB_T) { sw += part[2 * (sg.chunk0 + k)]; su += part[2 * (sg.chunk0 + k) + 1]; }
    lamb_block_sum(sw, su, red);
    if (threadIdx.x == 0) {
        const double nw = sqrt(sw), nu = sqrt(su);
        ratio[s] = ((sg.flags & UNETRIR_LAMB_ADAPT) && nw > 0.0 && nu > 0.0) ? (float)(nw / nu) : 1.f;
    }
}

__global__ __launch_bounds__(LAMB_T) void lamb_apply_kernel(float* __restrict__ theta, const float* __restrict__ m, const float* __restrict__ v,
                                                            const unetrir_lamb_seg* __restrict__ segs, const int* __restrict__ chunk_seg,
                                                            int chunk_lo, LambHyper hy, const unsigned long long* __restrict__ state,
                                                            const float* __restrict__ cfg, const float* __restrict__ ratio) {
    const LambHyper h = lamb_hyper(hy, state, cfg);
    const LambChunk c = lamb_chunk(segs, chunk_seg, chunk_lo + blockIdx.x);
    const bool decay = (c.flags & UNETRIR_LAMB_DECAY) != 0 && h.wd != 0.f;
    const float step = h.lr * ratio[c.seg];
    for (int it = 0; it < 2; ++it) {
        const long long ea = c.e0 + 4ll * (threadIdx.x + 2 * it * LAMB_T), eb = ea + 4ll * LAMB_T;
        const bool one = ea < c.e1, two = eb < c.e1;
        float4 t[2], mm[2], vv[2];
        if (one) {
            t[0] = *reinterpret_cast<const float4*>(theta + c.base + ea);
            mm[0] = *reinterpret_cast<const float4*>(m + c.base + ea); vv[0] = *reinterpret_cast<const float4*>(v + c.base + ea);
        }
        if (two) {
            t[1] = *reinterpret_cast<const float4*>(theta + c.base + eb);
            mm[1] = *reinterpret_cast<const float4*>(m + c.base + eb); vv[1] = *reinterpret_cast<const float4*>(v + c.base + eb);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (!(u ? two : one)) break;
            const long long e = u ? eb : ea;
            float* tp = &t[u].x; const float* mp = &mm[u].x; const float* vp = &vv[u].x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#pragma clang fp contract(off)
                if (e + k < c.e1) tp[k] = tp[k] - step * lamb_u(mp[k], vp[k], tp[k], h, decay);
            }
            *reinterpret_cast<float4*>(theta + c.base + e) = t[u];
        }
    }
}

// the variables [s0, s1) whose slots are exactly [lo, hi); false: not a range of whole variables
static bool lamb_find_range(const unetrir_lamb_seg* segs, int n_seg, long long lo, long long hi, int* s0, int* s1) {
    int a = -1, b = -1;
    for (int i = 0; i < n_seg; ++i) {
        if (segs[i].offset == lo) a = i;
        if (segs[i].offset + segs[i].slot == hi) b = i + 1;
    }
    if (a < 0 || b <= a) return false;
    *s0 = a; *s1 = b;
    return true;
}

static int lamb_launch(float* theta, const float* g, float* m, float* v, const unetrir_lamb_seg* segs_host, const unetrir_lamb_seg* segs,
                       const int* chunk_seg, int n_seg, long long lo, long long hi, LambHyper h, const unsigned long long* state,
                       const float* cfg, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!theta || !g || !m || !v || !segs_host || !segs || !chunk_seg || !ws || n_seg <= 0) return UNETRIR_EINVAL;
    if (((uintptr_t)theta | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15 || ((uintptr_t)ws & 7)) return UNETRIR_EINVAL;
    int s0, s1;
    if (!lamb_find_range(segs_host, n_seg, lo, hi, &s0, &s1)) return UNETRIR_EINVAL;
    const long long n_chunks = segs_host[n_seg - 1].chunk0 + lamb_chunks_of(segs_host[n_seg - 1].count);
    if (ws_bytes < unetrir_lamb_ws_bytes(n_seg, n_chunks)) return UNETRIR_EINVAL;
    const int c0 = segs_host[s0].chunk0;
    const int c1 = (int)(segs_host[s1 - 1].chunk0 + lamb_chunks_of(segs_host[s1 - 1].count));
    double* part = (double*)ws;
    float* ratio = (float*)((char*)ws + 16 * (size_t)n_chunks);
    hipLaunchKernelGGL(lamb_moments_kernel, dim3(c1 - c0), dim3(LAMB_T), 0, s, theta, g, m, v, segs, chunk_seg, c0, h, state, cfg, part);
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3(s1 - s0), dim3(LAMB_T), 0, s, segs, s0, part, ratio);
    hipLaunchKernelGGL(lamb_apply_kernel, dim3(c1 - c0), dim3(LAMB_T), 0, s, theta, m, v, segs, chunk_seg, c0, h, state, cfg, ratio);
    return (int)hipGetLastError();
}

extern "C" {

int unetrir_lamb_chunk_elems(void) { return LAMB_CHUNK; }

long long unetrir_lamb_table_init(unetrir_lamb_seg* segs, int n_seg, int32_t* chunk_seg, long long chunk_cap) {
    if (!segs || n_seg <= 0) return -1;
    long long n = 0;
    for (int i = 0; i < n_seg; ++i) {
        unetrir_lamb_seg& s = segs[i];
        if (s.offset < 0 || (s.offset & 3) || s.slot <= 0 || (s.slot & 3) || s.count <= 0 || s.count > s.slot) return -1;
        if (i && s.offset != segs[i - 1].offset + segs[i - 1].slot) return -1;
        if (s.flags & ~(UNETRIR_LAMB_DECAY | UNETRIR_LAMB_ADAPT)) return -1;
        const long long c = lamb_chunks_of(s.count);
        if (n + c > 0x7FFFFFFFll) return -1;
        s.chunk0 = (int)n;
        if (chunk_seg) {
            if (n + c > chunk_cap) return -1;
            for (long long k = 0; k < c; ++k) chunk_seg[n + k] = i;
        }
        n += c;
    }
    return n;
}

size_t unetrir_lamb_ws_bytes(int n_seg, long long n_chunks) {
    if (n_seg <= 0 || n_chunks <= 0) return 0;
    return 16 * (size_t)n_chunks + 4 * (size_t)n_seg;
}

int unetrir_lamb_f32(float* theta, const float* g, float* m, float* v, const unetrir_lamb_seg* segs_host, const unetrir_lamb_seg* segs,
                     const int32_t* chunk_seg, int n_seg, long long lo, long long hi, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float corr1, float corr2, float grad_scale, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    const LambHyper h = {lr, beta1, beta2, eps, weight_decay, corr1, corr2, grad_scale};
    return lamb_launch(theta, g, m, v, segs_host, segs, chunk_seg, n_seg, lo, hi, h, nullptr, nullptr, ws, ws_bytes, (hipStream_t)stream);
}

int unetrir_lamb_dev_f32(float* theta, const float* g, float* m, float* v, const unetrir_lamb_seg* segs_host, const unetrir_lamb_seg* segs,
                         const int32_t* chunk_seg, int n_seg, long long lo, long long hi, float weight_decay,
                         const unsigned long long* state, const float* cfg, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!state || !cfg) return UNETRIR_EINVAL;
    const LambHyper h = {0.f, 0.f, 0.f, 0.f, weight_decay, 1.f, 1.f, 0.f};
    return lamb_launch(theta, g, m, v, segs_host, segs, chunk_seg, n_seg, lo, hi, h, state, cfg, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
