// head1x1.hip - the output head Conv2D(2, (1, 1), activation='linear') of dl_models/diff_u_net.py:247 on a bf16 trunk, as streaming
// kernels: a C-to-2 dot product per pixel is memory bound, so the forward pass is one sweep over the activations and the whole
// backward pass - data gradient, weight gradient, bias gradient - a second one.
//
// A pixel's C bf16 channels are C / 8 16-byte vectors.  G = the power of two >= C / 8 consecutive lanes share a pixel, one vector
// each (lanes beyond C / 8 idle: only where C / 8 is no power of two), so a wave's loads and stores are consecutive 16-byte units;
// each lane keeps its 8 columns of the two kernel rows (rounded to bf16, as the generic path's work copy is) in registers for the
// whole launch.  A workgroup owns a contiguous range of pixels whose length depends on the pixel count alone.
//
// No float atomics: the backward kernel sums its lanes' partial dw / dbias over the wave by a butterfly (an order fixed by the lane
// numbers), over its waves through LDS in wave order, and stores one slab [2][C] dw, dbias[2] to the workspace; a second launch sums
// the slabs in a fixed order: 64 runs of consecutive slabs, each in index order, then the 64 run sums in run order.  Nothing here
// depends on the device, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

#define H1_THREADS 256
#define H1_WAVES (H1_THREADS / 64)
#define H1_FWD_MAX_WG 2048        // workgroups of the forward pass at most
#define H1_BWD_MAX_WG 1024        // workgroups (= slabs) of the backward pass at most
#define H1_MIN_CHUNK 256          // pixels a workgroup owns at least
#define H1_FIN_PARTS 64           // the slab sum: 64 runs of consecutive slabs per element (16 slabs each at most), combined in run order
#define H1_FIN_ELEMS 4            // ... 4 elements per workgroup of 256 threads: the slab reads are latency, so they are spread wide
#define H1_FIN_BATCH 8            // ... and issued 8 at a time

typedef __bf16 bf16x8_1 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_1 __attribute__((ext_vector_type(2)));

namespace {

inline long long h1_chunk(long long P, int max_wg) {
    const long long c = (P + max_wg - 1) / max_wg;
    return c < H1_MIN_CHUNK ? H1_MIN_CHUNK : c;
}
inline int h1_nwg(long long P, int max_wg) { return (int)((P + h1_chunk(P, max_wg) - 1) / h1_chunk(P, max_wg)); }
inline int h1_slab(int C) { return 2 * C + 8; }           // floats per slab: dw[2][C], dbias[2], padding to 16 bytes
inline bool h1_c_ok(int C) { return C >= 8 && C <= 256 && (C % 8) == 0; }
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

__device__ __forceinline__ float h1_round_bf16(float v) { return (float)(__bf16)v; }

// this lane's 8 columns of the two kernel rows, rounded to bf16 (zeros for an idle lane)
__device__ __forceinline__ void h1_load_w(const float* __restrict__ w, int C, int v, bool live, float (&w0)[8], float (&w1)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        w0[k] = live ? h1_round_bf16(w[v * 8 + k]) : 0.f;
        w1[k] = live ? h1_round_bf16(w[C + v * 8 + k]) : 0.f;
    }
}

// forward: y[p][0..1] = bias + sum_c x[p][c] * w[0..1][c]; y[p][2..3] = 0
template <int G>
__global__ __launch_bounds__(H1_THREADS) void head1x1_fwd_kernel(const __bf16* __restrict__ x, int ldx, long long P, long long chunk, int C,
                                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                                 float* __restrict__ y, int ldy) {
    constexpr int PPI = H1_THREADS / G;          // pixels per iteration
    const int v = threadIdx.x % G, slot = threadIdx.x / G;
    const bool live = v * 8 < C;
    float w0[8], w1[8];
    h1_load_w(w, C, v, live, w0, w1);
    const float b0 = bias[0], b1 = bias[1];
    const long long p0 = (long long)blockIdx.x * chunk;
    const long long p1 = (p0 + chunk < P) ? p0 + chunk : P;
#pragma unroll 2
    for (long long pb = p0; pb < p1; pb += PPI) {
        const long long p = pb + slot;
        float a0 = 0.f, a1 = 0.f;
        if (live && p < p1) {
            const bf16x8_1 xv = *reinterpret_cast<const bf16x8_1*>(x + (size_t)p * ldx + v * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xf = (float)xv[k];
                a0 += xf * w0[k];
                a1 += xf * w1[k];
            }
        }
#pragma unroll
        for (int off = 1; off < G; off <<= 1) {
            a0 += __shfl_xor(a0, off);
            a1 += __shfl_xor(a1, off);
        }
        if (v == 0 && p < p1) {
            float* yp = y + (size_t)p * ldy;
            if ((ldy & 3) == 0) {
                *reinterpret_cast<float4*>(yp) = make_float4(a0 + b0, a1 + b1, 0.f, 0.f);
            } else {
                yp[0] = a0 + b0; yp[1] = a1 + b1; yp[2] = 0.f; yp[3] = 0.f;
            }
        }
    }
}

// backward: dx[p][c] = dy[p][0] w[0][c] + dy[p][1] w[1][c] (bf16, first writer); slab[blockIdx.x] = the block's sums of
// dy[p][j] x[p][c] and dy[p][j]
template <int G>
__global__ __launch_bounds__(H1_THREADS) void head1x1_bwd_kernel(const __bf16* __restrict__ x, int ldx, const __bf16* __restrict__ dy, int lddy,
                                                                 long long P, long long chunk, int C, const float* __restrict__ w,
                                                                 __bf16* __restrict__ dx, int lddx, float* __restrict__ ws, int slab) {
    constexpr int PPI = H1_THREADS / G;
    __shared__ float red[H1_WAVES][G][18];
    const int v = threadIdx.x % G, slot = threadIdx.x / G;
    const bool live = v * 8 < C;
    float w0[8], w1[8];
    h1_load_w(w, C, v, live, w0, w1);
    float s0[8], s1[8], d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s0[k] = s1[k] = 0.f;
    const long long p0 = (long long)blockIdx.x * chunk;
    const long long p1 = (p0 + chunk < P) ? p0 + chunk : P;
    const bool dy_pair = (lddy & 1) == 0;        // an even pixel stride: both channels in one 4-byte load
#pragma unroll 2
    for (long long pb = p0; pb < p1; pb += PPI) {
        const long long p = pb + slot;
        if (live && p < p1) {
            const __bf16* dp = dy + (size_t)p * lddy;
            float g0, g1;
            if (dy_pair) {
                const bf16x2_1 gv = *reinterpret_cast<const bf16x2_1*>(dp);
                g0 = (float)gv[0]; g1 = (float)gv[1];
            } else {
                g0 = (float)dp[0]; g1 = (float)dp[1];
            }
            const bf16x8_1 xv = *reinterpret_cast<const bf16x8_1*>(x + (size_t)p * ldx + v * 8);
            bf16x8_1 o;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float xf = (float)xv[k];
                o[k] = (__bf16)(g0 * w0[k] + g1 * w1[k]);
                s0[k] += g0 * xf;
                s1[k] += g1 * xf;
            }
            *reinterpret_cast<bf16x8_1*>(dx + (size_t)p * lddx + v * 8) = o;
            d0 += g0; d1 += g1;
        }
    }
    // the lanes that hold the same vector v: lane numbers v + G * i.  Butterfly over i, then the waves in order through LDS.
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s0[k] += __shfl_xor(s0[k], off);
            s1[k] += __shfl_xor(s1[k], off);
        }
        d0 += __shfl_xor(d0, off);
        d1 += __shfl_xor(d1, off);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < G) {            // lane == v here
#pragma unroll
        for (int k = 0; k < 8; ++k) { red[wave][lane][k] = s0[k]; red[wave][lane][8 + k] = s1[k]; }
        red[wave][lane][16] = d0; red[wave][lane][17] = d1;
    }
    __syncthreads();
    float* out = ws + (size_t)blockIdx.x * slab;
    for (int e = threadIdx.x; e < 2 * C + 2; e += H1_THREADS) {
        int vv, kk;
        if (e < 2 * C) {
            const int j = e / C, c = e - j * C;
            vv = c >> 3; kk = j * 8 + (c & 7);
        } else {
            vv = 0; kk = 16 + (e - 2 * C);
        }
        float s = red[0][vv][kk];
#pragma unroll
        for (int wv = 1; wv < H1_WAVES; ++wv) s += red[wv][vv][kk];
        out[e] = s;
    }
}

// dw[0..2C) and dbias[0..2) = the sum of the slabs in a fixed order: 64 runs of consecutive slabs, each summed in index order, then
// the 64 run sums in run order (not one sequential pass over the slabs: that is 1024 dependent additions in a single workgroup)
__global__ __launch_bounds__(H1_FIN_ELEMS * H1_FIN_PARTS) void head1x1_finalize_kernel(const float* __restrict__ ws, int nslab, int slab, int C,
                                                                                        float* __restrict__ dw, float* __restrict__ dbias) {
    __shared__ float red[H1_FIN_PARTS][H1_FIN_ELEMS];
    const int el = threadIdx.x % H1_FIN_ELEMS, part = threadIdx.x / H1_FIN_ELEMS;
    const int e = blockIdx.x * H1_FIN_ELEMS + el, n = 2 * C + 2;
    const int per = (nslab + H1_FIN_PARTS - 1) / H1_FIN_PARTS;
    const int lo = part * per, hi = (lo + per < nslab) ? lo + per : nslab;
    float s = 0.f;
    if (e < n) {
        for (int i0 = lo; i0 < hi; i0 += H1_FIN_BATCH) {
            float v[H1_FIN_BATCH];
#pragma unroll
            for (int j = 0; j < H1_FIN_BATCH; ++j) v[j] = (i0 + j < hi) ? ws[(size_t)(i0 + j) * slab + e] : 0.f;
#pragma unroll
            for (int j = 0; j < H1_FIN_BATCH; ++j) s += v[j];          // slabs beyond the run add an exact 0
        }
    }
    red[part][el] = s;
    __syncthreads();
    if (part == 0 && e < n) {
        float t = red[0][el];
#pragma unroll
        for (int q = 1; q < H1_FIN_PARTS; ++q) t += red[q][el];
        if (e < 2 * C) dw[e] = t;
        else dbias[e - 2 * C] = t;
    }
}

namespace {

template <int G>
void h1_launch_fwd(const __bf16* x, int ldx, long long P, int C, const float* w, const float* bias, float* y, int ldy, hipStream_t s) {
    hipLaunchKernelGGL(head1x1_fwd_kernel<G>, dim3(h1_nwg(P, H1_FWD_MAX_WG)), dim3(H1_THREADS), 0, s, x, ldx, P, h1_chunk(P, H1_FWD_MAX_WG), C, w, bias, y, ldy);
}

template <int G>
void h1_launch_bwd(const __bf16* x, int ldx, const __bf16* dy, int lddy, long long P, int C, const float* w, __bf16* dx, int lddx, float* ws,
                   hipStream_t s) {
    hipLaunchKernelGGL(head1x1_bwd_kernel<G>, dim3(h1_nwg(P, H1_BWD_MAX_WG)), dim3(H1_THREADS), 0, s, x, ldx, dy, lddy, P, h1_chunk(P, H1_BWD_MAX_WG), C, w, dx, lddx, ws,
                       h1_slab(C));
}

}  // namespace

extern "C" {

/* The passes offered: 1 forward, 2 backward.  Decided by the measured record (profiles/diffunet.json, scripts/time_diffunet.py): a pass
 * is offered only if it is no slower than the generic path at the default head (144 x 160, batch 32, C = 32).  There: forward 14.0-14.6 us
 * against 33.8-34.6 us, backward 27.4-27.5 us against 84.6-84.8 us (data gradient + weight gradient + colsum): both stay. */
int unetrir_head1x1_supported(int C) { return h1_c_ok(C) ? 3 : 0; }

int unetrir_head1x1_fwd_bf16(const unetrir_bf16* x, int ldx, int B, int H, int W, int C, const float* w, const float* bias, float* y, int ldy,
                             unetrir_stream_t stream) {
    if (!x || !w || !bias || !y || B <= 0 || H <= 0 || W <= 0 || !h1_c_ok(C) || ldx < C || (ldx & 7) || ldy < 4 || !al16(x) || !al16(w) ||
        !al16(bias) || !al16(y))
        return UNETRIR_EINVAL;
    const long long P = (long long)B * H * W;
    const __bf16* xh = (const __bf16*)x;
    const hipStream_t s = (hipStream_t)stream;
    const int V = C / 8;
    if (V <= 1) h1_launch_fwd<1>(xh, ldx, P, C, w, bias, y, ldy, s);
    else if (V <= 2) h1_launch_fwd<2>(xh, ldx, P, C, w, bias, y, ldy, s);
    else if (V <= 4) h1_launch_fwd<4>(xh, ldx, P, C, w, bias, y, ldy, s);
    else if (V <= 8) h1_launch_fwd<8>(xh, ldx, P, C, w, bias, y, ldy, s);
    else if (V <= 16) h1_launch_fwd<16>(xh, ldx, P, C, w, bias, y, ldy, s);
    else h1_launch_fwd<32>(xh, ldx, P, C, w, bias, y, ldy, s);
    return (int)hipGetLastError();
}

size_t unetrir_head1x1_bwd_ws_bytes(int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || !h1_c_ok(C)) return 0;
    return (size_t)h1_nwg((long long)B * H * W, H1_BWD_MAX_WG) * h1_slab(C) * sizeof(float);
}

int unetrir_head1x1_bwd_bf16(const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy, int B, int H, int W, int C, const float* w,
                             unetrir_bf16* dx, int lddx, float* dw, float* dbias, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!x || !dy || !w || !dx || !dw || !dbias || !ws || B <= 0 || H <= 0 || W <= 0 || !h1_c_ok(C) || ldx < C || (ldx & 7) || lddx < C ||
        (lddx & 7) || lddy < 8 || !al16(x) || !al16(dy) || !al16(w) || !al16(dx) || !al16(dw) || !al16(dbias) || !al16(ws) ||
        ws_bytes < unetrir_head1x1_bwd_ws_bytes(B, H, W, C))
        return UNETRIR_EINVAL;
    const long long P = (long long)B * H * W;
    const __bf16 *xh = (const __bf16*)x, *dyh = (const __bf16*)dy;
    __bf16* dxh = (__bf16*)dx;
    const hipStream_t s = (hipStream_t)stream;
    const int V = C / 8;
    if (V <= 1) h1_launch_bwd<1>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    else if (V <= 2) h1_launch_bwd<2>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    else if (V <= 4) h1_launch_bwd<4>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    else if (V <= 8) h1_launch_bwd<8>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    else if (V <= 16) h1_launch_bwd<16>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    else h1_launch_bwd<32>(xh, ldx, dyh, lddy, P, C, w, dxh, lddx, (float*)ws, s);
    int err = (int)hipGetLastError();
    if (err) return err;
    hipLaunchKernelGGL(head1x1_finalize_kernel, dim3((2 * C + 2 + H1_FIN_ELEMS - 1) / H1_FIN_ELEMS), dim3(H1_FIN_ELEMS * H1_FIN_PARTS), 0, s,
                       (const float*)ws, h1_nwg(P, H1_BWD_MAX_WG), h1_slab(C), C, dw, dbias);
    return (int)hipGetLastError();
}

}  // extern "C"
