// head_up2.hip - UpSampling2D((2, 2)) -> Conv2D(2, (6,6), padding='same') (dl_models/u_net.py:247-248, resize_factor_0 = [2, 2])
// without the up-sampled tensor.  Nearest-neighbour x2 followed by the 6x6 'same' convolution is a 4x4 'same' convolution
// (pad 1 before, 2 after) with 8 output channels (o, a, b) on the coarse grid followed by depth-to-space:
//     logit[o, 2i+a, 2j+b] = bias[o] + sum_{u,v,c} K'[(o,a,b),u,v,c] * x[i+u-1, j+v-1, c]
//     K'[(o,a,b),u,v,c]    = sum_{dh: (a+dh)>>1 == u} sum_{dw: (b+dw)>>1 == v} K[o,dh,dw,c]          ("fold")
// The folded kernel K' [8][4][4][C] is a work copy of the [PAD][6][6][C] master (fp32; for a bf16 trunk its values are rounded to
// bf16 once, after the fp32 sum); taps (a = 0, u = 3) and (b = 0, v = 3) are identically zero and are skipped.  Direct (non-MFMA)
// kernels in the style of head.hip: a lane owns one coarse pixel (forward, data gradient) or one (tap, channel) pair (weight
// gradient), the weights are wave-uniform scalar loads, and the depth-to-space / space-to-depth lives in the fine-grid addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "kernels.h"

#define UT 16                 // coarse tile edge
#define UK 4                  // folded kernel size
#define UP (UT + UK - 1)      // 19: patch edge
#define UPAD_T 1              // coarse padding (1, 2)
#define UJ 8                  // folded output channels (o, a, b)
#define UDS 12                // floats per pixel of the staged dlogits patch (8 used; 48-byte stride keeps 16-byte reads conflict-free)
#define UP2_WGRAD_BLOCKS 256

typedef __bf16 bf16x4_u __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_u __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8_u __attribute__((ext_vector_type(8)));
__device__ __forceinline__ float4 ld4u(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4u(const __bf16* p) {
    const bf16x4_u v = *reinterpret_cast<const bf16x4_u*>(p);
    return make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
}
__device__ __forceinline__ float2 ld2u(const float* p) { return *reinterpret_cast<const float2*>(p); }
__device__ __forceinline__ float2 ld2u(const __bf16* p) {
    const bf16x2_u v = *reinterpret_cast<const bf16x2_u*>(p);
    return make_float2((float)v[0], (float)v[1]);
}
__device__ __forceinline__ void st8u(float* p, const float* a) {
    *reinterpret_cast<float4*>(p) = make_float4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(a[4], a[5], a[6], a[7]);
}
__device__ __forceinline__ void st8u(__bf16* p, const float* a) {
    bf16x8_u v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (__bf16)a[i];          // one rounding, to nearest even
    *reinterpret_cast<bf16x8_u*>(p) = v;
}

// fold: one thread per element of K'; the sum runs dh outer, dw inner, both ascending, in fp32
__global__ __launch_bounds__(256) void up2_fold_kernel(const float* __restrict__ w, int C, float* __restrict__ wf, int round_bf16) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= UJ * UK * UK * C) return;
    const int c = idx % C, t = idx / C;
    const int v = t % UK, u = (t / UK) % UK, j = t / (UK * UK);
    const int o = j >> 2, a = (j >> 1) & 1, b = j & 1;
    float s = 0.f;
    for (int dh = 0; dh < 6; ++dh) {
        if (((a + dh) >> 1) != u) continue;
        for (int dw = 0; dw < 6; ++dw)
            if (((b + dw) >> 1) == v) s += w[((size_t)(o * 6 + dh) * 6 + dw) * C + c];
    }
    wf[idx] = round_bf16 ? (float)(__bf16)s : s;
}

// unfold (the transpose of fold): dK[o,dh,dw,c] = sum_{a,b} dK'[(o,a,b), (a+dh)>>1, (b+dw)>>1, c], a outer, b inner; rows o >= 2 of the
// padded master gradient are not written
__global__ __launch_bounds__(256) void up2_unfold_kernel(const float* __restrict__ dwf, int C, float* __restrict__ dw) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 2 * 36 * C) return;
    const int c = idx % C, t = idx / C;
    const int kw = t % 6, kh = (t / 6) % 6, o = t / 36;
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
            s += dwf[((size_t)((o * 4 + a * 2 + b) * UK + ((a + kh) >> 1)) * UK + ((b + kw) >> 1)) * C + c];
    dw[idx] = s;
}

// stage channels [c0, c0+CC) of the coarse patch around tile (ty0, tx0) of image n into LDS, zero outside the image
template <int CC, typename T>
__device__ __forceinline__ void up2_load_patch(const T* __restrict__ x, int ldx, int h, int w, int n, int ty0, int tx0, int c0,
                                               float* __restrict__ As) {
    constexpr int Q = CC / 4, LD = CC + 4;
    for (int i = threadIdx.x; i < UP * UP * Q; i += 256) {
        const int pix = i / Q, q = i - pix * Q;
        const int py = pix / UP, px = pix - py * UP;
        const int iy = ty0 + py - UPAD_T, ix = tx0 + px - UPAD_T;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w)
            v = ld4u(x + ((size_t)((long long)n * h + iy) * w + ix) * ldx + c0 + q * 4);
        *reinterpret_cast<float4*>(&As[pix * LD + q * 4]) = v;
    }
}

__device__ __forceinline__ void ld8u(const float* p, float* a) {
    const float4 v0 = *reinterpret_cast<const float4*>(p), v1 = *reinterpret_cast<const float4*>(p + 4);
    a[0] = v0.x; a[1] = v0.y; a[2] = v0.z; a[3] = v0.w; a[4] = v1.x; a[5] = v1.y; a[6] = v1.z; a[7] = v1.w;
}
__device__ __forceinline__ void ld8u(const __bf16* p, float* a) {
    const bf16x8_u v = *reinterpret_cast<const bf16x8_u*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (float)v[i];
}

// forward: a lane owns coarse pixel (i, j) of a 16 x 16 tile and its 2x2 fine pixels x 2 channels.  Per 8 channels the 19 x 19 patch
// is staged in LDS (zero outside the image), the lane takes its 4x4 neighbourhood into registers, and the inner loop is scalar weight
// loads (8 channels of one folded tap each) and FMAs alone - the shape of the data-gradient kernel; with LDS reads inside that loop
// they and the scalar loads wait on one counter.  y is the fine grid [B][2h][2w][ldy] as head6x6_fwd writes it (channels 2.. zeroed
// up to 4).
template <typename T>
__global__ __launch_bounds__(256) void up2_fwd_kernel(const T* __restrict__ x, int ldx, int B, int h, int w, int C,
                                                      const float* __restrict__ wf, const float* __restrict__ bias,
                                                      float* __restrict__ y, int ldy) {
    __shared__ __attribute__((aligned(16))) float As[UP * UP * UDS];
    const int tilesx = (w + UT - 1) / UT, tilesy = (h + UT - 1) / UT;
    int bid = blockIdx.x;
    const int n = bid / (tilesx * tilesy);
    bid -= n * tilesx * tilesy;
    const int ty0 = (bid / tilesx) * UT, tx0 = (bid % tilesx) * UT;
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    float acc[UJ];
#pragma unroll
    for (int j = 0; j < UJ; ++j) acc[j] = 0.f;
    const int ldw = UK * UK * C;
    const T* xn = x + (size_t)n * h * w * ldx;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += 8) {
        if (c0) __syncthreads();
        for (int i = threadIdx.x; i < UP * UP; i += 256) {
            const int py = i / UP, px = i - py * UP;
            const int iy = ty0 + py - UPAD_T, ix = tx0 + px - UPAD_T;
            float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w) ld8u(xn + ((size_t)iy * w + ix) * ldx + c0, v);
            st8u(&As[i * UDS], v);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UK; ++u) {
#pragma unroll
            for (int v = 0; v < UK; ++v) {
                const float* ap = &As[((ly + u) * UP + lx + v) * UDS];
                const float4 a0 = *reinterpret_cast<const float4*>(ap), a1 = *reinterpret_cast<const float4*>(ap + 4);
                const float a[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                const float* wp = wf + (u * UK + v) * C + c0;          // uniform address -> scalar loads, 8 channels each
#pragma unroll
                for (int j = 0; j < UJ; ++j) {
                    if ((!(j & 1) && v == 3) || (!(j & 2) && u == 3)) continue;      // b = 0 / a = 0 have taps 0..2
                    const float* wj = wp + j * ldw;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j] += a[e] * wj[e];
                }
            }
        }
    }
    const int oy = ty0 + ly, ox = tx0 + lx;
    if (oy >= h || ox >= w) return;
    const float b0 = bias ? bias[0] : 0.f, b1 = bias ? bias[1] : 0.f;
    const int W = 2 * w;
#pragma unroll
    for (int a = 0; a < 2; ++a) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const size_t px = ((size_t)((long long)n * 2 * h + 2 * oy + a)) * W + 2 * ox + b;
            const float v0 = acc[a * 2 + b] + b0, v1 = acc[4 + a * 2 + b] + b1;
            if (ldy >= 4) {
                *reinterpret_cast<float4*>(y + px * ldy) = make_float4(v0, v1, 0.f, 0.f);
            } else {
                y[px * ldy] = v0;
                y[px * ldy + 1] = v1;
            }
        }
    }
}

// data gradient: dx[i,j,c] = sum_{o,a,b,u,v} K'[(o,a,b),u,v,c] * dy[o, 2(i-u+1)+a, 2(j-v+1)+b].  The dlogits of the 19x19 coarse
// pixels around the tile are staged once as [pixel][(o,a,b)]; a lane owns one coarse pixel and walks the channels 8 at a time.
template <typename T>
__global__ __launch_bounds__(256) void up2_dgrad_kernel(const T* __restrict__ dy, int lddy, int B, int h, int w,
                                                        const float* __restrict__ wf, int C, T* __restrict__ dx, int lddx) {
    __shared__ __attribute__((aligned(16))) float Ds[UP * UP * UDS];
    const int tilesx = (w + UT - 1) / UT, tilesy = (h + UT - 1) / UT;
    int bid = blockIdx.x;
    const int n = bid / (tilesx * tilesy);
    bid -= n * tilesx * tilesy;
    const int ty0 = (bid / tilesx) * UT, tx0 = (bid % tilesx) * UT;
    const int W = 2 * w;
    // patch pixel (py, px) is coarse pixel (ty0 + py - 2, tx0 + px - 2): tap u of output row ly reads patch row ly + 3 - u
    for (int i = threadIdx.x; i < UP * UP * 4; i += 256) {
        const int pix = i >> 2, a = (i >> 1) & 1, b = i & 1;
        const int py = pix / UP, px = pix - py * UP;
        const int iy = ty0 + py - 2, ix = tx0 + px - 2;
        float2 d = make_float2(0.f, 0.f);
        if ((unsigned)iy < (unsigned)h && (unsigned)ix < (unsigned)w)
            d = ld2u(dy + (((size_t)((long long)n * 2 * h + 2 * iy + a)) * W + 2 * ix + b) * lddy);
        Ds[pix * UDS + a * 2 + b] = d.x;
        Ds[pix * UDS + 4 + a * 2 + b] = d.y;
    }
    __syncthreads();
    const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
    const int oy = ty0 + ly, ox = tx0 + lx;
    if (oy >= h || ox >= w) return;
    const int ldw = UK * UK * C;
    T* out = dx + ((size_t)((long long)n * h + oy) * w + ox) * lddx;
#pragma unroll 1
    for (int c0 = 0; c0 < C; c0 += 8) {
        float acc[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
#pragma unroll
        for (int u = 0; u < UK; ++u) {
#pragma unroll
            for (int v = 0; v < UK; ++v) {
                const float* dp = &Ds[((ly + 3 - u) * UP + lx + 3 - v) * UDS];
                const float4 d0 = *reinterpret_cast<const float4*>(dp), d1 = *reinterpret_cast<const float4*>(dp + 4);
                const float d[UJ] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
                const float* wp = wf + (u * UK + v) * C + c0;          // uniform address -> scalar loads
#pragma unroll
                for (int j = 0; j < UJ; ++j) {
                    if ((!(j & 1) && v == 3) || (!(j & 2) && u == 3)) continue;
                    const float* wj = wp + j * ldw;
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += d[j] * wj[e];
                }
            }
        }
        st8u(out + c0, acc);
    }
}

// weight gradient of the folded kernel: part[blk][(o,a,b)][tap][c] = sum over the block's tiles of dy[o, 2i+a, 2j+b] * x[(i,j) + off_tap][c]
// thread = (channel c in the CC-chunk, tap group g); tap t belongs to group t % NG
template <int CC, typename T>
__global__ __launch_bounds__(256) void up2_wgrad_kernel(const T* __restrict__ x, int ldx, int B, int h, int w, int C,
                                                        const T* __restrict__ dy, int lddy, float* __restrict__ part, int ntiles_total) {
    constexpr int LD = CC + 4, NG = 256 / CC, NT = UK * UK, TPG = (NT + NG - 1) / NG;
    __shared__ __attribute__((aligned(16))) float As[UP * UP * LD];
    __shared__ __attribute__((aligned(16))) float Ds[UT * UT * UJ];
    const int c0 = blockIdx.y * CC;
    const int cl = threadIdx.x % CC, g = threadIdx.x / CC;
    const int tilesx = (w + UT - 1) / UT, tilesy = (h + UT - 1) / UT;
    const int W = 2 * w;
    float acc[TPG][UJ];
    int base[TPG];
#pragma unroll
    for (int i = 0; i < TPG; ++i) {
#pragma unroll
        for (int j = 0; j < UJ; ++j) acc[i][j] = 0.f;
        const int t = g + i * NG;                    // taps beyond 15 read in-bounds values and are never stored
        base[i] = (t < NT) ? ((t / UK) * UP + (t % UK)) * LD + cl : cl;
    }
    for (int tile = blockIdx.x; tile < ntiles_total; tile += gridDim.x) {
        const int n = tile / (tilesx * tilesy);
        const int r = tile - n * tilesx * tilesy;
        const int ty0 = (r / tilesx) * UT, tx0 = (r % tilesx) * UT;
        __syncthreads();
        up2_load_patch<CC, T>(x, ldx, h, w, n, ty0, tx0, c0, As);
        {
            const int ly = threadIdx.x >> 4, lx = threadIdx.x & 15;
            const int oy = ty0 + ly, ox = tx0 + lx;
            const bool in = oy < h && ox < w;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float2 d = make_float2(0.f, 0.f);
                    if (in) d = ld2u(dy + (((size_t)((long long)n * 2 * h + 2 * oy + a)) * W + 2 * ox + b) * lddy);
                    Ds[threadIdx.x * UJ + a * 2 + b] = d.x;
                    Ds[threadIdx.x * UJ + 4 + a * 2 + b] = d.y;
                }
            }
        }
        __syncthreads();
        for (int ly = 0; ly < UT; ++ly) {
#pragma unroll 4
            for (int lx = 0; lx < UT; ++lx) {
                const float* dp = &Ds[(ly * UT + lx) * UJ];                  // same address in every lane: LDS broadcast
                const float4 d0 = *reinterpret_cast<const float4*>(dp), d1 = *reinterpret_cast<const float4*>(dp + 4);
                const int off = (ly * UP + lx) * LD;
#pragma unroll
                for (int i = 0; i < TPG; ++i) {
                    const float a = As[base[i] + off];
                    acc[i][0] += d0.x * a; acc[i][1] += d0.y * a; acc[i][2] += d0.z * a; acc[i][3] += d0.w * a;
                    acc[i][4] += d1.x * a; acc[i][5] += d1.y * a; acc[i][6] += d1.z * a; acc[i][7] += d1.w * a;
                }
            }
        }
    }
    float* out = part + (size_t)blockIdx.x * UJ * NT * C;
#pragma unroll
    for (int i = 0; i < TPG; ++i) {
        const int t = g + i * NG;
        if (t < NT) {
#pragma unroll
            for (int j = 0; j < UJ; ++j) out[(size_t)(j * NT + t) * C + c0 + cl] = acc[i][j];
        }
    }
}

namespace {

inline bool up2_c_ok(int C) { return C > 0 && (C % 8) == 0; }

inline long long up2_tiles(int B, int h, int w) { return (long long)B * ((h + UT - 1) / UT) * ((w + UT - 1) / UT); }

inline int up2_wgrad_blocks(int B, int h, int w) {
    const long long tiles = up2_tiles(B, h, w);
    return tiles < UP2_WGRAD_BLOCKS ? (int)tiles : UP2_WGRAD_BLOCKS;
}

size_t up2_wgrad_ws(int B, int h, int w, int C) {
    if (B <= 0 || h <= 0 || w <= 0 || !up2_c_ok(C) || up2_tiles(B, h, w) > 0x7fffffffLL) return 0;
    return ((size_t)up2_wgrad_blocks(B, h, w) + 1) * UJ * UK * UK * C * sizeof(float);      // the slabs, then the folded gradient
}

template <typename T>
int up2_fwd_impl(const T* x, int ldx, int B, int h, int w, int C, const float* wf, const float* bias, float* y, int ldy, hipStream_t s) {
    constexpr int G = 16 / (int)sizeof(T);
    if (!x || !wf || !y || B <= 0 || h <= 0 || w <= 0 || !up2_c_ok(C) || ldx < C || (ldx % G) || ldy < 2 || (ldy >= 4 && (ldy & 3)) ||
        ((uintptr_t)x & 15) || ((uintptr_t)wf & 15) || ((uintptr_t)y & (ldy >= 4 ? 15 : 3)) || ((uintptr_t)bias & 3) ||
        up2_tiles(B, h, w) > 0x7fffffffLL)
        return UNETRIR_EINVAL;
    hipLaunchKernelGGL((up2_fwd_kernel<T>), dim3((unsigned)up2_tiles(B, h, w)), dim3(256), 0, s, x, ldx, B, h, w, C, wf, bias, y, ldy);
    return (int)hipGetLastError();
}

template <typename T>
int up2_dgrad_impl(const T* dy, int lddy, int B, int h, int w, const float* wf, int C, T* dx, int lddx, hipStream_t s) {
    constexpr int G = 16 / (int)sizeof(T);
    if (!dy || !wf || !dx || B <= 0 || h <= 0 || w <= 0 || !up2_c_ok(C) || lddy < 2 || (lddy & 1) || lddx < C || (lddx % G) ||
        ((uintptr_t)dy & (2 * sizeof(T) - 1)) || ((uintptr_t)wf & 15) || ((uintptr_t)dx & 15) || up2_tiles(B, h, w) > 0x7fffffffLL)
        return UNETRIR_EINVAL;
    hipLaunchKernelGGL((up2_dgrad_kernel<T>), dim3((unsigned)up2_tiles(B, h, w)), dim3(256), 0, s, dy, lddy, B, h, w, wf, C, dx, lddx);
    return (int)hipGetLastError();
}

template <typename T>
int up2_wgrad_impl(const T* x, int ldx, int B, int h, int w, int C, const T* dy, int lddy, float* dw, void* ws, size_t ws_bytes,
                   hipStream_t s) {
    constexpr int G = 16 / (int)sizeof(T);
    const size_t need = up2_wgrad_ws(B, h, w, C);
    if (!x || !dy || !dw || !ws || need == 0 || ws_bytes < need || ldx < C || (ldx % G) || lddy < 2 || (lddy & 1) ||
        ((uintptr_t)x & 15) || ((uintptr_t)dy & (2 * sizeof(T) - 1)) || ((uintptr_t)dw & 15) || ((uintptr_t)ws & 15))
        return UNETRIR_EINVAL;
    const int tiles = (int)up2_tiles(B, h, w), nblk = up2_wgrad_blocks(B, h, w);
    float* part = (float*)ws;
    const size_t nfold = (size_t)UJ * UK * UK * C;
    float* dwf = part + (size_t)nblk * nfold;
    if (C % 32 == 0)
        hipLaunchKernelGGL((up2_wgrad_kernel<32, T>), dim3(nblk, C / 32), dim3(256), 0, s, x, ldx, B, h, w, C, dy, lddy, part, tiles);
    else if (C % 16 == 0)
        hipLaunchKernelGGL((up2_wgrad_kernel<16, T>), dim3(nblk, C / 16), dim3(256), 0, s, x, ldx, B, h, w, C, dy, lddy, part, tiles);
    else
        hipLaunchKernelGGL((up2_wgrad_kernel<8, T>), dim3(nblk, C / 8), dim3(256), 0, s, x, ldx, B, h, w, C, dy, lddy, part, tiles);
    int err = (int)hipGetLastError();
    if (err) return err;
    err = launch_splitk_reduce(part, nblk, nfold, dwf, 0.f, nullptr, s);       // fixed order: slab 0, 1, ..
    if (err) return err;
    hipLaunchKernelGGL(up2_unfold_kernel, dim3((2 * 36 * C + 255) / 256), dim3(256), 0, s, dwf, C, dw);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int unetrir_head_up2_supported_f32(int C) { return up2_c_ok(C) ? 7 : 0; }
int unetrir_head_up2_supported_bf16(int C) { return up2_c_ok(C) ? 7 : 0; }

int unetrir_head_up2_fold(const float* w, int C, float* wf, int round_bf16, unetrir_stream_t stream) {
    if (!w || !wf || !up2_c_ok(C) || ((uintptr_t)w & 3) || ((uintptr_t)wf & 15)) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(up2_fold_kernel, dim3((UJ * UK * UK * C + 255) / 256), dim3(256), 0, (hipStream_t)stream, w, C, wf, round_bf16);
    return (int)hipGetLastError();
}

int unetrir_head_up2_fwd_f32(const float* x, int ldx, int B, int h, int w, int C, const float* wf, const float* bias, float* y, int ldy,
                             unetrir_stream_t stream) {
    return up2_fwd_impl<float>(x, ldx, B, h, w, C, wf, bias, y, ldy, (hipStream_t)stream);
}

int unetrir_head_up2_fwd_bf16(const unetrir_bf16* x, int ldx, int B, int h, int w, int C, const float* wf, const float* bias, float* y,
                              int ldy, unetrir_stream_t stream) {
    return up2_fwd_impl<__bf16>((const __bf16*)x, ldx, B, h, w, C, wf, bias, y, ldy, (hipStream_t)stream);
}

int unetrir_head_up2_dgrad_f32(const float* dy, int lddy, int B, int h, int w, const float* wf, int C, float* dx, int lddx,
                               unetrir_stream_t stream) {
    return up2_dgrad_impl<float>(dy, lddy, B, h, w, wf, C, dx, lddx, (hipStream_t)stream);
}

int unetrir_head_up2_dgrad_bf16(const unetrir_bf16* dy, int lddy, int B, int h, int w, const float* wf, int C, unetrir_bf16* dx, int lddx,
                                unetrir_stream_t stream) {
    return up2_dgrad_impl<__bf16>((const __bf16*)dy, lddy, B, h, w, wf, C, (__bf16*)dx, lddx, (hipStream_t)stream);
}

size_t unetrir_head_up2_wgrad_ws_bytes(int B, int h, int w, int C) { return up2_wgrad_ws(B, h, w, C); }

int unetrir_head_up2_wgrad_f32(const float* x, int ldx, int B, int h, int w, int C, const float* dy, int lddy, float* dw, void* ws,
                               size_t ws_bytes, unetrir_stream_t stream) {
    return up2_wgrad_impl<float>(x, ldx, B, h, w, C, dy, lddy, dw, ws, ws_bytes, (hipStream_t)stream);
}

int unetrir_head_up2_wgrad_bf16(const unetrir_bf16* x, int ldx, int B, int h, int w, int C, const unetrir_bf16* dy, int lddy, float* dw,
                                void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    return up2_wgrad_impl<__bf16>((const __bf16*)x, ldx, B, h, w, C, (const __bf16*)dy, lddy, dw, ws, ws_bytes, (hipStream_t)stream);
}

}  // extern "C"
