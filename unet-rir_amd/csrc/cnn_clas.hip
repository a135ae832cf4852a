// cnn_clas.hip - what the room classifier deep_CNN (dl_models/cnn_clas.py:19-53) needs beyond the generator models: Conv2D(3x3,
// strides 1, padding='valid', activation='relu') and its two gradients, AveragePooling2D(2x2, strides 2, 'valid') and
// GlobalAveragePooling2D with the BatchNormalization affine of the layer in front folded in, and the softmax output fused with
// categorical_crossentropy and the accuracy count.  fp32 storage, plain HIP C++; the contracts are in include/unetrir.h.
//
// Why direct arithmetic and not the matrix cores: the whole train step is ~6 GFLOP at 144 x 160, batch 32, and on gfx950 the fp32
// MFMA rate equals the fp32 vector rate, so a matrix-core form buys no arithmetic here; every launch is bound by memory and by
// launch count.  The convolution therefore keeps one output pixel per lane and CC_NG output channels per thread, reads its 3x3
// input patch straight from global memory (16-byte loads; neighbouring lanes read neighbouring pixels) and its weights through
// wave-uniform addresses, which the compiler serves from the scalar cache: no LDS, no barrier, every sum a k-ordered fmaf chain.
#include "kernels.h"

#define CC_T 256
#define CC_NG 16            // output channels per thread of the gather kernel (4 for a 4-channel output)

// out[b, oy, ox, n] = sum_t sum_c in[b, oy + ty - pad, ox + tx - pad, c] * w[n][flip ? 8 - t : t][c] (+ bias[n]) (ReLU), pixels
// outside the input contributing nothing.  Forward: pad 0, in = x.  Data gradient: pad 2, flip, in = dy (MASK: times [y > 0]),
// w = the kernel with the channel roles swapped.
template <int NG, bool MASK>
__global__ __launch_bounds__(CC_T) void conv_valid_gather_kernel(const float* __restrict__ in, int ldi, int IH, int IW, int C,
                                                                 const float* __restrict__ mask, int ldm, const float* __restrict__ w,
                                                                 const float* __restrict__ bias, int relu, float* __restrict__ out, int ldo,
                                                                 int OH, int OW, int pad, int flip, long long npix) {
    const long long p = (long long)blockIdx.x * CC_T + threadIdx.x;
    if (p >= npix) return;
    const int n0 = blockIdx.y * NG;
    const int ox = (int)(p % OW);
    const long long q = p / OW;
    const int oy = (int)(q % OH);
    const long long b = q / OH;
    float acc[NG];
#pragma unroll
    for (int n = 0; n < NG; ++n) acc[n] = 0.f;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const int iy = oy + t / 3 - pad, ix = ox + t % 3 - pad;
        const bool ok = iy >= 0 && iy < IH && ix >= 0 && ix < IW;
        const long long ipix = ok ? ((b * IH + iy) * IW + ix) : 0;
        const float* ip = in + ipix * ldi;
        const float* mp = MASK ? mask + ipix * ldm : nullptr;
        const float* wp = w + ((long long)n0 * 9 + (flip ? 8 - t : t)) * C;          // wave-uniform
        for (int c = 0; c < C; c += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                v = *reinterpret_cast<const float4*>(ip + c);
                if (MASK) {
                    const float4 m = *reinterpret_cast<const float4*>(mp + c);
                    v.x = m.x > 0.f ? v.x : 0.f;
                    v.y = m.y > 0.f ? v.y : 0.f;
                    v.z = m.z > 0.f ? v.z : 0.f;
                    v.w = m.w > 0.f ? v.w : 0.f;
                }
            }
#pragma unroll
            for (int n = 0; n < NG; ++n) {
                const float4 wv = *reinterpret_cast<const float4*>(wp + (long long)n * 9 * C + c);
                acc[n] = fmaf(v.x, wv.x, acc[n]);
                acc[n] = fmaf(v.y, wv.y, acc[n]);
                acc[n] = fmaf(v.z, wv.z, acc[n]);
                acc[n] = fmaf(v.w, wv.w, acc[n]);
            }
        }
    }
    float* op = out + p * ldo + n0;
#pragma unroll
    for (int n = 0; n < NG; n += 4) {
        float4 o = make_float4(acc[n], acc[n + 1], acc[n + 2], acc[n + 3]);
        if (bias) {
            const float4 bv = *reinterpret_cast<const float4*>(bias + n0 + n);
            o.x += bv.x; o.y += bv.y; o.z += bv.z; o.w += bv.w;
        }
        if (relu) {
            o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
        }
        *reinterpret_cast<float4*>(op + n) = o;
    }
}

// Weight and bias gradient partials.  One thread owns the pair (co, ci) for all nine taps; a slab is a range of output rows
// (b, oy), walked left to right with the 3x3 window of x kept in registers (three new values per pixel).  part[slab] holds
// [CO][9][CI] followed by [CO] (the bias gradient, written by the ci == 0 threads).  MASK: dy times [y > 0] on load.
template <int CI, bool MASK>
__global__ __launch_bounds__(CC_T) void conv_valid_wgrad_kernel(const float* __restrict__ x, int ldx, int IH, int IW,
                                                                const float* __restrict__ dy, int lddy, const float* __restrict__ y, int ldy,
                                                                int OH, int OW, int CO, long long rows, int rows_per_slab, int nslab,
                                                                float* __restrict__ part) {
    const int pairs = CO * CI;
    int slab, pair;
    if (pairs >= CC_T) {
        const int bps = pairs / CC_T;
        slab = blockIdx.x / bps;
        pair = (blockIdx.x % bps) * CC_T + threadIdx.x;
    } else {
        const int sub = CC_T / pairs;
        slab = blockIdx.x * sub + threadIdx.x / pairs;
        pair = threadIdx.x % pairs;
    }
    if (slab >= nslab) return;
    const int ci = pair % CI, co = pair / CI;
    float acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = 0.f;
    float accb = 0.f;
    const long long r0 = (long long)slab * rows_per_slab;
    const long long r1 = r0 + rows_per_slab < rows ? r0 + rows_per_slab : rows;
    for (long long r = r0; r < r1; ++r) {
        const long long b = r / OH;
        const int oy = (int)(r - b * OH);
        const float* xr = x + ((b * IH + oy) * IW) * ldx + ci;
        const float* gr = dy + (r * OW) * lddy + co;
        const float* yr = MASK ? y + (r * OW) * ldy + co : nullptr;
        float a0[3], a1[3], a2[3];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            a0[ky] = xr[(long long)ky * IW * ldx];
            a1[ky] = xr[((long long)ky * IW + 1) * ldx];
        }
        for (int ox = 0; ox < OW; ++ox) {
            float g = gr[(long long)ox * lddy];
            if (MASK) g = yr[(long long)ox * ldy] > 0.f ? g : 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                a2[ky] = xr[((long long)ky * IW + ox + 2) * ldx];
                acc[ky * 3 + 0] = fmaf(g, a0[ky], acc[ky * 3 + 0]);
                acc[ky * 3 + 1] = fmaf(g, a1[ky], acc[ky * 3 + 1]);
                acc[ky * 3 + 2] = fmaf(g, a2[ky], acc[ky * 3 + 2]);
                a0[ky] = a1[ky];
                a1[ky] = a2[ky];
            }
            accb += g;
        }
    }
    const long long stride = (long long)CO * 9 * CI + CO;
    float* ps = part + slab * stride;
#pragma unroll
    for (int t = 0; t < 9; ++t) ps[((long long)co * 9 + t) * CI + ci] = acc[t];
    if (ci == 0) ps[(long long)CO * 9 * CI + co] = accb;
}

// dw / dbias = the slabs summed in a fixed order: 16 lanes per output take every 16th slab in slab order, a fixed tree joins them
#define CC_RG 16
__global__ __launch_bounds__(CC_T) void conv_valid_wgrad_reduce_kernel(const float* __restrict__ part, int nslab, int n, int nw,
                                                                       float* __restrict__ dw, float* __restrict__ dbias) {
    __shared__ float red[CC_T];
    const int lane = threadIdx.x % 16, grp = threadIdx.x / 16;
    const int i = blockIdx.x * 16 + lane;
    float s = 0.f;
    if (i < n)
        for (int k = grp; k < nslab; k += CC_RG) s += part[(long long)k * n + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = CC_RG / 2; h > 0; h >>= 1) {
        if (grp < h) red[threadIdx.x] += red[threadIdx.x + h * 16];
        __syncthreads();
    }
    if (grp == 0 && i < n) {
        if (i < nw) dw[i] = red[lane];
        else dbias[i - nw] = red[lane];
    }
}

// AveragePooling2D(2x2, strides 2, 'valid') of BatchNormalization(x): the affine is per channel, so pool(x scale + shift) =
// pool(x) scale + shift; one thread per (pooled pixel, 4 channels).  affine NULL: plain pooling.
__global__ void avgpool2_fwd_kernel(const float* __restrict__ x, int ldx, int H, int W, int C4, int PH, int PW,
                                    const float* __restrict__ affine, float* __restrict__ y, int ldy, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) << 2;
        long long q = i / C4;
        const int px = (int)(q % PW);
        q /= PW;
        const int py = (int)(q % PH);
        const long long b = q / PH;
        const float* p0 = x + ((b * H + 2 * py) * W + 2 * px) * ldx + c;
        const float4 a = *reinterpret_cast<const float4*>(p0);
        const float4 bq = *reinterpret_cast<const float4*>(p0 + ldx);
        const float4 cq = *reinterpret_cast<const float4*>(p0 + (long long)W * ldx);
        const float4 d = *reinterpret_cast<const float4*>(p0 + (long long)(W + 1) * ldx);
        float4 o;
        o.x = 0.25f * ((a.x + bq.x) + (cq.x + d.x));
        o.y = 0.25f * ((a.y + bq.y) + (cq.y + d.y));
        o.z = 0.25f * ((a.z + bq.z) + (cq.z + d.z));
        o.w = 0.25f * ((a.w + bq.w) + (cq.w + d.w));
        if (affine) {
            const float4 sc = *reinterpret_cast<const float4*>(affine + c);
            const float4 sh = *reinterpret_cast<const float4*>(affine + 4 * C4 + c);
            o.x = fmaf(o.x, sc.x, sh.x); o.y = fmaf(o.y, sc.y, sh.y); o.z = fmaf(o.z, sc.z, sh.z); o.w = fmaf(o.w, sc.w, sh.w);
        }
        *reinterpret_cast<float4*>(y + ((b * PH + py) * PW + px) * ldy + c) = o;
    }
}

// its adjoint: every pixel of the 2x2 cell gets dy / 4, a trailing odd row or column (read by nothing) exactly zero
__global__ void avgpool2_bwd_kernel(const float* __restrict__ dy, int lddy, int H, int W, int C4, int PH, int PW,
                                    float* __restrict__ dx, int lddx, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) << 2;
        long long q = i / C4;
        const int ix = (int)(q % W);
        q /= W;
        const int iy = (int)(q % H);
        const long long b = q / H;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((iy >> 1) < PH && (ix >> 1) < PW) {
            const float4 g = *reinterpret_cast<const float4*>(dy + ((b * PH + (iy >> 1)) * PW + (ix >> 1)) * lddy + c);
            o = make_float4(0.25f * g.x, 0.25f * g.y, 0.25f * g.z, 0.25f * g.w);
        }
        *reinterpret_cast<float4*>(dx + ((b * H + iy) * W + ix) * lddx + c) = o;
    }
}

// GlobalAveragePooling2D (of BatchNormalization(x), as above): one workgroup per image; thread = (4 channels, pixel lane), every
// lane sums its pixels in index order, a fixed tree joins the lanes.
__global__ __launch_bounds__(CC_T) void gap_fwd_kernel(const float* __restrict__ x, int ldx, int HW, int C4, int lanes, float inv,
                                                       const float* __restrict__ affine, float* __restrict__ y, int ldy) {
    __shared__ float4 red[CC_T];
    const int c4 = threadIdx.x % C4, pl = threadIdx.x / C4;
    const long long b = blockIdx.x;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (pl < lanes) {
        const float* xp = x + b * HW * ldx + 4 * c4;
        for (int p = pl; p < HW; p += lanes) {
            const float4 v = *reinterpret_cast<const float4*>(xp + (long long)p * ldx);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = lanes / 2; h > 0; h >>= 1) {
        if (pl < h) {
            const float4 o = red[threadIdx.x + h * C4];
            float4 m = red[threadIdx.x];
            m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
            red[threadIdx.x] = m;
        }
        __syncthreads();
    }
    if (pl == 0) {
        float4 o = red[threadIdx.x];
        o.x *= inv; o.y *= inv; o.z *= inv; o.w *= inv;
        if (affine) {
            const float4 sc = *reinterpret_cast<const float4*>(affine + 4 * c4);
            const float4 sh = *reinterpret_cast<const float4*>(affine + 4 * C4 + 4 * c4);
            o.x = fmaf(o.x, sc.x, sh.x); o.y = fmaf(o.y, sc.y, sh.y); o.z = fmaf(o.z, sc.z, sh.z); o.w = fmaf(o.w, sc.w, sh.w);
        }
        *reinterpret_cast<float4*>(y + b * ldy + 4 * c4) = o;
    }
}

__global__ void gap_bwd_kernel(const float* __restrict__ dy, int lddy, int HW, int C4, float inv, float* __restrict__ dx, int lddx,
                               long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % C4) << 2;
        const long long pix = i / C4;
        const long long b = pix / HW;
        const float4 g = *reinterpret_cast<const float4*>(dy + b * lddy + c);
        *reinterpret_cast<float4*>(dx + pix * lddx + c) = make_float4(g.x * inv, g.y * inv, g.z * inv, g.w * inv);
    }
}

// ---- softmax (+ categorical_crossentropy + accuracy).  One wave per row, the classes strided over its lanes; every cross-lane
// reduction is a butterfly, so all lanes hold the same bits and two runs agree.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// (largest value, lowest index among equals)
__device__ __forceinline__ void wave_argmax(float& v, int& i) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const float ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(i, m, 64);
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
}

__device__ __forceinline__ void row_argmax(const float* __restrict__ r, int K, int lane, float& best, int& idx) {
    best = -INFINITY;
    idx = 0x7fffffff;
    for (int c = lane; c < K; c += 64) {
        const float v = r[c];
        if (v > best || idx == 0x7fffffff) { best = v; idx = c; }      // strict: the lowest index of a lane stays
    }
    wave_argmax(best, idx);
}

// probabilities of row `z` into `p` from the max-subtracted logits; returns log(sum exp(z - m)) and m
__device__ __forceinline__ float row_softmax(const float* __restrict__ z, int K, int lane, float m, float* __restrict__ p) {
    float s = 0.f;
    for (int c = lane; c < K; c += 64) s += expf(z[c] - m);
    s = wave_sum(s);
    const float inv = 1.0f / s;
    for (int c = lane; c < K; c += 64) p[c] = expf(z[c] - m) * inv;
    return logf(s);
}

// target != NULL: ONE workgroup; probs, dlogits = (p sum(y) - y) inv_norm, loss_out, acc_out.  The loss is the log-softmax of the
// max-subtracted logits, CE_b = -sum_c y_c ((z_c - m) - log sum exp(z - m)); rows are added in fp64 in row order per wave, the
// four waves in wave order.  target == NULL: probabilities only, any grid.
__global__ __launch_bounds__(CC_T) void softmax_ce_kernel(const float* __restrict__ logits, int ldl, const float* __restrict__ target,
                                                          int B, int K, float inv_norm, float* __restrict__ probs,
                                                          float* __restrict__ dlogits, int ldd, float* __restrict__ loss_out,
                                                          float* __restrict__ acc_out) {
    __shared__ double red_ce[CC_T / 64];
    __shared__ int red_ok[CC_T / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (CC_T / 64) * gridDim.x;
    double ce = 0.0;
    int n_ok = 0;
    for (int b = blockIdx.x * (CC_T / 64) + wave; b < B; b += nw) {
        const float* z = logits + (long long)b * ldl;
        float* p = probs + (long long)b * K;
        float m;
        int am;
        row_argmax(z, K, lane, m, am);
        const float logs = row_softmax(z, K, lane, m, p);
        if (!target) continue;
        const float* y = target + (long long)b * K;
        float ym;
        int ay;
        row_argmax(y, K, lane, ym, ay);
        float sy = 0.f, e = 0.f;
        for (int c = lane; c < K; c += 64) {
            sy += y[c];
            e -= y[c] * ((z[c] - m) - logs);
        }
        sy = wave_sum(sy);
        e = wave_sum(e);
        float* d = dlogits + (long long)b * ldd;
        for (int c = lane; c < ldd; c += 64) d[c] = c < K ? (p[c] * sy - y[c]) * inv_norm : 0.f;
        ce += (double)e;
        n_ok += am == ay;
    }
    if (!target) return;
    if (lane == 0) { red_ce[wave] = ce; red_ok[wave] = n_ok; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        int k = 0;
        for (int w = 0; w < CC_T / 64; ++w) { t += red_ce[w]; k += red_ok[w]; }
        const float raw = (float)t;
        loss_out[0] = raw * inv_norm;
        loss_out[1] = raw;
        loss_out[2] = 0.f;
        acc_out[0] = (float)k;
    }
}

// dlogits from an upstream gradient on the probabilities: dz_c = p_c (dp_c - sum_k dp_k p_k)
__global__ __launch_bounds__(CC_T) void softmax_bwd_kernel(const float* __restrict__ probs, const float* __restrict__ dprobs, int B, int K,
                                                           float* __restrict__ dlogits, int ldd) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nw = (CC_T / 64) * gridDim.x;
    for (int b = blockIdx.x * (CC_T / 64) + wave; b < B; b += nw) {
        const float* p = probs + (long long)b * K;
        const float* g = dprobs + (long long)b * K;
        float s = 0.f;
        for (int c = lane; c < K; c += 64) s += g[c] * p[c];
        s = wave_sum(s);
        float* d = dlogits + (long long)b * ldd;
        for (int c = lane; c < ldd; c += 64) d[c] = c < K ? p[c] * (g[c] - s) : 0.f;
    }
}

// ---- host side
static inline bool cc_misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline bool cc_bad_ld(int ld, int C) { return ld < C || (ld & 3); }
static inline unsigned cc_grid(long long n) {
    const long long b = (n + CC_T - 1) / CC_T;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}
static inline bool cc_cin_ok(int c) { return c == 4 || c == 16 || c == 32; }
static inline bool cc_cout_ok(int c) { return c == 16 || c == 32 || c == 64; }
static inline bool cc_geom_ok(const unetrir_conv_geom* g) {
    return g && g->k == 3 && g->stride == 1 && g->B > 0 && g->H >= 3 && g->W >= 3 && cc_cin_ok(g->Cin) && cc_cout_ok(g->Cout);
}

// The split of the weight gradient depends on the geometry alone: ~8192 waves in flight (eight per SIMD: the row walk waits on
// global loads and has little else to do), a slab = whole output rows.
static void cc_wgrad_plan(const unetrir_conv_geom* g, long long* rows, int* rows_per_slab, int* nslab) {
    const long long R = (long long)g->B * (g->H - 2);
    const int pairs = g->Cin * g->Cout;
    long long target = 8192LL * 64 / pairs;
    if (target < 1) target = 1;
    if (target > R) target = R;
    const long long rps = (R + target - 1) / target;
    *rows = R;
    *rows_per_slab = (int)rps;
    *nslab = (int)((R + rps - 1) / rps);
}

template <int NG>
static int cc_launch_gather(bool masked, dim3 grid, hipStream_t s, const float* in, int ldi, int IH, int IW, int C, const float* mask,
                            int ldm, const float* w, const float* bias, int relu, float* out, int ldo, int OH, int OW, int pad, int flip,
                            long long npix) {
    if (masked)
        hipLaunchKernelGGL((conv_valid_gather_kernel<NG, true>), grid, dim3(CC_T), 0, s, in, ldi, IH, IW, C, mask, ldm, w, bias, relu, out,
                           ldo, OH, OW, pad, flip, npix);
    else
        hipLaunchKernelGGL((conv_valid_gather_kernel<NG, false>), grid, dim3(CC_T), 0, s, in, ldi, IH, IW, C, mask, ldm, w, bias, relu, out,
                           ldo, OH, OW, pad, flip, npix);
    return (int)hipGetLastError();
}

// Output channels per thread: 16, or 4 for a 4-channel output (the first layer's data gradient).  Measured: 8 per thread, for twice
// the waves on the deep layers' small images, is 2.4 - 3 x SLOWER - the kernel is bound by its
// 16-byte patch loads, which at >= 16 channels per pixel touch one cache line per lane, and halving the channels per thread
// doubles those loads.
static int cc_gather(bool masked, long long npix, int N, hipStream_t s, const float* in, int ldi, int IH, int IW, int C, const float* mask,
                     int ldm, const float* w, const float* bias, int relu, float* out, int ldo, int OH, int OW, int pad, int flip) {
    const unsigned gx = (unsigned)((npix + CC_T - 1) / CC_T);
    if (N == 4) return cc_launch_gather<4>(masked, dim3(gx, 1), s, in, ldi, IH, IW, C, mask, ldm, w, bias, relu, out, ldo, OH, OW, pad, flip, npix);
    return cc_launch_gather<CC_NG>(masked, dim3(gx, N / CC_NG), s, in, ldi, IH, IW, C, mask, ldm, w, bias, relu, out, ldo, OH, OW, pad, flip, npix);
}

template <int CI>
static int cc_launch_wgrad(bool masked, dim3 grid, hipStream_t s, const float* x, int ldx, int IH, int IW, const float* dy, int lddy,
                           const float* y, int ldy, int OH, int OW, int CO, long long rows, int rps, int nslab, float* part) {
    if (masked)
        hipLaunchKernelGGL((conv_valid_wgrad_kernel<CI, true>), grid, dim3(CC_T), 0, s, x, ldx, IH, IW, dy, lddy, y, ldy, OH, OW, CO, rows,
                           rps, nslab, part);
    else
        hipLaunchKernelGGL((conv_valid_wgrad_kernel<CI, false>), grid, dim3(CC_T), 0, s, x, ldx, IH, IW, dy, lddy, y, ldy, OH, OW, CO, rows,
                           rps, nslab, part);
    return (int)hipGetLastError();
}

extern "C" {

int unetrir_conv3x3_valid_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* w, const float* bias, int relu,
                                  float* y, int ldy, unetrir_stream_t stream) {
    if (!cc_geom_ok(g) || !x || !w || !bias || !y || cc_bad_ld(ldx, g->Cin) || cc_bad_ld(ldy, g->Cout)) return UNETRIR_EINVAL;
    if (cc_misaligned(x) || cc_misaligned(w) || cc_misaligned(bias) || cc_misaligned(y)) return UNETRIR_EINVAL;
    const int OH = g->H - 2, OW = g->W - 2;
    const long long npix = (long long)g->B * OH * OW;
    return cc_gather(false, npix, g->Cout, (hipStream_t)stream, x, ldx, g->H, g->W, g->Cin, nullptr, 0, w, bias, relu, y, ldy, OH, OW, 0, 0);
}

int unetrir_conv3x3_valid_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy, const float* y, int ldy, int relu,
                                    const float* wt, float* dx, int lddx, unetrir_stream_t stream) {
    if (!cc_geom_ok(g) || !dy || !wt || !dx || (relu && !y) || cc_bad_ld(lddy, g->Cout) || cc_bad_ld(lddx, g->Cin)) return UNETRIR_EINVAL;
    if (relu && cc_bad_ld(ldy, g->Cout)) return UNETRIR_EINVAL;
    if (cc_misaligned(dy) || cc_misaligned(wt) || cc_misaligned(dx) || (relu && cc_misaligned(y))) return UNETRIR_EINVAL;
    const int OH = g->H - 2, OW = g->W - 2;
    const long long npix = (long long)g->B * g->H * g->W;
    return cc_gather(relu != 0, npix, g->Cin, (hipStream_t)stream, dy, lddy, OH, OW, g->Cout, y, ldy, wt, nullptr, 0, dx, lddx, g->H, g->W, 2, 1);
}

size_t unetrir_conv3x3_valid_wgrad_ws_bytes(const unetrir_conv_geom* g) {
    if (!cc_geom_ok(g)) return 0;
    long long rows;
    int rps, nslab;
    cc_wgrad_plan(g, &rows, &rps, &nslab);
    return (size_t)nslab * ((size_t)g->Cout * 9 * g->Cin + g->Cout) * sizeof(float);
}

int unetrir_conv3x3_valid_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* dy, int lddy, const float* y,
                                    int ldy, int relu, float* dw, float* dbias, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!cc_geom_ok(g) || !x || !dy || !dw || !dbias || !ws || (relu && !y) || cc_bad_ld(ldx, g->Cin) || cc_bad_ld(lddy, g->Cout))
        return UNETRIR_EINVAL;
    if (relu && cc_bad_ld(ldy, g->Cout)) return UNETRIR_EINVAL;
    if (ws_bytes < unetrir_conv3x3_valid_wgrad_ws_bytes(g) || cc_misaligned(ws)) return UNETRIR_EINVAL;
    long long rows;
    int rps, nslab;
    cc_wgrad_plan(g, &rows, &rps, &nslab);
    const int pairs = g->Cin * g->Cout;
    const unsigned blocks = pairs >= CC_T ? (unsigned)nslab * (pairs / CC_T) : (unsigned)((nslab + CC_T / pairs - 1) / (CC_T / pairs));
    const int OH = g->H - 2, OW = g->W - 2;
    hipStream_t s = (hipStream_t)stream;
    int err;
    if (g->Cin == 4)
        err = cc_launch_wgrad<4>(relu != 0, dim3(blocks), s, x, ldx, g->H, g->W, dy, lddy, y, ldy, OH, OW, g->Cout, rows, rps, nslab, (float*)ws);
    else if (g->Cin == 16)
        err = cc_launch_wgrad<16>(relu != 0, dim3(blocks), s, x, ldx, g->H, g->W, dy, lddy, y, ldy, OH, OW, g->Cout, rows, rps, nslab, (float*)ws);
    else
        err = cc_launch_wgrad<32>(relu != 0, dim3(blocks), s, x, ldx, g->H, g->W, dy, lddy, y, ldy, OH, OW, g->Cout, rows, rps, nslab, (float*)ws);
    if (err) return err;
    const int nw = g->Cout * 9 * g->Cin, n = nw + g->Cout;
    hipLaunchKernelGGL(conv_valid_wgrad_reduce_kernel, dim3((n + 15) / 16), dim3(CC_T), 0, s, (const float*)ws, nslab, n, nw, dw, dbias);
    return (int)hipGetLastError();
}

int unetrir_avgpool2_fwd_f32(const float* x, int ldx, int B, int H, int W, int C, const float* affine, float* y, int ldy,
                             unetrir_stream_t stream) {
    if (!x || !y || B <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3) || cc_bad_ld(ldx, C) || cc_bad_ld(ldy, C)) return UNETRIR_EINVAL;
    if (cc_misaligned(x) || cc_misaligned(y) || cc_misaligned(affine)) return UNETRIR_EINVAL;
    const int PH = H / 2, PW = W / 2;
    const long long n = (long long)B * PH * PW * (C / 4);
    hipLaunchKernelGGL(avgpool2_fwd_kernel, dim3(cc_grid(n)), dim3(CC_T), 0, (hipStream_t)stream, x, ldx, H, W, C / 4, PH, PW, affine, y, ldy, n);
    return (int)hipGetLastError();
}

int unetrir_avgpool2_bwd_f32(const float* dy, int lddy, int B, int H, int W, int C, float* dx, int lddx, unetrir_stream_t stream) {
    if (!dy || !dx || B <= 0 || H < 2 || W < 2 || C <= 0 || (C & 3) || cc_bad_ld(lddy, C) || cc_bad_ld(lddx, C)) return UNETRIR_EINVAL;
    if (cc_misaligned(dy) || cc_misaligned(dx)) return UNETRIR_EINVAL;
    const long long n = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(avgpool2_bwd_kernel, dim3(cc_grid(n)), dim3(CC_T), 0, (hipStream_t)stream, dy, lddy, H, W, C / 4, H / 2, W / 2, dx, lddx, n);
    return (int)hipGetLastError();
}

int unetrir_gap_fwd_f32(const float* x, int ldx, int B, int H, int W, int C, const float* affine, float* y, int ldy,
                        unetrir_stream_t stream) {
    if (!x || !y || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || C > 4 * CC_T || cc_bad_ld(ldx, C) || cc_bad_ld(ldy, C)) return UNETRIR_EINVAL;
    if (cc_misaligned(x) || cc_misaligned(y) || cc_misaligned(affine)) return UNETRIR_EINVAL;
    const int C4 = C / 4;
    int lanes = 1;
    while (lanes * 2 * C4 <= CC_T) lanes *= 2;
    hipLaunchKernelGGL(gap_fwd_kernel, dim3(B), dim3(CC_T), 0, (hipStream_t)stream, x, ldx, H * W, C4, lanes, 1.0f / (float)((long long)H * W),
                       affine, y, ldy);
    return (int)hipGetLastError();
}

int unetrir_gap_bwd_f32(const float* dy, int lddy, int B, int H, int W, int C, float* dx, int lddx, unetrir_stream_t stream) {
    if (!dy || !dx || B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || cc_bad_ld(lddy, C) || cc_bad_ld(lddx, C)) return UNETRIR_EINVAL;
    if (cc_misaligned(dy) || cc_misaligned(dx)) return UNETRIR_EINVAL;
    const long long n = (long long)B * H * W * (C / 4);
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(cc_grid(n)), dim3(CC_T), 0, (hipStream_t)stream, dy, lddy, H * W, C / 4,
                       1.0f / (float)((long long)H * W), dx, lddx, n);
    return (int)hipGetLastError();
}

int unetrir_softmax_ce_f32(const float* logits, int ldl, const float* target, int B, int classes, float inv_norm, float* probs,
                           float* dlogits, int ldd, float* loss_out, float* acc_out, unetrir_stream_t stream) {
    if (!logits || !target || !probs || !dlogits || !loss_out || !acc_out || B <= 0 || classes < 1 || classes > 1024 || ldl < classes ||
        ldd < classes)
        return UNETRIR_EINVAL;
    hipLaunchKernelGGL(softmax_ce_kernel, dim3(1), dim3(CC_T), 0, (hipStream_t)stream, logits, ldl, target, B, classes, inv_norm, probs,
                       dlogits, ldd, loss_out, acc_out);
    return (int)hipGetLastError();
}

int unetrir_softmax_fwd_f32(const float* logits, int ldl, int B, int classes, float* probs, unetrir_stream_t stream) {
    if (!logits || !probs || B <= 0 || classes < 1 || classes > 1024 || ldl < classes) return UNETRIR_EINVAL;
    const int blocks = (B + 3) / 4 > 1024 ? 1024 : (B + 3) / 4;
    hipLaunchKernelGGL(softmax_ce_kernel, dim3(blocks), dim3(CC_T), 0, (hipStream_t)stream, logits, ldl, (const float*)nullptr, B, classes,
                       0.f, probs, (float*)nullptr, 0, (float*)nullptr, (float*)nullptr);
    return (int)hipGetLastError();
}

int unetrir_softmax_bwd_f32(const float* probs, const float* dprobs, int B, int classes, float* dlogits, int ldd,
                            unetrir_stream_t stream) {
    if (!probs || !dprobs || !dlogits || B <= 0 || classes < 1 || classes > 1024 || ldd < classes) return UNETRIR_EINVAL;
    const int blocks = (B + 3) / 4 > 1024 ? 1024 : (B + 3) / 4;
    hipLaunchKernelGGL(softmax_bwd_kernel, dim3(blocks), dim3(CC_T), 0, (hipStream_t)stream, probs, dprobs, B, classes, dlogits, ldd);
    return (int)hipGetLastError();
}

}  // extern "C"
