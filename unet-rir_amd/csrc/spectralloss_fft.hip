// spectralloss_fft.hip - the FFT form of the multi-resolution STFT loss: the definition of spectralloss.hip's header (same E0, P0, delta,
// M_x, SC, LM, Q_b, L, same gradient, same frames, same fold of the reflected edges, resolutions summed in index order) with fp32
// transforms held in LDS (fft_lds.h) in place of fp64 DFTs on the matrix cores (gfx950).
//
// Arithmetic.  Window taps, spectra and every per-bin quantity (M_y^, M_y, their difference, the logarithms, g, g X^) are fp32.  Every
// reduction - E0, sum w^2, the three sums of a (row, resolution), the sums over r and b, the overlap-add and fold of a sample - is
// accumulated in fp64 from fp32 terms in a fixed order, and every element of dwav is rounded once.  The error against the fp64
// definition is that of an fp32 STFT and its adjoint (include/unetrir.h), not the derived fp64 bound of the DFT form: that form is
// the one to hold a gradient to a bound, this one is for a term that is paid every step.
//
// A real transform of N points is a complex FFT of M = N / 2 points worked by M / 8 threads (fft_lds.h).  fl_fft meets at workgroup
// barriers only, so thread group g (M / 8 consecutive threads) works the image at buf + g M with t = tid mod (M / 8), and all groups run
// the same passes in lockstep: one workgroup of 256 threads carries 2048 / M images in 16 KB.  Here these are FR = 1024 / M consecutive
// frames of one (row, resolution), of y^ (groups 0 ... FR - 1) and of y (groups FR ... 2 FR - 1).
//
// Four launches for loss and gradient whatever B and R are, two for the loss alone:
//   1 slf_analysis_kernel  the loader builds the windowed, reflected frames directly as the packed image z[n] = a[2n] + i a[2n+1] at the
//                          swizzled address; fl_fft<M, -1>, fl_split_fwd<M> (slot 0 holds bins 0 and N / 2, both real); the epilogue forms
//                          M_y^, M_y and the three partial sums of the workgroup: one slab.  No spectrum is written to memory.  E0_b and
//                          sum w^2 are recomputed per workgroup in a fixed order (every workgroup of a row forms the same bits).
//   2 sl_finalize_kernel   the DFT form's (spectralloss_common.h), over these slabs.
//   3 slf_adjoint_kernel   recomputes the analysis of its frames (cheaper than four planes of spectra in memory), forms G = g X^ with
//                          the row scalars, halves the interior bins 0 < k < N / 2 (exact) - sum_{k=0}^{N/2} (dRe cos - dIm sin) is N
//                          irfft of that, and the header's inverse returns the signal times 2 M = N, so nothing else scales - runs
//                          fl_split_inv and fl_fft<M, +1> in the same image, multiplies by the window and writes the win non-zero taps
//                          of each frame as fp32.
//   4 sl_fold_kernel       the DFT form's gather (spectralloss_common.h) on fp32 frames, accumulated in fp64.
// No atomics, every summation order fixed, complex products through fl_mul (contraction off): two runs give the same bits, and a row's
// bits depend neither on B nor on its place in the batch.  Nothing is allocated, cleared or waited for, so the call can be captured
// in a HIP graph.  A row with a silent target counts nothing and gets zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"
#include "spectralloss_common.h"
#include "fft_lds.h"

namespace {

using namespace fftlds;

constexpr int SF_IMG = 2048;                  // complex points of the workgroup's image: 16 KB

struct SfRes {
    int N, win, hop, F, K, n_lo;
    int ntiles;                               // workgroups of 2048 / N frames
    int tile0;                                // this resolution's first workgroup in the grid of a row
    long long frame0;                         // offset (floats) of its frames inside a row's share
};

struct SfPlan {
    int R, B, T;
    int tiles;                                // workgroups of one row
    long long frames_row;                     // floats per row
    SfRes res[SL_MAX_R];
};

// workspace:  doubles  slabs [B][tiles][3] | terms [B][R][2] (SC, LM) | coef [B][R][2] | rows [B][3],  then floats  frames [B][frames_row]
struct SfWs {
    double *slabs, *terms, *coef, *rows;
    float* frames;
};

// The window table and delta P0 of (row, resolution): E0 and sum w^2 as a thread's groups of four samples (taps: the ones it has just
// written) in index order, fp32 squares added in fp64, then the fixed pairing - the same bits in every workgroup of the row, whatever
// the row's alignment (zeros past its end add exact zeros).  Returns false for a silent target (uniform over the workgroup).
__device__ __forceinline__ bool sf_floor(float* wtab, double (*red)[SL_T / 64], const float* __restrict__ yt, const SfRes& g, int T,
                                         double delta, float& dp0) {
    const int tid = threadIdx.x;
    double e0 = 0.0, w2 = 0.0, none = 0.0;
    for (int n = tid; n < g.N; n += SL_T) {
        const float w = stft_hann<float>(n, g.N, g.win);
        wtab[n] = w;
        w2 += (double)(w * w);
    }
    const bool vec = (T % 4 == 0) && aligned16(yt);
    for (int t = 4 * tid; t < T; t += 4 * SL_T) {
        const float4 v = ld_group(yt, t, T, vec);
        e0 += (double)(v.x * v.x); e0 += (double)(v.y * v.y); e0 += (double)(v.z * v.z); e0 += (double)(v.w * v.w);
    }
    sl_block_sum3(red, e0, w2, none);                                // its barriers also stand behind the table
    dp0 = (float)(delta * (w2 * e0 / (double)T));
    return e0 != 0.0;
}

// The packed spectra of FR = 1024 / M frames from f0 on: y^ in img[lf M ...], y in img[(FR + lf) M ...], lf = f - f0; bin k of a frame at
// fl_swz(k), slot 0 = (bin 0, bin N / 2).  Frames past F are zeros.  Returns with the image complete.
template <int M>
__device__ __forceinline__ void sf_spectra(cf* img, const float* wtab, const float* __restrict__ yp, const float* __restrict__ yt,
                                           const SfRes& g, int T, int f0) {
    constexpr int TG = M / 8, FR = 1024 / M;
    const int grp = threadIdx.x / TG, t = threadIdx.x % TG;
    const int lf = grp < FR ? grp : grp - FR, f = f0 + lf;
    const float* __restrict__ src = grp < FR ? yp : yt;
    cf* buf = img + grp * M;
    const int n_hi = g.n_lo + g.win, at0 = g.hop * f - M;            // sample index of tap 0, before the reflection
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int i = t + TG * e;
        float v[2] = {0.f, 0.f};
        if (f < g.F) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int n = 2 * i + s;
                if (n >= g.n_lo && n < n_hi) {
                    int j = at0 + n;                                 // in [-N/2, T + N/2): one reflection reaches [0, T) as T > N/2
                    if (j < 0) j = -j;
                    if (j >= T) j = 2 * (T - 1) - j;
                    v[s] = wtab[n] * src[j];
                }
            }
        }
        buf[fl_swz(i)] = {v[0], v[1]};
    }
    __syncthreads();
    fl_fft<M, -1>(buf, t);
    fl_split_fwd<M>(buf, t, TG);
    __syncthreads();
}

// one bin with the spectra (re_p, im_p) of y^ and (re_t, im_t) of y: the smoothed magnitudes and the two differences
struct SfBin {
    float mp, my, d, l;
};
__device__ __forceinline__ SfBin sf_bin(float re_p, float im_p, float re_t, float im_t, float dp0) {
#pragma clang fp contract(off)
    SfBin o;
    o.mp = sqrtf(re_p * re_p + im_p * im_p + dp0);
    o.my = sqrtf(re_t * re_t + im_t * im_t + dp0);
    o.d = o.mp - o.my;
    o.l = logf(o.mp) - logf(o.my);
    return o;
}

template <int M>
__device__ __forceinline__ void sf_analysis(cf* img, float* wtab, double (*red)[SL_T / 64], const float* __restrict__ yp,
                                            const float* __restrict__ yt, const SfRes& g, int T, int f0, double delta,
                                            double* __restrict__ slab) {
#pragma clang fp contract(off)
    constexpr int FR = 1024 / M;
    const int tid = threadIdx.x;
    float dp0;
    if (!sf_floor(wtab, red, yt, g, T, delta, dp0)) {
        if (tid == 0) { slab[0] = 0.0; slab[1] = 0.0; slab[2] = 0.0; }
        return;
    }
    sf_spectra<M>(img, wtab, yp, yt, g, T, f0);
    double s_d = 0.0, s_y = 0.0, s_l = 0.0;
    auto add = [&](const SfBin& o) { s_d += (double)(o.d * o.d); s_y += (double)(o.my * o.my); s_l += (double)(o.l * o.l); };
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                    // FR M = 1024 (frame, slot) pairs, four per thread
        const int q = tid + SL_T * e, lf = q / M, i = q % M;
        if (f0 + lf >= g.F) continue;
        const cf a = img[lf * M + fl_swz(i)], c = img[(FR + lf) * M + fl_swz(i)];
        if (i == 0) {
            add(sf_bin(a.x, 0.f, c.x, 0.f, dp0));
            add(sf_bin(a.y, 0.f, c.y, 0.f, dp0));
        } else {
            add(sf_bin(a.x, a.y, c.x, c.y, dp0));
        }
    }
    sl_block_sum3(red, s_d, s_y, s_l);
    if (tid == 0) { slab[0] = s_d; slab[1] = s_y; slab[2] = s_l; }
}

__global__ __launch_bounds__(SL_T) void slf_analysis_kernel(const float* __restrict__ wav_pred, const float* __restrict__ wav_true, SfPlan p,
                                                            double delta, SfWs ws) {
    __shared__ cf img[SF_IMG];
    __shared__ float wtab[SL_MAX_NFFT];
    __shared__ double red[3][SL_T / 64];
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    int local;
    const SfRes g = p.res[sl_find(p, &SfRes::tile0, tile, local)];
    const float* yp = wav_pred + (size_t)b * p.T;
    const float* yt = wav_true + (size_t)b * p.T;
    double* slab = ws.slabs + ((size_t)b * p.tiles + tile) * 3;
    const int f0 = local * (2048 / g.N);
    switch (g.N) {
        case 128: sf_analysis<64>(img, wtab, red, yp, yt, g, p.T, f0, delta, slab); break;
        case 256: sf_analysis<128>(img, wtab, red, yp, yt, g, p.T, f0, delta, slab); break;
        case 512: sf_analysis<256>(img, wtab, red, yp, yt, g, p.T, f0, delta, slab); break;
        default: sf_analysis<512>(img, wtab, red, yp, yt, g, p.T, f0, delta, slab); break;
    }
}

// frames[f][n - n_lo] = w[n] sum_k g[f,k] (Re X^[f,k] cos(2 pi k n / N) - Im X^[f,k] sin(2 pi k n / N)) for the non-zero taps
template <int M>
__device__ __forceinline__ void sf_adjoint(cf* img, float* wtab, double (*red)[SL_T / 64], const float* __restrict__ yp,
                                           const float* __restrict__ yt, const SfRes& g, int T, int f0, double delta, float ca, float cb,
                                           float* __restrict__ fr) {
#pragma clang fp contract(off)
    constexpr int TG = M / 8, FR = 1024 / M;
    const int tid = threadIdx.x;
    float dp0;
    if (!sf_floor(wtab, red, yt, g, T, delta, dp0)) return;          // not reached: the row is counted
    sf_spectra<M>(img, wtab, yp, yt, g, T, f0);
    const float inv_fk = (float)(1.0 / ((double)g.F * (double)g.K));
    // g = [ca 2 (M_y^ - M_y) + cb 2 (ln M_y^ - ln M_y) / (F K M_y^)] / M_y^
    auto gain = [&](const SfBin& o) { return (ca * (2.f * o.d) + cb * (2.f * o.l * inv_fk / o.mp)) / o.mp; };
#pragma unroll
    for (int e = 0; e < 4; ++e) {                                    // a thread rewrites the slots of y^ it has read itself
        const int q = tid + SL_T * e, lf = q / M, i = q % M;
        const cf a = img[lf * M + fl_swz(i)], c = img[(FR + lf) * M + fl_swz(i)];
        cf G;
        if (i == 0) {
            G = {gain(sf_bin(a.x, 0.f, c.x, 0.f, dp0)) * a.x, gain(sf_bin(a.y, 0.f, c.y, 0.f, dp0)) * a.y};
        } else {
            const float h = 0.5f * gain(sf_bin(a.x, a.y, c.x, c.y, dp0));
            G = {h * a.x, h * a.y};
        }
        img[lf * M + fl_swz(i)] = G;
    }
    __syncthreads();
    // every group runs the inverse in lockstep; those of y transform what is left in their images, which nobody reads
    const int grp = tid / TG, t = tid % TG;
    cf* buf = img + grp * M;
    fl_split_inv<M>(buf, t, TG);
    __syncthreads();
    fl_fft<M, 1>(buf, t);
    const int n_hi = g.n_lo + g.win;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int q = tid + SL_T * e, lf = q / M, i = q % M, f = f0 + lf;
        if (f >= g.F) continue;
        const cf z = img[lf * M + fl_swz(i)];
        float* __restrict__ o = fr + (size_t)f * g.win;
        const int n = 2 * i;
        if (n >= g.n_lo && n < n_hi) o[n - g.n_lo] = wtab[n] * z.x;
        if (n + 1 >= g.n_lo && n + 1 < n_hi) o[n + 1 - g.n_lo] = wtab[n + 1] * z.y;
    }
}

__global__ __launch_bounds__(SL_T) void slf_adjoint_kernel(const float* __restrict__ wav_pred, const float* __restrict__ wav_true, SfPlan p,
                                                           double delta, SfWs ws) {
    __shared__ cf img[SF_IMG];
    __shared__ float wtab[SL_MAX_NFFT];
    __shared__ double red[3][SL_T / 64];
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    if (ws.rows[3 * (size_t)b + 2] == 0.0) return;                   // a row that is not counted: the fold writes its zeros
    int local;
    const int r_of = sl_find(p, &SfRes::tile0, tile, local);
    const SfRes g = p.res[r_of];
    const float* yp = wav_pred + (size_t)b * p.T;
    const float* yt = wav_true + (size_t)b * p.T;
    const float ca = (float)ws.coef[2 * ((size_t)b * p.R + r_of)], cb = (float)ws.coef[2 * ((size_t)b * p.R + r_of) + 1];
    float* fr = ws.frames + (size_t)b * p.frames_row + g.frame0;
    const int f0 = local * (2048 / g.N);
    switch (g.N) {
        case 128: sf_adjoint<64>(img, wtab, red, yp, yt, g, p.T, f0, delta, ca, cb, fr); break;
        case 256: sf_adjoint<128>(img, wtab, red, yp, yt, g, p.T, f0, delta, ca, cb, fr); break;
        case 512: sf_adjoint<256>(img, wtab, red, yp, yt, g, p.T, f0, delta, ca, cb, fr); break;
        default: sf_adjoint<512>(img, wtab, red, yp, yt, g, p.T, f0, delta, ca, cb, fr); break;
    }
}

bool sf_supported(int T, int N, int win, int hop) {
    return (N == 128 || N == 256 || N == 512 || N == 1024) && win >= 2 && win <= N && hop >= 1 && T >= N / 2 + 1 && T <= SL_MAX_T;
}

// the plan of a call; the doubles and the floats of its workspace (false: not supported)
bool sf_plan(int B, int T, int R, const int* res, SfPlan* out, size_t& doubles, size_t& floats) {
    if (B <= 0 || R < 1 || R > SL_MAX_R || !res) return false;
    SfPlan p = {};
    p.R = R; p.B = B; p.T = T;
    long long tiles = 0, frames = 0;
    for (int r = 0; r < R; ++r) {
        const int N = res[3 * r], win = res[3 * r + 1], hop = res[3 * r + 2];
        if (!sf_supported(T, N, win, hop)) return false;
        SfRes& g = p.res[r];
        const int per = 2048 / N;
        sl_res_fill(g, T, N, win, hop, frames);
        g.ntiles = (g.F + per - 1) / per;
        g.tile0 = (int)tiles;
        tiles += g.ntiles;
    }
    if (tiles * B > 0x7fffffffLL || sl_fold_blocks(B, T) > 0x7fffffffLL) return false;              // the grids are one-dimensional
    p.tiles = (int)tiles; p.frames_row = frames;
    if (out) *out = p;
    doubles = sl_head_doubles(B, tiles, R);
    floats = (size_t)B * (size_t)frames;
    return true;
}

size_t sf_bytes(size_t doubles, size_t floats) { return doubles * sizeof(double) + ((floats + 1) / 2) * 2 * sizeof(float); }

}  // namespace

extern "C" {

int unetrir_spectral_loss_fft_supported(int T, int n_fft, int win_length, int hop_length) {
    return sf_supported(T, n_fft, win_length, hop_length) ? 1 : 0;
}

size_t unetrir_spectral_loss_fft_ws_bytes(int B, int T, int R, const int* res) {
    size_t d, f;
    return sf_plan(B, T, R, res, nullptr, d, f) ? sf_bytes(d, f) : 0;
}

int unetrir_spectral_loss_fft_f32(const float* wav_pred, const float* wav_true, int B, int T, int R, const int* res, double floor_db,
                                  double sc_weight, double log_weight, double weight, double inv_global_batch, int accumulate, float* dwav,
                                  double* spectral_out, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!sl_args_ok(wav_pred, wav_true, B, R, res, floor_db, sc_weight, log_weight, weight, inv_global_batch, accumulate, dwav,
                    spectral_out, ws))
        return UNETRIR_EINVAL;
    SfPlan p;
    size_t doubles, floats;
    if (!sf_plan(B, T, R, res, &p, doubles, floats)) return UNETRIR_EINVAL;
    if (ws_bytes < sf_bytes(doubles, floats)) return UNETRIR_EINVAL;
    SfWs w;
    w.frames = (float*)sl_head_carve(w, ws, B, p.tiles, R);
    const double delta = pow(10.0, -floor_db / 10.0), scale = weight * inv_global_batch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(slf_analysis_kernel, dim3((unsigned)(B * p.tiles)), dim3(SL_T), 0, s, wav_pred, wav_true, p, delta, w);
    hipLaunchKernelGGL(sl_finalize_kernel, dim3(1), dim3(SL_T), 0, s, p, sc_weight, log_weight, scale, w, spectral_out, loss_out);
    if (dwav) {
        hipLaunchKernelGGL(slf_adjoint_kernel, dim3((unsigned)(B * p.tiles)), dim3(SL_T), 0, s, wav_pred, wav_true, p, delta, w);
        hipLaunchKernelGGL(sl_fold_kernel, dim3((unsigned)sl_fold_blocks(B, T)), dim3(SL_T), 0, s, p, w, accumulate, dwav);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
