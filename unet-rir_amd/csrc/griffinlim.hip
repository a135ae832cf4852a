// griffinlim.hip - magnitude-only reconstruction on the device (gfx950): librosa.griffinlim as PostProcess.griffinlim calls it
// (postprocess.py:47-50, :130-131; selected by `algorithm='gl'`, rir_generation.py:62, :137, :424), for a whole batch in one call.
//
// PARITY UNPINNED, like features.hip: the arithmetic lives in librosa, which the reference does not pin ((c) 2022 headers =>
// librosa 0.9.x).  What is built is librosa 0.9's published loop at its defaults (n_iter 32, momentum 0.99, init 'random',
// pad_mode 'reflect'):
//
//     S       = denormalised magnitude plane, un-padded to n_bins x n_frames (not clamped; the phase plane is ignored)
//     angles  = exp(2 pi i u), u uniform in [0, 1) per bin;   rebuilt = 0
//     n_iter times:  tprev = rebuilt;  rebuilt = stft(istft(S angles));
//                    angles = rebuilt - momentum / (1 + momentum) tprev;  angles /= |angles| + 1e-16
//     wav     = istft(S angles)
//
// with exactly the centred Hann pair of features.hip (same window, centring, `wss > tiny32` envelope rule, trimming).  librosa
// keeps `angles` in complex64; here ALL state and arithmetic are fp64 (twiddles from sincospi) and the waveform is rounded to
// fp32 once, so the result can be held to an fp64 restatement per element - the iteration does not amplify rounding.
//
// Both transforms are GEMMs against a twiddle matrix and run on v_mfma_f64_16x16x4_f64; the twiddle matrix itself never exists:
// each B fragment is looked up in the n_fft-entry LDS table at (k n) mod n_fft.
//
//   gl_init      S, S angles0                                                        (one launch)
//   gl_synth     16 frames x 64 window taps per workgroup: frames[f][n] = w[n] irfft(S angles)[f][n]     } n_iter + 1 launches
//   gl_analysis  16 frames x 64 bins per workgroup.  Its loader overlap-adds `frames` into the waveform sample each tap needs
//                (a gather in fixed frame order, the envelope rule, the reflected edge) - the intermediate waveform is never
//                stored; its epilogue is the angle update and the product with S for the next synthesis       } n_iter launches
//   gl_ola       the last overlap-add, rounded to fp32                                                   (one launch)
//
// 2 n_iter + 3 launches whatever B is; no atomics and fixed summation orders, so two runs are bit-identical; nothing is
// allocated, cleared or waited for, so the call can be captured in a HIP graph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "kernels.h"
#include "griffinlim_common.h"
#include "stft_common.h"

namespace {

constexpr int GL_MAX_NFFT = 1024;
constexpr int GL_TM = 16;                     // frames per workgroup = rows of one MFMA tile
constexpr int GL_KC = 128;                    // K elements staged in LDS at a time
constexpr int GL_LD = GL_KC + 4;              // LDS row stride in doubles: 16 rows land 8 banks apart (2-way, the b64 minimum)
constexpr int GL_T = 256;                     // 4 waves, one 16-column tile each

typedef double gl_d4 __attribute__((ext_vector_type(4)));

__global__ void uniform_kernel(float* __restrict__ out, long long n, unsigned long long seed, unsigned long long step) {
    const unsigned long long key = gl_uniform_key(seed, step);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = gl_uniform_at(key, i);
}

struct GlGeom {
    int B, H, W, n_bins, n_frames, n_fft, win, hop, T_out;
};

// S[b][f][k] and spec = S exp(2 pi i u) as two planes [b][f][k]; u is init_phase[b][k][f] or element (b n_bins + k) n_frames + f
// of draw (seed, draw) - the same element unetrir_uniform_f32 writes into a [B][n_bins][n_frames] tensor.
__global__ __launch_bounds__(256) void gl_init_kernel(const float* __restrict__ feat, GlGeom g, int denormalize,
                                                      const float* __restrict__ init_phase, unsigned long long seed,
                                                      unsigned long long draw, double* __restrict__ S, double* __restrict__ spec_re,
                                                      double* __restrict__ spec_im) {
    const unsigned long long key = gl_uniform_key(seed, draw);
    const long long n = (long long)g.B * g.n_frames * g.n_bins;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(e % g.n_bins);
        const long long bf = e / g.n_bins;
        const int f = (int)(bf % g.n_frames), b = (int)(bf / g.n_frames);
        double amp = (double)feat[(((size_t)b * 2) * g.H + k) * g.W + f];
        if (denormalize) amp = (pow(10.0, (amp * GL_MD - GL_MD) / 20.0) - GL_EP) * GL_REF;
        const long long i = ((long long)b * g.n_bins + k) * g.n_frames + f;
        const float u = init_phase ? init_phase[i] : gl_uniform_at(key, i);
        double sn, cs;
        sincospi(2.0 * (double)u, &sn, &cs);
        S[e] = amp;
        spec_re[e] = amp * cs;
        spec_im[e] = amp * sn;
    }
}

// Synthesis: frames[b][f][n - n_lo] = w[n] / N * sum_k c_k (Re X[f][k] cos(2 pi k n / N) - Im X[f][k] sin(2 pi k n / N)) for the
// non-zero window taps n in [n_lo, n_lo + win); c_k = 1 for k = 0 and N/2, else 2 - numpy.fft.irfft, which ignores the imaginary
// parts of those two bins (their sines are exact zeros in the table).  A = X (16 frames x K bins, re and im), B = the twiddles.
// grid (frame tiles, B, groups of 4 tap tiles); wave w owns taps n_lo + 16 (4 blockIdx.z + w) ... + 15.
__global__ __launch_bounds__(GL_T) void gl_synth_kernel(const double* __restrict__ spec_re, const double* __restrict__ spec_im, GlGeom g,
                                                        double* __restrict__ frames) {
    __shared__ double tw_c[GL_MAX_NFFT], tw_s[GL_MAX_NFFT], xr[GL_TM * GL_LD], xi[GL_TM * GL_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, f0 = blockIdx.x * GL_TM;
    const int n_lo = (g.n_fft - g.win) / 2, n_hi = n_lo + g.win, mask = g.n_fft - 1;
    const int n = n_lo + (blockIdx.z * 4 + wave) * 16 + row;          // this lane's column: a window tap (may be >= n_hi: not stored)
    stft_tables(tw_c, tw_s, nullptr, g.n_fft, g.win, blockDim.x);
    gl_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < g.n_bins; kc += GL_KC) {
        __syncthreads();                                             // the previous chunk is no longer read (first pass: tables)
        for (int e = tid; e < GL_TM * GL_KC; e += GL_T) {
            const int r = e / GL_KC, kk = e % GL_KC, k = kc + kk, f = f0 + r;
            double vr = 0.0, vi = 0.0;
            if (k < g.n_bins && f < g.n_frames) {
                const size_t src = ((size_t)b * g.n_frames + f) * g.n_bins + k;
                vr = spec_re[src]; vi = spec_im[src];
            }
            xr[r * GL_LD + kk] = vr; xi[r * GL_LD + kk] = vi;
        }
        __syncthreads();
        const int valid = g.n_bins - kc < GL_KC ? g.n_bins - kc : GL_KC;
        const int steps = (valid + 3) >> 2;
        for (int s = 0; s < steps; ++s) {
            const int kk = 4 * s + kq, k = kc + kk;
            const double ck = k >= g.n_bins ? 0.0 : ((k == 0 || k == g.n_bins - 1) ? 1.0 : 2.0);
            const int idx = (int)(((long long)k * n) & mask);
            const double ar = xr[row * GL_LD + kk], ai = xi[row * GL_LD + kk];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, ck * tw_c[idx], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, -ck * tw_s[idx], acc, 0, 0, 0);
        }
    }
    if (n < n_hi) {
        const double w = stft_hann<double>(n, g.n_fft, g.win) / (double)g.n_fft;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 r
            const int f = f0 + kq + 4 * r;
            if (f < g.n_frames) frames[((size_t)b * g.n_frames + f) * g.win + (n - n_lo)] = w * acc[r];
        }
    }
}

// librosa.istft's sample at padded coordinate q (= output index + n_fft/2) from the windowed frames: sum over the frames whose
// non-zero taps reach q, in frame order, divided by the squared-window envelope where that exceeds tiny32.
__device__ __forceinline__ double gl_ola_sample(const double* __restrict__ fr_b, const double* wtab, int q, int n_lo, int win, int hop,
                                                int n_frames) {
    int g_lo, g_hi;
    stft_frame_range<false>(q, n_lo, win, hop, n_frames, g_lo, g_hi);
    double acc = 0.0, wss = 0.0;
    for (int gi = g_lo; gi <= g_hi; ++gi) {
        const int m = q - hop * gi;                                  // tap of frame gi, in [n_lo, n_hi)
        const double w = wtab[m];
        acc += fr_b[(size_t)gi * win + (m - n_lo)];
        wss += w * w;
    }
    return wss > GL_TINY32 ? acc / wss : acc;
}

// Analysis + angle update: rebuilt[f][k] = sum_n w[n] y_pad[hop f + n] exp(-2 pi i k n / N) over the non-zero taps, y the
// overlap-added waveform (length T_out) padded by N/2 each side ('reflect' as numpy.pad does it, or zeros).  A = windowed samples
// (16 frames x K taps), B = twiddles.  Epilogue: angles = rebuilt - alpha tprev (tprev = 0 in the first pass), / (|.| + 1e-16),
// spec = S angles.  grid (frame tiles, B, groups of 4 bin tiles); wave w owns bins 16 (4 blockIdx.z + w) ... + 15.
__global__ __launch_bounds__(GL_T) void gl_analysis_kernel(const double* __restrict__ frames, GlGeom g, int pad_mode, int first, double alpha,
                                                           const double* __restrict__ S, const double* __restrict__ prev_re,
                                                           const double* __restrict__ prev_im, double* __restrict__ cur_re,
                                                           double* __restrict__ cur_im, double* __restrict__ spec_re,
                                                           double* __restrict__ spec_im) {
    __shared__ double tw_c[GL_MAX_NFFT], tw_s[GL_MAX_NFFT], wtab[GL_MAX_NFFT], xw[GL_TM * GL_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kq = lane >> 4;
    const int b = blockIdx.y, f0 = blockIdx.x * GL_TM;
    const int n_lo = (g.n_fft - g.win) / 2, n_hi = n_lo + g.win, mask = g.n_fft - 1, half = g.n_fft / 2;
    const int k = (blockIdx.z * 4 + wave) * 16 + row;                // this lane's column: a bin (may be >= n_bins: not stored)
    const double* __restrict__ fr_b = frames + (size_t)b * g.n_frames * g.win;
    const long long period = 2LL * (g.T_out - 1);
    stft_tables(tw_c, tw_s, wtab, g.n_fft, g.win, blockDim.x);
    gl_d4 acc_re = {0.0, 0.0, 0.0, 0.0}, acc_im = {0.0, 0.0, 0.0, 0.0};
    for (int tc = 0; tc < g.win; tc += GL_KC) {
        __syncthreads();                                             // the previous chunk is no longer read (first pass: tables)
        for (int e = tid; e < GL_TM * GL_KC; e += GL_T) {
            const int r = e / GL_KC, j = e % GL_KC, n = n_lo + tc + j, f = f0 + r;
            double v = 0.0;
            if (n < n_hi && f < g.n_frames) {
                long long i = (long long)g.hop * f + n - half;       // sample index in the unpadded waveform
                bool inside = i >= 0 && i < g.T_out;
                if (!inside && pad_mode == 0) {                      // numpy 'reflect' of any depth: period 2 (T - 1), edge not repeated
                    if (period == 0) i = 0;
                    else {
                        i %= period;
                        if (i < 0) i += period;
                        if (i >= g.T_out) i = period - i;
                    }
                    inside = true;
                }
                if (inside) v = wtab[n] * gl_ola_sample(fr_b, wtab, (int)i + half, n_lo, g.win, g.hop, g.n_frames);
            }
            xw[r * GL_LD + j] = v;
        }
        __syncthreads();
        const int valid = g.win - tc < GL_KC ? g.win - tc : GL_KC;
        const int steps = (valid + 3) >> 2;
        for (int s = 0; s < steps; ++s) {
            const int j = 4 * s + kq, n = n_lo + tc + j;             // taps past n_hi were staged as zeros
            const int idx = (int)(((long long)k * n) & mask);
            const double a = xw[row * GL_LD + j];
            acc_re = __builtin_amdgcn_mfma_f64_16x16x4f64(a, tw_c[idx], acc_re, 0, 0, 0);
            acc_im = __builtin_amdgcn_mfma_f64_16x16x4f64(a, -tw_s[idx], acc_im, 0, 0, 0);
        }
    }
    if (k < g.n_bins) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 r
            const int f = f0 + kq + 4 * r;
            if (f < g.n_frames) {
                const size_t e = ((size_t)b * g.n_frames + f) * g.n_bins + k;
                const double re = acc_re[r], im = acc_im[r];
                cur_re[e] = re; cur_im[e] = im;
                double ar = re, ai = im;
                if (!first) { ar -= alpha * prev_re[e]; ai -= alpha * prev_im[e]; }
                const double d = hypot(ar, ai) + 1e-16;
                const double s = S[e];
                spec_re[e] = s * (ar / d);
                spec_im[e] = s * (ai / d);
            }
        }
    }
}

// the last overlap-add: wav[b][t] = (float) istft sample t
__global__ __launch_bounds__(256) void gl_ola_kernel(const double* __restrict__ frames, GlGeom g, float* __restrict__ wav) {
    __shared__ double wtab[GL_MAX_NFFT];
    for (int n = threadIdx.x; n < g.n_fft; n += blockDim.x) wtab[n] = stft_hann<double>(n, g.n_fft, g.win);
    __syncthreads();
    const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= g.T_out) return;
    const int n_lo = (g.n_fft - g.win) / 2;
    const double y = gl_ola_sample(frames + (size_t)b * g.n_frames * g.win, wtab, t + g.n_fft / 2, n_lo, g.win, g.hop, g.n_frames);
    wav[(size_t)b * g.T_out + t] = (float)y;
}

bool gl_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

bool gl_geometry_ok(int B, int n_bins, int n_frames, int n_fft) {
    return B > 0 && B <= 65535 && gl_pow2(n_fft) && n_fft >= 4 && n_fft <= GL_MAX_NFFT && n_bins == n_fft / 2 + 1 && n_frames >= 2;
}

// workspace in doubles: S, spec (2 planes), rebuilt x 2 (2 planes each) over B n_frames n_bins, then the windowed frames
// B n_frames n_fft (win_length <= n_fft taps are used)
size_t gl_plane(int B, int n_bins, int n_frames) { return (size_t)B * n_frames * n_bins; }

unsigned gl_grid(long long n) {
    long long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

}  // namespace

extern "C" {

int unetrir_uniform_f32(float* out, long long n, unsigned long long seed, unsigned long long step, unetrir_stream_t stream) {
    if (!out || n <= 0) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(uniform_kernel, dim3(gl_grid(n)), dim3(256), 0, (hipStream_t)stream, out, n, seed, step);
    return (int)hipGetLastError();
}

size_t unetrir_griffinlim_ws_bytes(int B, int n_bins, int n_frames, int n_fft) {
    if (!gl_geometry_ok(B, n_bins, n_frames, n_fft)) return 0;
    return (7 * gl_plane(B, n_bins, n_frames) + (size_t)B * n_frames * n_fft) * sizeof(double);
}

int unetrir_griffinlim_f32(const float* feat, int B, int H, int W, int n_bins, int n_frames, int n_fft, int win_length, int hop_length,
                           int pad_mode, int denormalize, int n_iter, float momentum, const float* init_phase, unsigned long long seed,
                           unsigned long long draw, float* wav, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!feat || !wav || !ws || ((uintptr_t)ws & 7) || !gl_geometry_ok(B, n_bins, n_frames, n_fft) || win_length <= 0 ||
        win_length > n_fft || hop_length <= 0 || n_bins > H || n_frames > W ||
        (long long)hop_length * n_frames + n_fft > 0x7fffffffLL || n_iter < 0 || !(momentum >= 0.f) || !isfinite(momentum) ||
        (pad_mode != 0 && pad_mode != 1) || ws_bytes < unetrir_griffinlim_ws_bytes(B, n_bins, n_frames, n_fft))
        return UNETRIR_EINVAL;
    const GlGeom g = {B, H, W, n_bins, n_frames, n_fft, win_length, hop_length, hop_length * (n_frames - 1)};
    const size_t P = gl_plane(B, n_bins, n_frames);
    double* S = (double*)ws;
    double* spec_re = S + P;
    double* spec_im = S + 2 * P;
    double* reb[2] = {S + 3 * P, S + 5 * P};                         // rebuilt / tprev ping-pong, planes (re, im)
    double* frames = S + 7 * P;
    hipStream_t s = (hipStream_t)stream;
    const double m = gl_decimal(momentum), alpha = m / (1.0 + m);
    const unsigned ftiles = (unsigned)((n_frames + GL_TM - 1) / GL_TM);
    const dim3 grid_syn(ftiles, B, (unsigned)((win_length + 63) / 64)), grid_ana(ftiles, B, (unsigned)((n_bins + 63) / 64));

    hipLaunchKernelGGL(gl_init_kernel, dim3(gl_grid((long long)P)), dim3(256), 0, s, feat, g, denormalize, init_phase, seed, draw, S, spec_re,
                       spec_im);
    for (int it = 0; it < n_iter; ++it) {
        double* cur = reb[it & 1];
        double* prev = reb[(it & 1) ^ 1];
        hipLaunchKernelGGL(gl_synth_kernel, grid_syn, dim3(GL_T), 0, s, spec_re, spec_im, g, frames);
        hipLaunchKernelGGL(gl_analysis_kernel, grid_ana, dim3(GL_T), 0, s, frames, g, pad_mode, (int)(it == 0), alpha, S, prev, prev + P, cur,
                           cur + P, spec_re, spec_im);
    }
    hipLaunchKernelGGL(gl_synth_kernel, grid_syn, dim3(GL_T), 0, s, spec_re, spec_im, g, frames);
    hipLaunchKernelGGL(gl_ola_kernel, dim3((unsigned)((g.T_out + 255) / 256), B), dim3(256), 0, s, frames, g, wav);
    return (int)hipGetLastError();
}

}  // extern "C"
