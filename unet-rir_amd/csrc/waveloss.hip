// waveloss.hip - a loss on the reconstructed waveform and its gradient with respect to the network's prediction (gfx950).
//
// The models are trained on the normalised spectrogram, yet graded on the impulse response PostProcess makes of it
// (rir_generation.py:207-223).  This file closes that loop: per sample b, with y^ = PostProcess(pred_b) - the arithmetic of
// istft_feature_kernel (features.hip) with denormalize = 1: un-pad to n_bins x n_frames, Normalizer.denormalize with python's phase
// wrap, the centred Hann inverse STFT divided by the squared-window envelope env[t] where that exceeds tiny - and y = wav_true[b],
//
//     E_b = sum_t w[t] (y^[t] - y[t])^2          w = time_weight, all ones when null            T = hop (n_frames - 1)
//     D_b = T (norm 0, "mse")   or   sum_t w[t] y[t]^2 (norm 1, "energy": the squared misalignment ratio of rir_generation.py:221-223)
//     L   = weight / global_batch * sum_b E_b / D_b          a sample with D_b == 0 contributes nothing, to L and to the gradient
//
// With phase_ref (the network input, NCHW; diff_gen, rir_generation.py:173-176) the reconstructed phase plane is pred[:,1] +
// phase_ref[:,1], summed in fp32 as the scoring kernel sums it (evalmetrics.hip).
//
// The gradient.  dL/dy^[t] = 2 weight w[t] (y^[t] - y[t]) / (global_batch D_b).  y^[t] = (sum_f hann(n) x_f[n]) / env[t] with n = t +
// N/2 - f hop and x_f = irfft(S[:, f]), so with
//     u[t]   = (dL/dy^[t]) / env[t]   where env[t] > tiny, 0 elsewhere (no non-zero tap reaches such a sample)
//     s_f[n] = hann(n) u[f hop + n - N/2],   zero outside [0, T)
// dL/dx_f[n] = s_f[n].  irfft is x[n] = (1/N) [X_0 + (-1)^n X_{N/2} + 2 sum_{0<k<N/2} (Re X_k cos(2 pi k n / N) - Im X_k sin(2 pi k n / N))]
// (the imaginary parts of bins 0 and N/2 are ignored), so with G_f[k] = sum_n s_f[n] e^{-2 pi i k n / N} - the analysis DFT of
// stft_feature_kernel with 'constant' padding, applied to u -
//     dL/dRe S[k,f] = c_k / N * Re G_f[k]        dL/dIm S[k,f] = c_k / N * Im G_f[k]
//     c_k = 2, except c_k = 1 and dL/dIm = 0 at k = 0 and k = N/2.
// S = A e^{i phi}:   dL/dA = dRe cos phi + dIm sin phi        dL/dphi = A (dIm cos phi - dRe sin phi)
// A = (10^((100 a - 100)/20) - 1e-5) 128, phi = wrap(2 pi p - pi) with a, p the two planes of pred:
//     dL/da = dL/dA * 128 * (ln 10 * 100 / 20) * 10^((100 a - 100)/20)
//     dL/dp = 2 pi dL/dphi          (the wrap has slope 1 and S is periodic in p: no special case)
// Rows >= n_bins and columns >= n_frames of the planes do not reach the waveform: their gradient is an exact zero.
//
// Fused spectrogram term.  The engines' backward(dpred=...) REPLACES the loss kernel's dL/dlogits, so the gradient of the existing
// loss on the prediction (sigmoid_loss_kernel, elementwise.hip) can ride along: with spec_target, over all H x W elements
//     dpred[:,0] += -2 alpha inv_norm (t0 - p0)        dpred[:,1] += -(1 - alpha) inv_norm 2 pi sin(ph) wgt
// t1 -= phase_ref (in fp32), wgt = phase_weight[column] and ph = pymod(2 pi (t1 - p1) + pi, 2 pi) - pi as there, but in fp64 like
// everything else here: with weight = 0 the result is the plain loss's dL/dpred up to that kernel's own fp32 roundings.
//
// Three launches whatever B is (two without dpred: the validation pass), all fp64 with one rounding per fp32 output, no atomics,
// every sum in a fixed order - two runs give the same bits and a sample's bits do not depend on B or on its place in the batch:
//   1 wave_synth_kernel     istft_feature_kernel's gather (one workgroup per 64 output samples, frames in order) + the residual:
//                           writes u[t] without the per-sample factor 2 weight / (global_batch D_b), one partial of sum w r^2 and
//                           one of sum w y^2 per workgroup, and (optionally) y^ as fp32 - bit for bit unetrir_istft_features_f32's
//   2 wave_finalize_kernel  one workgroup: E_b, D_b, the per-sample factors, wave_out = (sum_b E_b / D_b, sum_b E_b), loss_out[0] += L
//   3 wave_adjoint_kernel   one workgroup per (column, sample) over all W columns: the windowed segment of u in LDS, the direct DFT
//                           over its non-zero taps, the chain rule and the fused term; writes EVERY element of dpred, zeros included
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"
#include "stft_common.h"

namespace {

// the constants of features.hip; the window and the twiddle table are stft_common.h's
constexpr int WL_MAX_NFFT = 1024;
constexpr double WL_MD = 100.0;
constexpr double WL_EP = 1e-5;
constexpr double WL_REF = 128.0;
constexpr double WL_PI = 3.14159265358979323846;
constexpr double WL_TINY32 = 1.1754943508222875e-38;
constexpr double WL_LN10 = 2.30258509299404568402;
constexpr int WSEG = 64;                                // output samples per workgroup of the synthesis

// The loop of istft_feature_kernel, statement for statement (the fp32 waveform must come out with the same bits), then the residual.
__global__ __launch_bounds__(256) void wave_synth_kernel(const float* __restrict__ feat, const float* __restrict__ phase_ref, int H,
                                                         int W, int n_frames, int n_fft, int win, int hop,
                                                         const float* __restrict__ wav_true, const float* __restrict__ time_w,
                                                         int T_out, double* __restrict__ u, double* __restrict__ part,
                                                         float* __restrict__ wav) {
    __shared__ double tw_c[WL_MAX_NFFT], tw_s[WL_MAX_NFFT], xr[WL_MAX_NFFT / 2 + 1], xi[WL_MAX_NFFT / 2 + 1];
    __shared__ double red[4][WSEG];
    const int tid = threadIdx.x, s = tid & (WSEG - 1), kg = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * WSEG;
    const float* __restrict__ f_amp = feat + ((size_t)b * 2 + 0) * H * W;
    const float* __restrict__ f_ph = feat + ((size_t)b * 2 + 1) * H * W;
    const float* __restrict__ f_ref = phase_ref ? phase_ref + ((size_t)b * 2 + 1) * H * W : nullptr;
    const int nb = n_fft / 2 + 1, n_lo = (n_fft - win) / 2, n_hi = n_lo + win, mask = n_fft - 1;
    stft_tables(tw_c, tw_s, nullptr, n_fft, win, 256);
    const int p0 = t0 + n_fft / 2, p = p0 + s;
    int f_lo = (p0 - n_hi + 1 + hop - 1) / hop;
    if (p0 - n_hi + 1 <= 0) f_lo = 0;
    int f_hi = (p0 + WSEG - 1 - n_lo) / hop;
    if (f_hi > n_frames - 1) f_hi = n_frames - 1;
    double acc = 0.0, wss = 0.0;
    for (int f = f_lo; f <= f_hi; ++f) {
        __syncthreads();
        for (int k = tid; k < nb; k += 256) {
            float phf = f_ph[(size_t)k * W + f];
            if (f_ref) phf += f_ref[(size_t)k * W + f];
            double amp = (double)f_amp[(size_t)k * W + f], ph = (double)phf;
            amp = (pow(10.0, (amp * WL_MD - WL_MD) / 20.0) - WL_EP) * WL_REF;
            ph = ph * 2.0 * WL_PI - WL_PI;
            const double v = ph + WL_PI;
            ph = v - floor(v / (2.0 * WL_PI)) * (2.0 * WL_PI) - WL_PI;
            double sn, cs;
            sincos(ph, &sn, &cs);
            xr[k] = amp * cs; xi[k] = amp * sn;
        }
        __syncthreads();
        const int n = p - hop * f;
        if (n < n_lo || n >= n_hi) continue;
        const double w = stft_hann<double>(n, n_fft, win);
        double part_k = 0.0;
        for (int k = kg; k < nb; k += 4) {
            const int idx = (k * n) & mask;
            if (k == 0 || k == nb - 1) part_k += xr[k] * tw_c[idx];
            else part_k += 2.0 * (xr[k] * tw_c[idx] - xi[k] * tw_s[idx]);
        }
        acc += w * part_k / (double)n_fft;
        if (kg == 0) wss += w * w;
    }
    red[kg][s] = acc;
    __syncthreads();
    double e = 0.0, d = 0.0;
    if (kg == 0 && t0 + s < T_out) {
        double y = ((red[0][s] + red[1][s]) + red[2][s]) + red[3][s];
        if (wss > WL_TINY32) y /= wss;
        const size_t i = (size_t)b * T_out + t0 + s;
        if (wav) wav[i] = (float)y;
        const double yt = (double)wav_true[i], wt = time_w ? (double)time_w[t0 + s] : 1.0, r = y - yt;
        u[i] = wss > WL_TINY32 ? wt * r / wss : 0.0;
        e = wt * r * r; d = wt * yt * yt;
    }
    __syncthreads();                                     // every read of red above is done
    if (kg == 0) { red[0][s] = e; red[1][s] = d; }
    __syncthreads();
    for (int st = WSEG / 2; st > 0; st >>= 1) {          // fixed pairing order
        if (tid < st) { red[0][tid] += red[0][tid + st]; red[1][tid] += red[1][tid + st]; }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = part + ((size_t)b * gridDim.x + blockIdx.x) * 2;
        o[0] = red[0][0]; o[1] = red[1][0];
    }
}

__global__ __launch_bounds__(256) void wave_finalize_kernel(const double* __restrict__ part, int B, int nseg, int T_out, int norm,
                                                            double weight, double inv_gb, double* __restrict__ scale,
                                                            double* __restrict__ wave_out, float* __restrict__ loss_out) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    double sr = 0.0, se = 0.0;
    for (int b = tid; b < B; b += 256) {                 // a sample's sums: its own partials, in order
        const double* __restrict__ q = part + (size_t)b * nseg * 2;
        double E = 0.0, D = 0.0;
        for (int j = 0; j < nseg; ++j) { E += q[2 * j]; D += q[2 * j + 1]; }
        if (norm == 0) D = (double)T_out;
        const bool ok = D != 0.0;
        scale[b] = ok ? 2.0 * weight * inv_gb / D : 0.0;
        if (ok) sr += E / D;
        se += E;
    }
    red[0][tid] = sr; red[1][tid] = se;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {               // fixed pairing order
        if (tid < st) { red[0][tid] += red[0][tid + st]; red[1][tid] += red[1][tid + st]; }
        __syncthreads();
    }
    if (tid == 0) {
        wave_out[0] = red[0][0]; wave_out[1] = red[1][0];
        if (loss_out) loss_out[0] += (float)(weight * inv_gb * red[0][0]);
    }
}

__global__ __launch_bounds__(256) void wave_adjoint_kernel(const float* __restrict__ feat, const float* __restrict__ phase_ref,
                                                           const double* __restrict__ u, const double* __restrict__ scale, int H,
                                                           int W, int n_frames, int n_fft, int win, int hop, int T_out,
                                                           const float* __restrict__ target, const float* __restrict__ phase_w,
                                                           float alpha, float inv_norm, float* __restrict__ dpred) {
    __shared__ double tw_c[WL_MAX_NFFT], tw_s[WL_MAX_NFFT], sg[WL_MAX_NFFT];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t o0 = ((size_t)b * 2 + 0) * H * W, o1 = ((size_t)b * 2 + 1) * H * W;
    const bool framed = f < n_frames;                    // uniform over the workgroup
    if (framed) {
        const double sc = scale[b];
        const double* __restrict__ ub = u + (size_t)b * T_out;
        for (int n = tid; n < n_fft; n += 256) {
            double sn, cs;
            sincospi(2.0 * (double)n / (double)n_fft, &sn, &cs);
            tw_c[n] = cs; tw_s[n] = sn;
            const int i = f * hop + n - n_fft / 2;
            sg[n] = (i >= 0 && i < T_out) ? stft_hann<double>(n, n_fft, win) * (ub[i] * sc) : 0.0;
        }
        __syncthreads();
    }
    const int nb = n_fft / 2 + 1, n_lo = (n_fft - win) / 2, n_hi = n_lo + win, mask = n_fft - 1;
    for (int k = tid; k < H; k += 256) {
        const size_t e = (size_t)k * W + f;
        double g0 = 0.0, g1 = 0.0;
        if (framed && k < nb) {
            double re = 0.0, im = 0.0;
            int idx = (k * n_lo) & mask;
            for (int n = n_lo; n < n_hi; ++n) {
                const double v = sg[n];
                re += v * tw_c[idx];
                im -= v * tw_s[idx];
                idx = (idx + k) & mask;
            }
            const bool edge = k == 0 || k == nb - 1;
            const double dre = (edge ? 1.0 : 2.0) * re / (double)n_fft, dim = edge ? 0.0 : 2.0 * im / (double)n_fft;
            float phf = feat[o1 + e];
            if (phase_ref) phf += phase_ref[o1 + e];
            const double a = (double)feat[o0 + e];
            const double e10 = pow(10.0, (a * WL_MD - WL_MD) / 20.0), amp = (e10 - WL_EP) * WL_REF;
            double ph = (double)phf * 2.0 * WL_PI - WL_PI;
            const double v = ph + WL_PI;
            ph = v - floor(v / (2.0 * WL_PI)) * (2.0 * WL_PI) - WL_PI;
            double sn, cs;
            sincos(ph, &sn, &cs);
            g0 = (dre * cs + dim * sn) * (WL_REF * (WL_LN10 * WL_MD / 20.0)) * e10;
            g1 = 2.0 * WL_PI * (amp * (dim * cs - dre * sn));
        }
        if (target) {
            const float p0 = feat[o0 + e], p1 = feat[o1 + e], t0 = target[o0 + e];
            float t1 = target[o1 + e];
            if (phase_ref) t1 -= phase_ref[o1 + e];
            const double wgt = phase_w ? (double)phase_w[f] : 1.0;
            const double yt = (double)t1 * (2.0 * WL_PI) - WL_PI, yp = (double)p1 * (2.0 * WL_PI) - WL_PI;
            const double dd = (yt - yp) + WL_PI;
            const double ph = (dd - floor(dd / (2.0 * WL_PI)) * (2.0 * WL_PI)) - WL_PI;     // python-style modulo
            g0 += -2.0 * (double)alpha * (double)inv_norm * ((double)t0 - (double)p0);
            g1 += -(1.0 - (double)alpha) * (double)inv_norm * (2.0 * WL_PI) * sin(ph) * wgt;
        }
        dpred[o0 + e] = (float)g0;
        dpred[o1 + e] = (float)g1;
    }
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// ws: u fp64 [B][T], the partials fp64 [B][segments][2], the per-sample factors fp64 [B]
size_t ws_doubles(int B, int T, int nseg) { return (size_t)B * T + (size_t)B * nseg * 2 + (size_t)B; }

}  // namespace

extern "C" {

size_t unetrir_wave_loss_ws_bytes(int B, int n_frames, int hop_length) {
    if (B <= 0 || B > 65535 || n_frames < 2 || hop_length <= 0 || (long long)hop_length * n_frames + WL_MAX_NFFT > 0x7fffffffLL) return 0;
    const int T = hop_length * (n_frames - 1);
    return ws_doubles(B, T, (T + WSEG - 1) / WSEG) * sizeof(double);
}

int unetrir_wave_loss_f32(const float* pred, const float* phase_ref, const float* wav_true, const float* time_weight, int B, int H,
                          int W, int n_bins, int n_frames, int n_fft, int win_length, int hop_length, int norm, double weight,
                          double inv_global_batch, const float* spec_target, const float* phase_weight, float alpha, float inv_norm,
                          float* dpred, float* wav_pred, double* wave_out, float* loss_out, void* ws, size_t ws_bytes,
                          unetrir_stream_t stream) {
    if (!pred || !wav_true || !wave_out || !ws || B <= 0 || B > 65535 || !pow2(n_fft) || n_fft < 4 || n_fft > WL_MAX_NFFT ||
        win_length <= 0 || win_length > n_fft || hop_length <= 0 || n_bins != n_fft / 2 + 1 || n_bins > H || n_frames < 2 ||
        n_frames > W || (long long)hop_length * n_frames + n_fft > 0x7fffffffLL)
        return UNETRIR_EINVAL;
    if ((norm != 0 && norm != 1) || !(weight >= 0.0) || !isfinite(weight) || !(inv_global_batch > 0.0) || !isfinite(inv_global_batch))
        return UNETRIR_EINVAL;
    const size_t need = unetrir_wave_loss_ws_bytes(B, n_frames, hop_length);
    if (need == 0 || ws_bytes < need || ((uintptr_t)ws & 7)) return UNETRIR_EINVAL;
    const int T = hop_length * (n_frames - 1), nseg = (T + WSEG - 1) / WSEG;
    double* u = (double*)ws;
    double* part = u + (size_t)B * T;
    double* scale = part + (size_t)B * nseg * 2;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(wave_synth_kernel, dim3(nseg, B), dim3(256), 0, s, pred, phase_ref, H, W, n_frames, n_fft, win_length,
                       hop_length, wav_true, time_weight, T, u, part, wav_pred);
    hipLaunchKernelGGL(wave_finalize_kernel, dim3(1), dim3(256), 0, s, part, B, nseg, T, norm, weight, inv_global_batch, scale,
                       wave_out, loss_out);
    if (dpred)
        hipLaunchKernelGGL(wave_adjoint_kernel, dim3(W, B), dim3(256), 0, s, pred, phase_ref, u, scale, H, W, n_frames, n_fft,
                           win_length, hop_length, T, spec_target, phase_weight, alpha, inv_norm, dpred);
    return (int)hipGetLastError();
}

}  // extern "C"
