// istft_bwd.hip - the vector-Jacobian product of PostProcess (gfx950): for a cotangent dwav on the waveform y^ = PostProcess(pred) that
// unetrir_istft_features_f32(denormalize = 1) makes, dpred[b] = (d y^_b / d pred_b)^T dwav_b.  With it any loss on the waveform - the
// decay loss of decayloss.hip, or a torch expression behind features.PostProcess.differentiable - trains a model through an engine's
// backward(dpred=...).
//
// The math is the header of waveloss.hip with the residual taken out: u[t] = dwav[t] / env[t] where env[t] > tiny and 0 elsewhere,
// s_f[n] = hann(n) u[f hop + n - N/2], G_f[k] the DFT of s_f over its non-zero taps, dRe = c_k / N Re G, dIm = c_k / N Im G (c_k = 2,
// but c_k = 1 and dIm = 0 at k = 0 and k = N/2), then the chain rule through S = A e^{i phi}, A = (10^((100 a - 100)/20) - 1e-5) 128,
// phi = wrap(2 pi p - pi).  Rows >= n_bins and columns >= n_frames do not reach the waveform: structural zeros.
//
// One launch, one workgroup per (column, sample), no workspace and no atomics: the loader recomputes env[t] for each of its samples
// from the at most win / hop + 1 frames that reach it, in ascending frame order (the order of istft_feature_kernel's own envelope);
// fp64 inside, one rounding per output, every sum in a fixed order - two runs give the same bits and a sample's bits depend neither
// on B nor on its place in the batch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"
#include "stft_common.h"

namespace {

// the constants of features.hip
constexpr int IB_MAX_NFFT = 1024;
constexpr double IB_MD = 100.0;
constexpr double IB_EP = 1e-5;
constexpr double IB_REF = 128.0;
constexpr double IB_PI = 3.14159265358979323846;
constexpr double IB_TINY32 = 1.1754943508222875e-38;
constexpr double IB_LN10 = 2.30258509299404568402;

template <bool ACC>
__global__ __launch_bounds__(256) void istft_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ phase_ref,
                                                        const float* __restrict__ dwav, int H, int W, int n_frames, int n_fft, int win,
                                                        int hop, int T_out, float* __restrict__ dpred) {
    __shared__ double tw_c[IB_MAX_NFFT], tw_s[IB_MAX_NFFT], sg[IB_MAX_NFFT];
    const int f = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t o0 = ((size_t)b * 2 + 0) * H * W, o1 = ((size_t)b * 2 + 1) * H * W;
    const bool framed = f < n_frames;                    // uniform over the workgroup
    if (ACC && !framed) return;                          // structural zeros: left untouched
    const int nb = n_fft / 2 + 1, n_lo = (n_fft - win) / 2, n_hi = n_lo + win, mask = n_fft - 1;
    if (framed) {
        const float* __restrict__ db = dwav + (size_t)b * T_out;
        for (int n = tid; n < n_fft; n += 256) {
            double sn, cs;
            sincospi(2.0 * (double)n / (double)n_fft, &sn, &cs);
            tw_c[n] = cs; tw_s[n] = sn;
            const int i = f * hop + n - n_fft / 2;
            double v = 0.0;
            if (i >= 0 && i < T_out && n >= n_lo && n < n_hi) {
                // env[i]: the frames g with n_lo <= p - hop g < n_hi, ascending
                const int p = i + n_fft / 2;
                int g_lo = p - n_hi + 1 <= 0 ? 0 : (p - n_hi + 1 + hop - 1) / hop;
                int g_hi = (p - n_lo) / hop;
                if (g_hi > n_frames - 1) g_hi = n_frames - 1;
                double wss = 0.0;
                for (int g = g_lo; g <= g_hi; ++g) {
                    const double w = stft_hann<double>(p - hop * g, n_fft, win);
                    wss += w * w;
                }
                if (wss > IB_TINY32) v = stft_hann<double>(n, n_fft, win) * ((double)db[i] / wss);
            }
            sg[n] = v;
        }
        __syncthreads();
    }
    for (int k = tid; k < H; k += 256) {
        const size_t e = (size_t)k * W + f;
        const bool live = framed && k < nb;
        if (ACC && !live) continue;
        double g0 = 0.0, g1 = 0.0;
        if (live) {
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
            const double e10 = pow(10.0, (a * IB_MD - IB_MD) / 20.0), amp = (e10 - IB_EP) * IB_REF;
            double ph = (double)phf * 2.0 * IB_PI - IB_PI;
            const double v = ph + IB_PI;
            ph = v - floor(v / (2.0 * IB_PI)) * (2.0 * IB_PI) - IB_PI;
            double sn, cs;
            sincos(ph, &sn, &cs);
            g0 = (dre * cs + dim * sn) * (IB_REF * (IB_LN10 * IB_MD / 20.0)) * e10;
            g1 = 2.0 * IB_PI * (amp * (dim * cs - dre * sn));
        }
        if (ACC) {
            dpred[o0 + e] = (float)((double)dpred[o0 + e] + g0);
            dpred[o1 + e] = (float)((double)dpred[o1 + e] + g1);
        } else {
            dpred[o0 + e] = (float)g0;
            dpred[o1 + e] = (float)g1;
        }
    }
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

extern "C" {

int unetrir_istft_features_bwd_f32(const float* pred, const float* phase_ref, const float* dwav, int B, int H, int W, int n_bins,
                                   int n_frames, int n_fft, int win_length, int hop_length, int accumulate, float* dpred,
                                   unetrir_stream_t stream) {
    if (!pred || !dwav || !dpred || B <= 0 || B > 65535 || !pow2(n_fft) || n_fft < 4 || n_fft > IB_MAX_NFFT || win_length <= 0 ||
        win_length > n_fft || hop_length <= 0 || n_bins != n_fft / 2 + 1 || n_bins > H || n_frames < 2 || n_frames > W ||
        (long long)hop_length * n_frames + n_fft > 0x7fffffffLL)
        return UNETRIR_EINVAL;
    const int T = hop_length * (n_frames - 1);
    hipStream_t s = (hipStream_t)stream;
    if (accumulate)
        hipLaunchKernelGGL(istft_bwd_kernel<true>, dim3(n_frames, B), dim3(256), 0, s, pred, phase_ref, dwav, H, W, n_frames, n_fft,
                           win_length, hop_length, T, dpred);
    else
        hipLaunchKernelGGL(istft_bwd_kernel<false>, dim3(W, B), dim3(256), 0, s, pred, phase_ref, dwav, H, W, n_frames, n_fft,
                           win_length, hop_length, T, dpred);
    return (int)hipGetLastError();
}

}  // extern "C"
