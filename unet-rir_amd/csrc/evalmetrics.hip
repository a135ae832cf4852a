// evalmetrics.hip - scoring of generated impulse responses on the device (gfx950): the per-sample figures of the reference's
// evaluation loop (rir_generation.py:185-225) and their per-room bookkeeping (:227-290, :311-357), without a host round trip.
//
//   eval_metrics_kernel     one workgroup per sample, ONE pass over pred / target (/ phase_ref) [2][H][W] and the two waveforms
//                           [T]: seven fp64 sums -> the seven figures of the sample, out[b][0..6]:
//                             0 mse_spec   mean over both planes of (target - pred)^2, always the RAW pred          (:197)
//                             1 mse_amp    mean over plane 0 of (target - pred)^2                                   (:195)
//                             2 phase      mean over plane 1 of 1 - cos(2 pi (target - p))                          (:36-40, :196)
//                                          p = pred, or pred + phase_ref (diff_gen, :174, :191; the sum is taken in fp32 as
//                                          the reference takes it, and is the plane the reconstruction is given)
//                             3 mis_amp    20 log10(|pred0 - target0|_2 / |target0|_2)                              (:203-205)
//                             4 mse_wav    mean of (wav_true - wav_pred)^2                                          (:215)
//                             5 mse_wav50  the same over the first min(n50, T) samples                              (:218)
//                             6 mis_wav    20 log10(|wav_pred - wav_true|_2 / |wav_true|_2)                         (:221-223)
//                           Everything runs over the whole padded plane, as the reference does.  Without waveforms 4-6 are NaN.
//   eval_accumulate_kernel  one workgroup folds out[B][7] into acc[(G+1)][8] (row 0 global, rows 1..G the rooms; columns 0-6
//                           running sums, column 7 the count), walking the batch in index order.  The dB figures are summed as
//                           dB per sample (:205-207, :316-317).
//
// Degenerate samples follow IEEE arithmetic where the reference raises: a zero numerator gives -inf dB (math.log10(0) is a
// ValueError there), a zero denominator +inf, both zero NaN.
//
// Differences, squares and the cosine are fp64 from the fp32 inputs.  Reductions have a fixed order and no atomics: element group
// g (four consecutive floats) always belongs to thread g mod 1024 whether it is fetched as one 128-bit load or, when the row pitch
// or the pointer does not allow that, as scalars; lanes are combined by a shuffle tree and the 16 waves in index order.  A
// sample's row therefore has the same bits in every run and in every batch it arrives in.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"

namespace {

constexpr int EVAL_THREADS = 1024;
constexpr int EVAL_WAVES = EVAL_THREADS / 64;
constexpr int EVAL_NSUM = 7;

__global__ __launch_bounds__(EVAL_THREADS) void eval_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ target,
                                                                    const float* __restrict__ phase_ref, int H, int W,
                                                                    const float* __restrict__ wav_pred,
                                                                    const float* __restrict__ wav_true, int T, int n50,
                                                                    double* __restrict__ out) {
    __shared__ double red[EVAL_WAVES][EVAL_NSUM];
    const int b = blockIdx.x, tid = threadIdx.x;
    const long long hw = (long long)H * W;
    const float* p0 = pred + (long long)b * 2 * hw;
    const float* t0 = target + (long long)b * 2 * hw;
    const float* r1 = phase_ref ? phase_ref + ((long long)b * 2 + 1) * hw : nullptr;
    const float *p1 = p0 + hw, *t1 = t0 + hw;

    // s[0] |t0 - p0|^2   s[1] |t1 - p1|^2 (raw)   s[2] sum of 1 - cos   s[3] |t0|^2   s[4] |wt - wp|^2   s[5] the same, first n50
    // s[6] |wt|^2
    double s[EVAL_NSUM] = {0, 0, 0, 0, 0, 0, 0};

    const bool vec_a = (hw % 4 == 0) && aligned16(p0) && aligned16(t0);                         // then p1 / t1 are aligned too
    const bool vec_r = (hw % 4 == 0) && (!r1 || aligned16(r1));
    for (long long i = 4LL * tid; i < hw; i += 4LL * EVAL_THREADS) {
        const float4 a = ld_group(p0, i, hw, vec_a), c = ld_group(t0, i, hw, vec_a);
        const float4 q = ld_group(p1, i, hw, vec_a), u = ld_group(t1, i, hw, vec_a);
        const float4 r = r1 ? ld_group(r1, i, hw, vec_r) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
        const float qv[4] = {q.x, q.y, q.z, q.w}, uv[4] = {u.x, u.y, u.z, u.w}, rv[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < hw) {
                const double da = (double)cv[j] - (double)av[j];
                const double dp = (double)uv[j] - (double)qv[j];
                const float ps = r1 ? qv[j] + rv[j] : qv[j];                  // fp32 sum: the plane the reconstruction receives
                s[0] += da * da;
                s[1] += dp * dp;
                s[2] += 1.0 - cospi(2.0 * ((double)uv[j] - (double)ps));
                s[3] += (double)cv[j] * (double)cv[j];
            }
        }
    }

    if (wav_pred) {
        const float* wp = wav_pred + (long long)b * T;
        const float* wt = wav_true + (long long)b * T;
        const bool vec_w = (T % 4 == 0) && aligned16(wp) && aligned16(wt);
        for (long long i = 4LL * tid; i < T; i += 4LL * EVAL_THREADS) {
            const float4 x = ld_group(wp, i, T, vec_w), y = ld_group(wt, i, T, vec_w);
            const float xv[4] = {x.x, x.y, x.z, x.w}, yv[4] = {y.x, y.y, y.z, y.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (i + j < T) {
                    const double d = (double)yv[j] - (double)xv[j];
                    const double d2 = d * d;
                    s[4] += d2;
                    if (i + j < n50) s[5] += d2;
                    s[6] += (double)yv[j] * (double)yv[j];
                }
            }
        }
    }

    // lanes: shuffle tree (fixed pairing); waves: index order
#pragma unroll
    for (int k = 0; k < EVAL_NSUM; ++k) {
        double v = s[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        s[k] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < EVAL_NSUM; ++k) red[tid >> 6][k] = s[k];
    }
    __syncthreads();
    if (tid != 0) return;
    double t[EVAL_NSUM];
#pragma unroll
    for (int k = 0; k < EVAL_NSUM; ++k) {
        double v = red[0][k];
        for (int w = 1; w < EVAL_WAVES; ++w) v += red[w][k];
        t[k] = v;
    }
    double* o = out + (long long)b * 7;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    o[0] = (t[0] + t[1]) / (2.0 * (double)hw);
    o[1] = t[0] / (double)hw;
    o[2] = t[2] / (double)hw;
    o[3] = 20.0 * log10(sqrt(t[0]) / sqrt(t[3]));
    if (wav_pred) {
        const int m50 = n50 < T ? n50 : T;
        o[4] = t[4] / (double)T;
        o[5] = t[5] / (double)m50;
        o[6] = 20.0 * log10(sqrt(t[4]) / sqrt(t[6]));
    } else {
        o[4] = nan; o[5] = nan; o[6] = nan;
    }
}

// cell (row, col) of acc belongs to one thread, which walks the batch in index order: the sums do not depend on the launch geometry
__global__ __launch_bounds__(256) void eval_accumulate_kernel(const double* __restrict__ out, const int* __restrict__ group, int B,
                                                              int G, double* __restrict__ acc) {
    for (int cell = threadIdx.x; cell < (G + 1) * 8; cell += blockDim.x) {
        const int row = cell >> 3, col = cell & 7;
        double v = acc[cell];
        for (int b = 0; b < B; ++b) {
            if (row == 0 || group[b] == row - 1) v += col < 7 ? out[(long long)b * 7 + col] : 1.0;
        }
        acc[cell] = v;
    }
}

}  // namespace

int launch_eval_metrics(const float* pred, const float* target, const float* phase_ref, int B, int H, int W, const float* wav_pred,
                        const float* wav_true, int T, int n50, double* out, hipStream_t s) {
    hipLaunchKernelGGL(eval_metrics_kernel, dim3(B), dim3(EVAL_THREADS), 0, s, pred, target, phase_ref, H, W, wav_pred, wav_true, T,
                       n50, out);
    return (int)hipGetLastError();
}

int launch_eval_accumulate(const double* out, const int* group, int B, int G, double* acc, hipStream_t s) {
    hipLaunchKernelGGL(eval_accumulate_kernel, dim3(1), dim3(256), 0, s, out, group, B, G, acc);
    return (int)hipGetLastError();
}
