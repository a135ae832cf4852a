// decayloss.hip - a loss on the energy decay curve (EDC, Schroeder's backward integral in dB) of a waveform and its gradient on the
// waveform (gfx950).  The figures a listener asks of a response - DRR, C50, centre time, EDT (acoustics.hip) - are all read off that
// curve; this file makes it trainable.  Per sample, fp32 waveforms y^ (the prediction) and y (the target) of length T, fp64 arithmetic:
//
//     S_y^[t] = sum_{s >= t} y^[s]^2      S_y[t] = sum_{s >= t} y[s]^2      E0 = S_y[0]      delta = 10^(-floor_db / 10)
//     c_y^[t] = 10 log10(S_y^[t] / E0 + delta)         c_y[t] = 10 log10(S_y[t] / E0 + delta)
//     Q_b = (1 / T) sum_t (c_y^[t] - c_y[t])^2         dB^2; a sample with E0 == 0 counts nothing, in loss and gradient
//     L   = weight inv_global_batch sum_b Q_b
//
// Both curves are normalised by the TARGET's energy, so a level error counts; the floor keeps every logarithm finite.
//
// The gradient.  dQ_b / dc_y^[t] = (2 / T) (c_y^[t] - c_y[t]);  dc_y^[t] / dS_y^[t] = (10 / ln 10) / (S_y^[t] + delta E0);
// dS_y^[t] / dy^[s] = 2 y^[s] for s >= t.  So with
//     g[t] = (2 / T) (c_y^[t] - c_y[t]) (10 / ln 10) / (S_y^[t] + delta E0)
//     dwav[b][s] = weight inv_global_batch 2 y^[s] sum_{t <= s} g[t]
// the curve is a suffix sum and its gradient a prefix sum.
//
// Two launches whatever B is, no atomics, every order fixed - two runs give the same bits, and a row's bits depend neither on B nor on
// its place in the batch:
//   1 decay_row_kernel       one workgroup per waveform, in the manner of acoustic_figures_kernel: thread t owns the contiguous run
//                            [t R, (t+1) R), R = 4 ceil(T / 4096) <= 16, held in registers (zeros past the end of the row add exact
//                            zeros to every sum).  The run's energies from its end; an exclusive suffix scan of the run sums over the
//                            workgroup (shuffles inside a wave, the waves above added in index order through LDS); E0 = S_y[0] from
//                            thread 0, formed exactly as S_y[t] is formed everywhere; then S[t] = (runs above) + (run so far) down the
//                            run with both curves, the squared difference and g[t]; an exclusive prefix scan of the runs' sums of g
//                            (shuffles, then the waves below in index order) and dwav up the run.  Writes (Q_b, counted) per row.
//   2 decay_finalize_kernel  one workgroup: decay_out = (sum_b Q_b, rows counted), loss_out[0] += L, in a fixed order
// One code path for every 1 <= T <= 16384 (threads past the end of the row hold empty runs).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"

namespace {

constexpr int DL_THREADS = 1024;
constexpr int DL_WAVES = DL_THREADS / 64;
constexpr int DL_RUN = 16;                                 // the longest run a thread keeps in registers
constexpr int DL_TMAX = DL_THREADS * DL_RUN;
constexpr double DL_10_LN10 = 4.34294481903251827651;      // 10 / ln 10

__global__ __launch_bounds__(DL_THREADS) void decay_row_kernel(const float* __restrict__ wav_pred, const float* __restrict__ wav_true,
                                                               int T, double delta, double scale, float* __restrict__ dwav,
                                                               double* __restrict__ rows) {
    __shared__ double tot_p[DL_WAVES], tot_t[DL_WAVES], tot_g[DL_WAVES], tot_q[DL_WAVES];
    __shared__ double e0_sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    const float* hp = wav_pred + b * T;
    const float* ht = wav_true + b * T;
    const bool vec_p = (T % 4 == 0) && aligned16(hp), vec_t = (T % 4 == 0) && aligned16(ht);
    const int R = 4 * ((T + 4 * DL_THREADS - 1) / (4 * DL_THREADS));
    const long long lo = (long long)tid * R;                          // the run is [lo, min(lo + R, T)), empty when lo >= T

    float xp[DL_RUN], xt[DL_RUN];
#pragma unroll
    for (int j = 0; j < DL_RUN; j += 4) {
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), c = a;
        if (j < R && lo + j < T) { a = ld_group(hp, lo + j, T, vec_p); c = ld_group(ht, lo + j, T, vec_t); }
        xp[j] = a.x; xp[j + 1] = a.y; xp[j + 2] = a.z; xp[j + 3] = a.w;
        xt[j] = c.x; xt[j + 1] = c.y; xt[j + 2] = c.z; xt[j + 3] = c.w;
    }

    // ---- the run's energies from its end, and the exclusive suffix scan of the run sums: above[t] = sum of run[u], u > t
    double run_p = 0.0, run_t = 0.0;
#pragma unroll
    for (int j = DL_RUN - 1; j >= 0; --j) {
        run_p += (double)xp[j] * (double)xp[j];
        run_t += (double)xt[j] * (double)xt[j];
    }
    double inc_p = run_p, inc_t = run_t;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double op = __shfl_down(inc_p, off, 64), ot = __shfl_down(inc_t, off, 64);
        if (lane + off < 64) { inc_p += op; inc_t += ot; }
    }
    double above_p = __shfl_down(inc_p, 1, 64), above_t = __shfl_down(inc_t, 1, 64);
    if (lane == 63) { above_p = 0.0; above_t = 0.0; }
    if (lane == 0) { tot_p[wave] = inc_p; tot_t[wave] = inc_t; }
    __syncthreads();
    double wp = 0.0, wt = 0.0;
    for (int w = DL_WAVES - 1; w > wave; --w) { wp += tot_p[w]; wt += tot_t[w]; }
    above_p += wp; above_t += wt;
    if (tid == 0) e0_sh = above_t + run_t;                            // S_y[0], the expression the walk below forms at t = 0
    __syncthreads();
    const double e0 = e0_sh;

    if (e0 == 0.0) {                                                  // a silent target: uniform over the workgroup
        if (dwav) {
#pragma unroll
            for (int j = 0; j < DL_RUN; ++j)
                if (j < R && lo + j < T) dwav[b * T + lo + j] = 0.f;
        }
        if (tid == 0) { rows[2 * b] = 0.0; rows[2 * b + 1] = 0.0; }
        return;
    }

    // ---- S[t] down the run: both curves, the squared difference and g[t]
    const double de0 = delta * e0, cg = (2.0 / (double)T) * DL_10_LN10;
    double g[DL_RUN];
    double part_p = 0.0, part_t = 0.0, q = 0.0;
#pragma unroll
    for (int j = DL_RUN - 1; j >= 0; --j) {
        g[j] = 0.0;
        if (j < R && lo + j < T) {
            part_p += (double)xp[j] * (double)xp[j];
            part_t += (double)xt[j] * (double)xt[j];
            const double sp = above_p + part_p, st = above_t + part_t;
            const double d = 10.0 * log10(sp / e0 + delta) - 10.0 * log10(st / e0 + delta);
            q += d * d;
            g[j] = cg * d / (sp + de0);
        }
    }
    // Q_b: lanes by a shuffle tree (fixed pairing), waves in index order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_down(q, off, 64);
    if (lane == 0) tot_q[wave] = q;

    if (dwav) {
        // exclusive prefix scan of the runs' sums of g: below[t] = sum of gs[u], u < t
        double gs = 0.0;
#pragma unroll
        for (int j = 0; j < DL_RUN; ++j) gs += g[j];
        double inc_g = gs;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(inc_g, off, 64);
            if (lane >= off) inc_g += o;
        }
        double below = __shfl_up(inc_g, 1, 64);
        if (lane == 0) below = 0.0;
        if (lane == 63) tot_g[wave] = inc_g;
        __syncthreads();
        double wg = 0.0;
        for (int w = 0; w < wave; ++w) wg += tot_g[w];
        below += wg;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < DL_RUN; ++j) {
            if (j < R && lo + j < T) {
                acc += g[j];
                dwav[b * T + lo + j] = (float)(scale * 2.0 * (double)xp[j] * (below + acc));
            }
        }
    } else {
        __syncthreads();
    }
    if (tid == 0) {
        double v = tot_q[0];
        for (int w = 1; w < DL_WAVES; ++w) v += tot_q[w];
        rows[2 * b] = v / (double)T;
        rows[2 * b + 1] = 1.0;
    }
}

__global__ __launch_bounds__(256) void decay_finalize_kernel(const double* __restrict__ rows, int B, double scale,
                                                             double* __restrict__ decay_out, float* __restrict__ loss_out) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    double sq = 0.0, sn = 0.0;
    for (int b = tid; b < B; b += 256) { sq += rows[2 * (long long)b]; sn += rows[2 * (long long)b + 1]; }
    red[0][tid] = sq; red[1][tid] = sn;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {               // fixed pairing order
        if (tid < st) { red[0][tid] += red[0][tid + st]; red[1][tid] += red[1][tid + st]; }
        __syncthreads();
    }
    if (tid == 0) {
        decay_out[0] = red[0][0]; decay_out[1] = red[1][0];
        if (loss_out) loss_out[0] += (float)(scale * red[0][0]);
    }
}

}  // namespace

extern "C" {

int unetrir_decay_loss_supported(int T) { return T >= 1 && T <= DL_TMAX ? 1 : 0; }

// ws: (Q_b, counted) fp64 per row
size_t unetrir_decay_loss_ws_bytes(int B, int T) {
    if (B <= 0 || !unetrir_decay_loss_supported(T)) return 0;
    return (size_t)B * 2 * sizeof(double);
}

int unetrir_decay_loss_f32(const float* wav_pred, const float* wav_true, int B, int T, double floor_db, double weight,
                           double inv_global_batch, float* dwav, double* decay_out, float* loss_out, void* ws, size_t ws_bytes,
                           unetrir_stream_t stream) {
    if (!wav_pred || !wav_true || !decay_out || !ws || B <= 0 || !unetrir_decay_loss_supported(T)) return UNETRIR_EINVAL;
    if (!isfinite(floor_db) || !(floor_db > 0.0) || floor_db > 200.0 || !(weight >= 0.0) || !isfinite(weight) ||
        !(inv_global_batch > 0.0) || !isfinite(inv_global_batch))
        return UNETRIR_EINVAL;
    const size_t need = unetrir_decay_loss_ws_bytes(B, T);
    if (need == 0 || ws_bytes < need || ((uintptr_t)ws & 7)) return UNETRIR_EINVAL;
    const double delta = pow(10.0, -floor_db / 10.0), scale = weight * inv_global_batch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(decay_row_kernel, dim3(B), dim3(DL_THREADS), 0, s, wav_pred, wav_true, T, delta, scale, dwav, (double*)ws);
    hipLaunchKernelGGL(decay_finalize_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, B, scale, decay_out, loss_out);
    return (int)hipGetLastError();
}

}  // extern "C"
