// acoustics.hip - room-acoustic figures of impulse responses on the device (gfx950): what a listener asks of a generated response
// and the reference's seven figures (evalmetrics.hip) do not answer - does the direct sound arrive on time, is the direct /
// reverberant and the early / late balance right, does the energy decay at the room's rate.
//
//   acoustic_figures_kernel     one workgroup per waveform h[0..T) (blockIdx.y picks wav_a / wav_b: one launch scores the predicted
//                               and the true waveform), fig[b][which][0..9]; fp64 from the fp32 samples, e = h*h:
//                                 0 n0       argmax |h|, lowest index on ties, |h| compared as fp32;  s = max(0, n0 - n_pre)
//                                 1 E_tot    S[s], with S[n] = sum_{k >= n} e[k] the Schroeder backward integral
//                                 2 E_dir    sum of e over s <= n <= min(T-1, n0 + n_dir)
//                                 3 E_early  sum of e over s <= n < min(T, s + n_early)
//                                 4 M1       sum_{n >= s} (n - s) e[n]
//                                 5 N_fit    #{n >= s : 10 S[n] >= E_tot}: the 0 .. -10 dB stretch of the decay curve
//                                 6 drr      10 log10(E_dir / (E_tot - E_dir))      dB
//                                 7 c50      10 log10(E_early / (E_tot - E_early))  dB
//                                 8 ts       M1 / E_tot / fs * 1e3                  centre time, ms
//                                 9 edt      -60 / slope, s;  slope = (N SkL - Sk SL) / (N Sk2 - Sk^2) * fs the least-squares line
//                                            through L[k] = 10 log10(S[s+k] / E_tot), k = 0..N-1, N = N_fit, Sk and Sk2 in closed
//                                            form; NaN when N < 2
//   acoustic_accumulate_kernel  one workgroup folds the errors of the (pred, true) pairs of a batch into acc[(G+1)][20] (row 0
//                               global, rows 1..G the rooms; per figure sum of errors, sum of pred values, sum of true values,
//                               count), walking the batch in index order.
//
// Degenerate rows follow IEEE arithmetic: an all-zero row gives NaN, no late energy +inf dB, a flat decay curve edt = -inf.
//
// Thread t owns the contiguous run [t R, (t+1) R) of its row, R = 4 ceil(T / 4096): whole groups of four samples, fetched as one
// 128-bit load when the row pitch and the pointer allow it and as bounds-checked scalars otherwise - the same samples in the same
// order either way.  Three walks over the run (the row is 38 KB at T = 9600: the second and third hit cache):
//   1  the arg-max: lanes by a shuffle tree under a total order (larger |h|, then lower index), waves in index order through LDS;
//   2  the energies of the run from its end, e[n] for n >= s only, with the window sums and M1; then an exclusive suffix scan of the
//      run sums over the workgroup (shuffles inside a wave, the waves above added in index order) and E_tot = S[s] from the thread
//      that owns s, formed exactly as walk 3 forms S[n];
//   3  the run again from its end: S[n] = (sum of the runs above) + (sum of the run so far), the range test and the regression sums.
// No atomics and no workspace; every order is fixed, so a waveform's row has the same bits in every run, in every batch position
// and in every batch size.  One code path for every T >= 1 (threads past the end of the row hold empty runs).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"

namespace {

constexpr int AC_THREADS = 1024;
constexpr int AC_WAVES = AC_THREADS / 64;
constexpr int AC_NSUM = 5;                       // E_dir, E_early, M1, sum L, sum k L
constexpr int AC_FIG = 10, AC_ERR = 5, AC_COLS = 4 * AC_ERR;

// (a, ia) before (b, ib): the larger magnitude, on ties the lower index - a total order, so the pairing of a reduction is free
__device__ __forceinline__ bool peak_before(float a, long long ia, float b, long long ib) { return a > b || (a == b && ia < ib); }

__global__ __launch_bounds__(AC_THREADS) void acoustic_figures_kernel(const float* __restrict__ wav_a, const float* __restrict__ wav_b,
                                                                      int T, int n_pre, int n_dir, int n_early, double fs,
                                                                      double* __restrict__ fig) {
    __shared__ float pk_v[AC_WAVES];
    __shared__ long long pk_i[AC_WAVES];
    __shared__ double wave_tot[AC_WAVES];
    __shared__ double etot_sh;
    __shared__ double red[AC_WAVES][AC_NSUM];
    __shared__ long long red_n[AC_WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int which = blockIdx.y, nwav = gridDim.y;
    const float* h = (which ? wav_b : wav_a) + (long long)blockIdx.x * T;
    const bool vec = (T % 4 == 0) && aligned16(h);
    const long long R = 4LL * (((long long)T + 4LL * AC_THREADS - 1) / (4LL * AC_THREADS));
    const long long lo = (long long)tid * R;                          // the run is [lo, hi), empty when lo >= T
    const long long hi = lo + R < T ? lo + R : T;

    // ---- walk 1: the peak
    float bv = -1.f;
    long long bi = 0x7fffffffffffffffLL;
    for (long long i = lo; i < hi; i += 4) {
        const float4 x = ld_group(h, i, T, vec);
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = fabsf(xv[j]);
            if (i + j < hi && a > bv) { bv = a; bi = i + j; }          // ascending index, strict: the lowest index of a tie stays
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const long long oi = __shfl_xor(bi, off, 64);
        if (peak_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { pk_v[wave] = bv; pk_i[wave] = bi; }
    __syncthreads();
    bv = pk_v[0]; bi = pk_i[0];
    for (int w = 1; w < AC_WAVES; ++w) {
        if (peak_before(pk_v[w], pk_i[w], bv, bi)) { bv = pk_v[w]; bi = pk_i[w]; }
    }
    const long long n0 = bi;                                           // thread 0 always holds a sample: n0 is in [0, T)
    const long long s = n0 > n_pre ? n0 - n_pre : 0;
    const long long dir_end = n0 + n_dir;                              // inclusive
    const long long early_end = s + n_early;                           // exclusive
    const long long first = lo > s ? lo : s;                           // the run's samples at or after s are [first, hi)

    // ---- walk 2: the run's energy from its end (samples before s take no part in any figure), window sums and M1
    double sum[AC_NSUM] = {0, 0, 0, 0, 0};
    double run = 0.0;
    for (long long i = hi - 1 - ((hi - 1 - lo) & 3); i >= lo && i + 3 >= first; i -= 4) {      // groups of the run, last first
        const float4 x = ld_group(h, i, T, vec);
        const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int j = 3; j >= 0; --j) {
            const long long n = i + j;
            if (n < hi && n >= first) {
                const double e = (double)xv[j] * (double)xv[j];
                run += e;
                if (n <= dir_end) sum[0] += e;
                if (n < early_end) sum[1] += e;
                sum[2] += (double)(n - s) * e;
            }
        }
    }
    // exclusive suffix scan of the run sums: above[t] = sum of run[u], u > t
    double incl = run;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_down(incl, off, 64);
        if (lane + off < 64) incl += o;
    }
    double above = __shfl_down(incl, 1, 64);
    if (lane == 63) above = 0.0;
    if (lane == 0) wave_tot[wave] = incl;
    __syncthreads();
    double waves_above = 0.0;
    for (int w = AC_WAVES - 1; w > wave; --w) waves_above += wave_tot[w];
    above += waves_above;
    if (s >= lo && s < hi) etot_sh = above + run;                      // S[s], the expression walk 3 forms at n = s
    __syncthreads();
    const double e_tot = etot_sh;

    // ---- walk 3: S[n] down the run, the 0 .. -10 dB range test and the regression sums.  S grows towards the start of the run, so
    // a run whose first sample fails the test holds no sample of the stretch.
    long long n_fit = 0;
    if (first < hi && 10.0 * (above + run) >= e_tot) {
        double part = 0.0;
        for (long long i = hi - 1 - ((hi - 1 - lo) & 3); i >= lo && i + 3 >= first; i -= 4) {
            const float4 x = ld_group(h, i, T, vec);
            const float xv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const long long n = i + j;
                if (n < hi && n >= first) {
                    part += (double)xv[j] * (double)xv[j];
                    const double S = above + part;
                    if (10.0 * S >= e_tot) {
                        const double L = 10.0 * log10(S / e_tot);
                        ++n_fit;
                        sum[3] += L;
                        sum[4] += (double)(n - s) * L;
                    }
                }
            }
        }
    }

    // lanes: shuffle tree (fixed pairing); waves: index order
#pragma unroll
    for (int k = 0; k < AC_NSUM; ++k) {
        double v = sum[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        sum[k] = v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n_fit += __shfl_down(n_fit, off, 64);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < AC_NSUM; ++k) red[wave][k] = sum[k];
        red_n[wave] = n_fit;
    }
    __syncthreads();
    if (tid != 0) return;
    double t[AC_NSUM];
#pragma unroll
    for (int k = 0; k < AC_NSUM; ++k) {
        double v = red[0][k];
        for (int w = 1; w < AC_WAVES; ++w) v += red[w][k];
        t[k] = v;
    }
    long long nf = red_n[0];
    for (int w = 1; w < AC_WAVES; ++w) nf += red_n[w];

    const double N = (double)nf;
    const double sk = N * (N - 1.0) / 2.0, sk2 = (N - 1.0) * N * (2.0 * N - 1.0) / 6.0;
    const double slope = (N * t[4] - sk * t[3]) / (N * sk2 - sk * sk) * fs;
    double* o = fig + ((long long)blockIdx.x * nwav + which) * AC_FIG;
    o[0] = (double)n0;
    o[1] = e_tot;
    o[2] = t[0];
    o[3] = t[1];
    o[4] = t[2];
    o[5] = N;
    o[6] = 10.0 * log10(t[0] / (e_tot - t[0]));
    o[7] = 10.0 * log10(t[1] / (e_tot - t[1]));
    o[8] = t[2] / e_tot / fs * 1e3;
    o[9] = nf < 2 ? __longlong_as_double(0x7ff8000000000000LL) : -60.0 / slope;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }          // false for NaN

// cell (row, col) of acc belongs to one thread, which walks the batch in index order: the sums do not depend on the launch geometry.
// col = 4 * figure + (0 error, 1 pred value, 2 true value, 3 count).  A figure of a pair counts when both sides are finite (edt:
// and positive); the other figures of that pair still count.
__global__ __launch_bounds__(256) void acoustic_accumulate_kernel(const double* __restrict__ fig, const int* __restrict__ group, int B,
                                                                  int G, double fs, double* __restrict__ err, double* __restrict__ acc) {
    for (int cell = threadIdx.x; cell < (G + 1) * AC_COLS; cell += blockDim.x) {
        const int row = cell / AC_COLS, col = cell % AC_COLS, f = col >> 2, kind = col & 3;
        double v = acc[cell];
        for (int b = 0; b < B; ++b) {
            const double* fp = fig + (long long)b * 2 * AC_FIG;
            const double* ft = fp + AC_FIG;
            double p, t, e;
            bool ok;
            if (f == 0) {
                p = fp[0] / fs * 1e3; t = ft[0] / fs * 1e3;
                e = fabs(fp[0] - ft[0]) / fs * 1e3;
                ok = true;
            } else {
                p = fp[5 + f]; t = ft[5 + f];
                e = f == 4 ? 100.0 * fabs(p - t) / t : fabs(p - t);
                ok = finite_d(p) && finite_d(t) && (f != 4 || (p > 0.0 && t > 0.0));
            }
            if (err && row == 0 && kind == 0) err[(long long)b * AC_ERR + f] = e;
            if (ok && (row == 0 || group[b] == row - 1)) v += kind == 0 ? e : kind == 1 ? p : kind == 2 ? t : 1.0;
        }
        acc[cell] = v;
    }
}

}  // namespace

int launch_acoustic_figures(const float* wav_a, const float* wav_b, int B, int T, int n_pre, int n_dir, int n_early, double fs,
                            double* fig, hipStream_t s) {
    hipLaunchKernelGGL(acoustic_figures_kernel, dim3(B, wav_b ? 2 : 1), dim3(AC_THREADS), 0, s, wav_a, wav_b, T, n_pre, n_dir, n_early,
                       fs, fig);
    return (int)hipGetLastError();
}

int launch_acoustic_accumulate(const double* fig, const int* group, int B, int G, double fs, double* err, double* acc, hipStream_t s) {
    hipLaunchKernelGGL(acoustic_accumulate_kernel, dim3(1), dim3(256), 0, s, fig, group, B, G, fs, err, acc);
    return (int)hipGetLastError();
}
