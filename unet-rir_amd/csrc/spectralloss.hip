// spectralloss.hip - the multi-resolution STFT loss (squared spectral convergence + squared log-magnitude distance) of a waveform against
// a target and its gradient on the waveform (gfx950).  The networks predict amplitude and phase as two planes at ONE resolution; a pair
// that is the STFT of no signal costs nothing under the spectrogram loss.  Looked at through other windows it shows at once, and a
// magnitude loss on the reconstructed waveform at those resolutions penalises exactly that.
//
// The definition.  fp32 waveforms y^ (the prediction) and y (the target) [B][T]; R resolutions (n_fft N, win_length, hop_length h), each
// with the analysis transform of features.hip: periodic Hann of win_length samples centred in N zeros (left pad (N - win) / 2), centred
// frames with REFLECT padding of N / 2 each side, F = 1 + T / h frames, one-sided bins K = N / 2 + 1, no mean removal, no
// normalisation.  fp64 arithmetic.  Per row b and resolution r:
//
//     E0_b     = sum_t y_b[t]^2                         a row with E0 == 0 counts nothing: zeros in its gradient, nothing in any sum
//     P0       = (sum_n w_r[n]^2) E0_b / T              the power a bin would carry with the target's energy spread evenly
//     delta    = 10^(-floor_db / 10)
//     M_x[f,k] = sqrt(|X[f,k]|^2 + delta P0)            one smoothed magnitude for both terms: >= sqrt(delta P0) > 0
//     SC_{b,r} = sum_{f,k} (M_y^ - M_y)^2 / sum_{f,k} M_y^2
//     LM_{b,r} = (1 / (F K)) sum_{f,k} (ln M_y^ - ln M_y)^2
//     Q_b      = (1 / R) sum_r (sc_weight SC_{b,r} + log_weight LM_{b,r})
//     L        = weight inv_global_batch sum_b Q_b
//
// The gradient, with c = weight inv_global_batch / R:
//
//     g[f,k]   = c [ sc_weight 2 (M_y^ - M_y) / sum M_y^2  +  log_weight 2 (ln M_y^ - ln M_y) / (F K M_y^) ] / M_y^
//     dRe[f,k] = g Re X^[f,k],   dIm[f,k] = g Im X^[f,k]
//     p[j]     = sum_f w[j - f h] sum_k (dRe[f,k] cos(2 pi k n / N) - dIm[f,k] sin(2 pi k n / N)),  n = j - f h in [0, N)   (padded j)
//     dwav[t]  = p[t + N/2] + the padded positions that reflect onto t: j = N/2 - t (1 <= t <= N/2) and j = 2 (T - 1) - t + N/2
//                (T - 1 - N/2 <= t <= T - 2), summed over the resolutions in index order.
//
// Four launches for loss and gradient whatever B and R are, two for the loss alone:
//   1 sl_analysis_kernel  16 frames x 64 bins of one (row, resolution) per workgroup, y^ and y together (bin N/2, which is real, rides in
//                         the idle imaginary part of bin 0's column: N/2 columns, no tile for one bin).  The loader builds the windowed,
//                         reflected frames in LDS; the DFT runs on v_mfma_f64_16x16x4_f64 against the cos / sin table of N entries in
//                         LDS, read at (k n) mod N (gl_analysis_kernel's structure).  E0_b and sum w^2 are recomputed per workgroup in a
//                         fixed order (every workgroup of a row forms the same bits).  The epilogue forms M_y^, M_y, the three partial
//                         sums of the workgroup (a slab in the workspace) and, per bin, Re X^, Im X^ and the two factors of g that do
//                         not need the row-wide sum:  a = 2 (M_y^ - M_y) / M_y^,  q = 2 (ln M_y^ - ln M_y) / (F K M_y^^2).
//   2 sl_finalize_kernel  (spectralloss_common.h: the FFT form's too) one workgroup: the slabs of each (b, r) in index order -> SC, LM
//                         and the two scalars that scale the gradient; Q_b over r in index order; spectral_out; loss_out[0] += (float) L.
//   3 sl_synth_kernel     16 frames x 64 window taps per workgroup: the loader forms dRe, dIm from the four planes and the two scalars,
//                         the GEMM against the same table gives frames[f][n] = w[n] sum_k (dRe cos - dIm sin) over the non-zero taps.
//   4 sl_fold_kernel      (spectralloss_common.h: the FFT form's too) gather: one thread owns one output sample; per resolution in
//                         index order the frames that reach t + N/2 and the reflected positions, each in ascending frame order; one
//                         rounding to fp32 (or (float)((double) dwav + g)).
// No atomics, every summation order fixed: two runs give the same bits, and a row's bits depend neither on B nor on its place in the
// batch.  Nothing is allocated, cleared or waited for, so the call can be captured in a HIP graph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"
#include "spectralloss_common.h"

namespace {

constexpr int SL_MIN_NFFT = 16;
constexpr int SL_TM = 16;                     // frames per workgroup = rows of one MFMA tile
constexpr int SL_TN = 64;                     // columns per workgroup: one 16-column tile per wave
constexpr int SL_KC = 128;                    // reduction elements staged in LDS at a time
constexpr int SL_LD = SL_KC + 4;              // LDS row stride in doubles (griffinlim.hip: 16 rows land 8 banks apart)

typedef double sl_d4 __attribute__((ext_vector_type(4)));

struct SlRes {
    int N, win, hop, F, K, n_lo;
    int ftiles, ktiles, ttiles;               // frame tiles; groups of 64 of the N/2 bin columns; groups of 64 window taps
    int tile0, stile0;                        // this resolution's first tile in the analysis / synthesis grid of a row
    int ntiles;                               // its tiles in the analysis grid, ftiles ktiles: one slab each
    long long plane0, frame0;                 // offsets (doubles) of its four planes / its frames inside a row's share
};

struct SlPlan {
    int R, B, T;
    int tiles, stiles;                        // tiles of one row: analysis, synthesis
    long long planes_row, frames_row;         // doubles per row
    SlRes res[SL_MAX_R];
};

// workspace, in doubles:  slabs [B][tiles][3] | terms [B][R][2] (SC, LM) | coef [B][R][2] | rows [B][3] | planes [B][planes_row] |
//                         frames [B][frames_row]
struct SlWs {
    double *slabs, *terms, *coef, *rows, *planes, *frames;
};

__global__ __launch_bounds__(SL_T) void sl_analysis_kernel(const float* __restrict__ wav_pred, const float* __restrict__ wav_true, SlPlan p,
                                                           double delta, int backward, SlWs ws) {
    __shared__ double tw_c[SL_MAX_NFFT], tw_s[SL_MAX_NFFT], wtab[SL_MAX_NFFT], xp[SL_TM * SL_LD], xt[SL_TM * SL_LD];
    __shared__ double red[3][SL_T / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / p.tiles, tile = blockIdx.x % p.tiles;
    int local;
    const SlRes g = p.res[sl_find(p, &SlRes::tile0, tile, local)];
    const int f0 = (local / g.ktiles) * SL_TM, k0 = (local % g.ktiles) * SL_TN + wave * 16;
    const int k = k0 + row;                                          // this lane's column: a bin below N/2 (may be past them: not counted)
    const int T = p.T, N = g.N, half = N / 2, n_hi = g.n_lo + g.win;
    const float* __restrict__ yp = wav_pred + (size_t)b * T;
    const float* __restrict__ yt = wav_true + (size_t)b * T;
    double* __restrict__ slab = ws.slabs + ((size_t)b * p.tiles + tile) * 3;

    stft_tables(tw_c, tw_s, wtab, N, g.win, SL_T);
    // E0 and sum w^2: a thread's groups of four samples (taps: the ones it has just written) in index order, then the fixed pairing -
    // the same bits in every workgroup of the row, whatever the row's alignment (zeros past its end add exact zeros)
    double e0 = 0.0, w2 = 0.0, none = 0.0;
    const bool vec = (T % 4 == 0) && aligned16(yt);
    for (int t = 4 * tid; t < T; t += 4 * SL_T) {
        const float4 v = ld_group(yt, t, T, vec);
        e0 += (double)v.x * (double)v.x; e0 += (double)v.y * (double)v.y; e0 += (double)v.z * (double)v.z; e0 += (double)v.w * (double)v.w;
    }
    for (int n = tid; n < N; n += SL_T) w2 += wtab[n] * wtab[n];
    sl_block_sum3(red, e0, w2, none);                                // its barriers also stand behind the tables
    if (e0 == 0.0) {                                                 // a silent target: uniform over the workgroup
        if (tid == 0) { slab[0] = 0.0; slab[1] = 0.0; slab[2] = 0.0; }
        return;
    }
    const double dp0 = delta * (w2 * e0 / (double)T);

    // Bins 0 and N/2 are real: column 0 carries bin N/2 in its "imaginary" accumulators (twiddle (-1)^n, exact in the table, where
    // bin 0's own -sin is an exact zero), so the tiles cover N/2 columns, a multiple of 64 for every N >= 128.
    const bool live = k0 < half;                                     // wave-uniform: a wave past the last column computes nothing
    sl_d4 pr = {0.0, 0.0, 0.0, 0.0}, pi = pr, tr = pr, ti = pr;
    for (int tc = 0; tc < g.win; tc += SL_KC) {
        __syncthreads();                                             // the previous chunk is no longer read
        for (int el = tid; el < SL_TM * SL_KC; el += SL_T) {
            const int r = el / SL_KC, j = el % SL_KC, n = g.n_lo + tc + j, f = f0 + r;
            double vp = 0.0, vt = 0.0;
            if (n < n_hi && f < g.F) {
                int i = g.hop * f + n - half;                        // in [-N/2, T + N/2): one reflection reaches [0, T) as T > N/2
                if (i < 0) i = -i;
                if (i >= T) i = 2 * (T - 1) - i;
                const double w = wtab[n];
                vp = w * (double)yp[i]; vt = w * (double)yt[i];
            }
            xp[r * SL_LD + j] = vp; xt[r * SL_LD + j] = vt;
        }
        __syncthreads();
        if (live) {
            const int valid = g.win - tc < SL_KC ? g.win - tc : SL_KC;
            const int steps = (valid + 3) >> 2;
            int idx = (int)(((long long)k * (g.n_lo + tc + kq)) % N);
            const int inc = (4 * k) % N;
            const double nyq = ((g.n_lo + tc + kq) & 1) ? tw_c[half] : tw_c[0];      // (-1)^n: n = n_lo + tc + 4 s + kq keeps its parity
            for (int s = 0; s < steps; ++s) {
                const int j = 4 * s + kq;                            // taps past n_hi were staged as zeros
                const double a = xp[row * SL_LD + j], c = xt[row * SL_LD + j];
                const double cs = tw_c[idx], ms = k == 0 ? nyq : -tw_s[idx];
                pr = __builtin_amdgcn_mfma_f64_16x16x4f64(a, cs, pr, 0, 0, 0);
                pi = __builtin_amdgcn_mfma_f64_16x16x4f64(a, ms, pi, 0, 0, 0);
                tr = __builtin_amdgcn_mfma_f64_16x16x4f64(c, cs, tr, 0, 0, 0);
                ti = __builtin_amdgcn_mfma_f64_16x16x4f64(c, ms, ti, 0, 0, 0);
                idx += inc;
                if (idx >= N) idx -= N;
            }
        }
    }
    double s_d = 0.0, s_y = 0.0, s_l = 0.0;
    if (k < half) {
        const double inv_fk = 1.0 / ((double)g.F * (double)g.K);
        double* __restrict__ pl = ws.planes + (size_t)b * p.planes_row + g.plane0;
        const size_t P = (size_t)g.F * g.K;
        // one bin (f, kb) with the spectra (re_p, im_p) of y^ and (re_t, im_t) of y
        auto bin = [&](int f, int kb, double re_p, double im_p, double re_t, double im_t) {
            const double mp = sqrt(re_p * re_p + im_p * im_p + dp0), my = sqrt(re_t * re_t + im_t * im_t + dp0);
            const double d = mp - my, l = log(mp) - log(my);
            s_d += d * d; s_y += my * my; s_l += l * l;
            if (backward) {
                const size_t at = (size_t)f * g.K + kb;
                pl[at] = re_p; pl[P + at] = im_p;
                pl[2 * P + at] = 2.0 * d / mp;
                pl[3 * P + at] = 2.0 * l * inv_fk / (mp * mp);
            }
        };
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 r
            const int f = f0 + kq + 4 * r;
            if (f < g.F) {
                if (k == 0) {
                    bin(f, 0, pr[r], 0.0, tr[r], 0.0);
                    bin(f, half, pi[r], 0.0, ti[r], 0.0);
                } else {
                    bin(f, k, pr[r], pi[r], tr[r], ti[r]);
                }
            }
        }
    }
    sl_block_sum3(red, s_d, s_y, s_l);
    if (tid == 0) { slab[0] = s_d; slab[1] = s_y; slab[2] = s_l; }
}

// frames[b][f][n - n_lo] = w[n] sum_k (dRe[f,k] cos(2 pi k n / N) - dIm[f,k] sin(2 pi k n / N)) for the non-zero taps.  A = dRe, dIm
// (16 frames x a chunk of bins), B = the twiddles; wave w owns taps n_lo + 16 (4 tap group + w) ... + 15.
__global__ __launch_bounds__(SL_T) void sl_synth_kernel(SlPlan p, SlWs ws) {
    __shared__ double tw_c[SL_MAX_NFFT], tw_s[SL_MAX_NFFT], xr[SL_TM * SL_LD], xi[SL_TM * SL_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / p.stiles, tile = blockIdx.x % p.stiles;
    if (ws.rows[3 * (size_t)b + 2] == 0.0) return;                   // a row that is not counted: the fold writes its zeros
    int local;
    const int r_of = sl_find(p, &SlRes::stile0, tile, local);
    const SlRes g = p.res[r_of];
    const int f0 = (local / g.ttiles) * SL_TM, m0 = (local % g.ttiles) * SL_TN + wave * 16;
    const int N = g.N, n_hi = g.n_lo + g.win;
    const int n = g.n_lo + m0 + row;                                 // this lane's column: a window tap (may be >= n_hi: not stored)
    const double ca = ws.coef[2 * ((size_t)b * p.R + r_of)], cb = ws.coef[2 * ((size_t)b * p.R + r_of) + 1];
    const double* __restrict__ pl = ws.planes + (size_t)b * p.planes_row + g.plane0;
    const size_t P = (size_t)g.F * g.K;
    stft_tables(tw_c, tw_s, nullptr, N, g.win, SL_T);
    const bool live = g.n_lo + m0 < n_hi;
    sl_d4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < g.K; kc += SL_KC) {
        __syncthreads();                                             // the previous chunk is no longer read (first pass: tables)
        for (int el = tid; el < SL_TM * SL_KC; el += SL_T) {
            const int r = el / SL_KC, kk = el % SL_KC, k = kc + kk, f = f0 + r;
            double vr = 0.0, vi = 0.0;
            if (k < g.K && f < g.F) {
                const size_t at = (size_t)f * g.K + k;
                const double gg = ca * pl[2 * P + at] + cb * pl[3 * P + at];
                vr = gg * pl[at]; vi = gg * pl[P + at];
            }
            xr[r * SL_LD + kk] = vr; xi[r * SL_LD + kk] = vi;
        }
        __syncthreads();
        if (live) {
            const int valid = g.K - kc < SL_KC ? g.K - kc : SL_KC;
            const int steps = (valid + 3) >> 2;
            int idx = (int)(((long long)(kc + kq) * n) % N);
            const int inc = (4 * n) % N;
            for (int s = 0; s < steps; ++s) {
                const int kk = 4 * s + kq;                           // bins past K were staged as zeros
                const double ar = xr[row * SL_LD + kk], ai = xi[row * SL_LD + kk];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ar, tw_c[idx], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ai, -tw_s[idx], acc, 0, 0, 0);
                idx += inc;
                if (idx >= N) idx -= N;
            }
        }
    }
    if (n < n_hi) {
        const double w = stft_hann<double>(n, N, g.win);
        double* __restrict__ fr = ws.frames + (size_t)b * p.frames_row + g.frame0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                // f64 C/D layout: column = lane & 15, row = (lane >> 4) + 4 r
            const int f = f0 + kq + 4 * r;
            if (f < g.F) fr[(size_t)f * g.win + (n - g.n_lo)] = w * acc[r];
        }
    }
}

bool sl_supported(int T, int N, int win, int hop) {
    return N >= SL_MIN_NFFT && N <= SL_MAX_NFFT && N % 2 == 0 && win >= 2 && win <= N && hop >= 1 && T >= N / 2 + 1 && T <= SL_MAX_T;
}

// the plan of a call and its workspace in doubles (0: not supported)
size_t sl_plan(int B, int T, int R, const int* res, SlPlan* out) {
    if (B <= 0 || R < 1 || R > SL_MAX_R || !res) return 0;
    SlPlan p = {};
    p.R = R; p.B = B; p.T = T;
    long long at = 0, st = 0, planes = 0, frames = 0;
    for (int r = 0; r < R; ++r) {
        const int N = res[3 * r], win = res[3 * r + 1], hop = res[3 * r + 2];
        if (!sl_supported(T, N, win, hop)) return 0;
        SlRes& g = p.res[r];
        sl_res_fill(g, T, N, win, hop, frames);
        g.ftiles = (g.F + SL_TM - 1) / SL_TM; g.ktiles = (N / 2 + SL_TN - 1) / SL_TN; g.ttiles = (win + SL_TN - 1) / SL_TN;
        g.tile0 = (int)at; g.stile0 = (int)st; g.ntiles = g.ftiles * g.ktiles; g.plane0 = planes;
        at += (long long)g.ftiles * g.ktiles; st += (long long)g.ftiles * g.ttiles;
        planes += 4LL * g.F * g.K;
    }
    if (at * B > 0x7fffffffLL || st * B > 0x7fffffffLL || sl_fold_blocks(B, T) > 0x7fffffffLL) return 0;      // the grids are one-dimensional
    p.tiles = (int)at; p.stiles = (int)st; p.planes_row = planes; p.frames_row = frames;
    if (out) *out = p;
    return sl_head_doubles(B, at, R) + (size_t)B * ((size_t)planes + (size_t)frames);
}

}  // namespace

extern "C" {

int unetrir_spectral_loss_supported(int T, int n_fft, int win_length, int hop_length) {
    return sl_supported(T, n_fft, win_length, hop_length) ? 1 : 0;
}

size_t unetrir_spectral_loss_ws_bytes(int B, int T, int R, const int* res) { return sl_plan(B, T, R, res, nullptr) * sizeof(double); }

int unetrir_spectral_loss_f32(const float* wav_pred, const float* wav_true, int B, int T, int R, const int* res, double floor_db,
                              double sc_weight, double log_weight, double weight, double inv_global_batch, int accumulate, float* dwav,
                              double* spectral_out, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!sl_args_ok(wav_pred, wav_true, B, R, res, floor_db, sc_weight, log_weight, weight, inv_global_batch, accumulate, dwav,
                    spectral_out, ws))
        return UNETRIR_EINVAL;
    SlPlan p;
    const size_t need = sl_plan(B, T, R, res, &p) * sizeof(double);
    if (need == 0 || ws_bytes < need) return UNETRIR_EINVAL;
    SlWs w;
    w.planes = sl_head_carve(w, ws, B, p.tiles, R);
    w.frames = w.planes + (size_t)B * p.planes_row;
    const double delta = pow(10.0, -floor_db / 10.0), scale = weight * inv_global_batch;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sl_analysis_kernel, dim3((unsigned)(B * p.tiles)), dim3(SL_T), 0, s, wav_pred, wav_true, p, delta, (int)(dwav != nullptr),
                       w);
    hipLaunchKernelGGL(sl_finalize_kernel, dim3(1), dim3(SL_T), 0, s, p, sc_weight, log_weight, scale, w, spectral_out, loss_out);
    if (dwav) {
        hipLaunchKernelGGL(sl_synth_kernel, dim3((unsigned)(B * p.stiles)), dim3(SL_T), 0, s, p, w);
        hipLaunchKernelGGL(sl_fold_kernel, dim3((unsigned)sl_fold_blocks(B, T)), dim3(SL_T), 0, s, p, w, accumulate, dwav);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
