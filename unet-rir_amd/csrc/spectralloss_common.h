// spectralloss_common.h - the tail the two forms of the multi-resolution STFT loss (spectralloss.hip, fp64 DFTs; spectralloss_fft.hip, fp32
// FFTs in LDS) share.  They are one definition with two transforms: once a workgroup has its three partial sums, everything up to the
// loss is fp64 arithmetic on slabs and the same for both, and so is the way back from windowed frames to dwav.  Here are the limits, the
// argument checks of the entry points, the part of a resolution's plan that does not depend on the tiling, the fp64 head of the
// workspace, the fixed-order sum of a workgroup, the tile lookup, the finalize kernel and the overlap-add / fold kernel.  What differs
// stays in the two files: the transforms, the tiling of a row's grid (and the DFT form's planes), and the _supported predicates.
//
// The kernels are templates on the form's plan and workspace.  A plan has  R, B, T, tiles (workgroups of one row's analysis grid),
// frames_row  and  res[R]  with  N, win, hop, F, K, n_lo, tile0 (first workgroup), ntiles (their count: one slab each), frame0;  a
// workspace has  slabs, terms, coef, rows  (fp64) and  frames  (fp64 or fp32, [f][tap - n_lo] per resolution).
//
// Nothing here carries `#pragma clang fp contract(off)`: none of the bodies it replaces did.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "stft_common.h"

constexpr int SL_MAX_NFFT = 1024;
constexpr int SL_MAX_T = 16384;
constexpr int SL_MAX_R = 8;
constexpr int SL_T = 256;                     // threads of every kernel of both forms: 4 waves

// the checks of the two entry points that do not need the plan
inline bool sl_args_ok(const float* wav_pred, const float* wav_true, int B, int R, const int* res, double floor_db, double sc_weight,
                       double log_weight, double weight, double inv_global_batch, int accumulate, const float* dwav,
                       const double* spectral_out, const void* ws) {
    if (!wav_pred || !wav_true || !spectral_out || !ws || ((uintptr_t)ws & 7) || !res || B <= 0 || R < 1 || R > SL_MAX_R) return false;
    return isfinite(floor_db) && floor_db > 0.0 && floor_db <= 200.0 && sc_weight >= 0.0 && isfinite(sc_weight) && log_weight >= 0.0 &&
           isfinite(log_weight) && weight >= 0.0 && isfinite(weight) && inv_global_batch > 0.0 && isfinite(inv_global_batch) &&
           !(accumulate && !dwav);
}

// the geometry of one resolution and its frames' place in a row's share; `frames` moves past them
template <class Res>
inline void sl_res_fill(Res& g, int T, int N, int win, int hop, long long& frames) {
    g.N = N; g.win = win; g.hop = hop; g.F = 1 + T / hop; g.K = N / 2 + 1; g.n_lo = (N - win) / 2;
    g.frame0 = frames;
    frames += (long long)g.F * win;
}

// the fp64 head of the workspace:  slabs [B][tiles][3] | terms [B][R][2] (SC, LM) | coef [B][R][2] | rows [B][3]
inline size_t sl_head_doubles(int B, long long tiles, int R) { return (size_t)B * ((size_t)tiles * 3 + (size_t)R * 4 + 3); }

template <class Ws>
inline double* sl_head_carve(Ws& w, void* ws, int B, int tiles, int R) {                  // returns what follows the head
    w.slabs = (double*)ws;
    w.terms = w.slabs + (size_t)B * tiles * 3;
    w.coef = w.terms + (size_t)B * R * 2;
    w.rows = w.coef + (size_t)B * R * 2;
    return w.rows + (size_t)B * 3;
}

// workgroups of the fold kernel: its grid is one-dimensional, so a plan holds this below 2^31
inline long long sl_fold_blocks(int B, int T) { return (long long)B * ((T + SL_T - 1) / SL_T); }

// three sums over the workgroup at once, every thread gets them: the lanes of a wave by a shuffle tree (a fixed pairing), the four
// waves in index order
__device__ __forceinline__ void sl_block_sum3(double (*red)[SL_T / 64], double& a, double& b, double& c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); c += __shfl_down(c, off, 64);
    }
    __syncthreads();                                                 // red is no longer read
    if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    c = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
}

// the resolution a tile of a row's grid belongs to, and the tile's index inside it; `first` names the grid: the field that holds a
// resolution's first tile in it
template <class Plan, class Res>
__device__ __forceinline__ int sl_find(const Plan& p, int Res::*first, int tile, int& local) {
    int r = 0;
    for (int i = 1; i < p.R; ++i)
        if (tile >= p.res[i].*first) r = i;
    local = tile - p.res[r].*first;
    return r;
}

// One workgroup: the slabs of each (b, r) in index order -> SC, LM and the two scalars that scale the gradient (c sc_weight / sum M_y^2,
// c log_weight; zeros for a row that is not counted); Q_b over r in index order; spectral_out = (sum_b mean_r SC, sum_b mean_r LM, rows
// counted); loss_out[0] += (float) L.
template <class Plan, class Ws>
__global__ __launch_bounds__(SL_T) void sl_finalize_kernel(Plan p, double sc_weight, double log_weight, double scale, Ws ws,
                                                           double* __restrict__ spectral_out, float* __restrict__ loss_out) {
    __shared__ double red[3][SL_T / 64];
    const int tid = threadIdx.x;
    const double c = scale / (double)p.R;
    for (long long pair = tid; pair < (long long)p.B * p.R; pair += SL_T) {
        const int b = (int)(pair / p.R), r = (int)(pair % p.R);
        const auto& g = p.res[r];
        const double* s = ws.slabs + ((size_t)b * p.tiles + g.tile0) * 3;
        double d = 0.0, y = 0.0, l = 0.0;
        for (int i = 0; i < g.ntiles; ++i) { d += s[3 * i]; y += s[3 * i + 1]; l += s[3 * i + 2]; }
        const bool counted = y > 0.0;                                // M_y >= sqrt(delta P0) > 0 in a counted row
        ws.terms[2 * pair] = counted ? d / y : 0.0;
        ws.terms[2 * pair + 1] = counted ? l / ((double)g.F * (double)g.K) : 0.0;
        ws.coef[2 * pair] = counted ? c * sc_weight / y : 0.0;
        ws.coef[2 * pair + 1] = counted ? c * log_weight : 0.0;
        if (r == 0) ws.rows[3 * (size_t)b + 2] = counted ? 1.0 : 0.0;
    }
    __syncthreads();
    double q_sc = 0.0, q_lm = 0.0, q_n = 0.0;
    for (int b = tid; b < p.B; b += SL_T) {
        double sc = 0.0, lm = 0.0;
        for (int r = 0; r < p.R; ++r) { sc += ws.terms[2 * ((size_t)b * p.R + r)]; lm += ws.terms[2 * ((size_t)b * p.R + r) + 1]; }
        sc /= (double)p.R; lm /= (double)p.R;
        ws.rows[3 * (size_t)b] = sc; ws.rows[3 * (size_t)b + 1] = lm;
        q_sc += sc; q_lm += lm; q_n += ws.rows[3 * (size_t)b + 2];
    }
    sl_block_sum3(red, q_sc, q_lm, q_n);
    if (tid == 0) {
        spectral_out[0] = q_sc; spectral_out[1] = q_lm; spectral_out[2] = q_n;
        if (loss_out) loss_out[0] += (float)(scale * (sc_weight * q_sc + log_weight * q_lm));
    }
}

// p[j]: the frames whose non-zero taps reach the padded position j, in ascending frame order, summed in fp64
template <class Res, class E>
__device__ __forceinline__ double sl_ola(const E* __restrict__ fr, const Res& g, int j) {
    int f_lo, f_hi;
    stft_frame_range(j, g.n_lo, g.win, g.hop, g.F, f_lo, f_hi);
    double acc = 0.0;
    for (int f = f_lo; f <= f_hi; ++f) acc += (double)fr[(size_t)f * g.win + (j - g.hop * f - g.n_lo)];
    return acc;
}

// Gather: one thread owns one output sample; per resolution in index order the frames that reach t + N/2 and the reflected positions
// j = N/2 - t and j = 2 (T - 1) - t + N/2, each in ascending frame order; one rounding to fp32 (or (float)((double) dwav + g)).  A row
// that is not counted gets zeros.  Grid: sl_fold_blocks.
template <class Plan, class Ws>
__global__ __launch_bounds__(SL_T) void sl_fold_kernel(Plan p, Ws ws, int accumulate, float* __restrict__ dwav) {
    const int chunks = (p.T + SL_T - 1) / SL_T;
    const int b = blockIdx.x / chunks, t = (blockIdx.x % chunks) * SL_T + threadIdx.x;
    if (t >= p.T) return;
    const size_t o = (size_t)b * p.T + t;
    double total = 0.0;
    if (ws.rows[3 * (size_t)b + 2] != 0.0) {
        for (int r = 0; r < p.R; ++r) {
            const auto& g = p.res[r];
            const auto* __restrict__ fr = ws.frames + (size_t)b * p.frames_row + g.frame0;
            const int half = g.N / 2;
            double acc = sl_ola(fr, g, t + half);
            if (t >= 1 && t <= half) acc += sl_ola(fr, g, half - t);
            if (t <= p.T - 2 && t >= p.T - 1 - half) acc += sl_ola(fr, g, 2 * (p.T - 1) - t + half);
            total += acc;
        }
    }
    dwav[o] = accumulate ? (float)((double)dwav[o] + total) : (float)total;
}
