// griffinlim_fft.hip - the FFT form of the Griffin-Lim reconstruction: the definition of griffinlim.hip's header (same un-pad and
// denormalisation, S not clamped, the phase plane ignored, angles0 = exp(2 pi i u), the same loop, the same centred periodic Hann pair,
// `wss > tiny32` envelope rule, trimming, both pad modes, gl_decimal for the momentum) with fp32 state and fp32 transforms held in LDS
// (fft_lds.h) in place of fp64 state and fp64 DFTs on the matrix cores (gfx950).  librosa holds its angles in complex64; this is that
// precision.  The iteration amplifies rounding, so no bound per element is derived: the DFT form is the one to hold a result to a bound,
// this one is for evaluation runs, which pay the loop on every batch (include/unetrir.h; tests/griffinlim_fft_ref.py for what it is held to).
//
// State, all fp32, [b][f][k] with the bin fastest: S = the value gl_init_kernel forms in fp64, rounded once; three complex planes that take
// turns as rebuilt, tprev and the plane being written; angles0 = the fp32 rounding of sincospi taken in fp64, in the first plane.
// `spec = S angles` is not stored: the loader of every synthesis forms it from the stored planes,
//     launch 0:  S angles0          launch 1:  S n(rebuilt)          launch j >= 2:  S n(rebuilt - alpha tprev),    n(a) = a / (hypotf(a) + 1e-16f)
// (rebuilt is 0 before the first iteration, so launch 1 subtracts nothing, as the DFT form's `first` does).  A workgroup reads the frames
// of its halo, which another workgroup owns: with spec stored in place the owner's epilogue would overwrite what the neighbour's loader is
// still reading, and a second copy of spec costs more memory than S n(.) costs arithmetic.  Two workgroups form a halo frame's spec from
// the same stored values by the same expression, so the bits do not depend on the tiling.
//
// A real transform of N = n_fft points is a complex FFT of M = N / 2 points worked by M / 8 threads plus fl_split_fwd / fl_split_inv;
// 2048 / M images ride side by side in the 16 KB of one 256-thread workgroup, all groups in lockstep (spectralloss_fft.hip).  Bins 0 and N / 2
// share slot 0 as two reals: their imaginary parts are ignored, as numpy.fft.irfft ignores them.
//
//   gf_init      S and angles0                                                                              (one launch)
//   gf_iterate   one launch per iteration.  A workgroup owns `own` consecutive frames of one row.  It finds the run of samples its
//                analysis windows reach - its frames' taps and, at the two ends of a row, the samples the reflection maps them to:
//                one contiguous run [s_lo, s_hi) - inverse-transforms every frame whose window reaches that run (its own, the halo
//                of ceil(win / hop) - 1 either side, the frames under the reflected samples), 2048 / M at a time, and overlap-adds
//                them into the run in LDS: the intermediate waveform never leaves the CU.  It then builds the windowed frames of its
//                own frames from the run, transforms them forward and stores rebuilt.
//   gf_final     the same synthesis over a run of output samples, stored as fp32                             (one launch)
//
// n_iter + 2 launches whatever B is.  Orders of summation: a sample of the run is (((0 + w[m_a] x_a[m_a]) + w[m_a+1] x_a+1[...]) + ...)
// over the frames a < a + 1 < ... that reach it in ascending order, one fp32 product and one fp32 addition each, whichever batch of
// images a frame arrives in; its envelope sum w^2 likewise in fp32; then times the exact 1 / N and divided by the envelope where that
// exceeds tiny32.  Complex products go through fl_mul (contraction off), everything else here is compiled with contraction off too.  No
// atomics: two runs give the same bits, and a row's bits depend neither on B nor on its place.  Nothing is allocated, cleared or waited
// for, so the call can be captured in a HIP graph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "kernels.h"
#include "griffinlim_common.h"
#include "stft_common.h"
#include "fft_lds.h"

namespace {

using namespace fftlds;

constexpr int GF_MAX_NFFT = 1024;
constexpr int GF_MIN_NFFT = 128;
constexpr int GF_T = 256;                     // 4 waves
constexpr int GF_IMG = 2048;                  // complex points of the workgroup's images: 16 KB
constexpr int GF_SEG = 4096;                  // samples of the workgroup's run of the waveform: 16 KB
constexpr float GF_TINY32 = (float)GL_TINY32;

struct GfGeom {
    int B, H, W, n_bins, n_frames, n_fft, win, hop, T_out;
    int n_lo;                                 // first non-zero tap of the padded window
    int pad_mode;
    int own, tiles;                           // frames a workgroup of gf_iterate owns; workgroups per row
    int chunk, chunks;                        // samples a workgroup of gf_final owns; workgroups per row
};

// workspace: three complex planes, then S
struct GfWs {
    cf* plane[3];
    float* S;
};

__global__ __launch_bounds__(256) void gf_init_kernel(const float* __restrict__ feat, GfGeom g, int denormalize,
                                                      const float* __restrict__ init_phase, unsigned long long seed, unsigned long long draw,
                                                      float* __restrict__ S, cf* __restrict__ angles) {
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
        S[e] = (float)amp;
        angles[e] = {(float)cs, (float)sn};
    }
}

// S angles of one bin from the stored planes (mode: the launch number capped at 2, see the header)
__device__ __forceinline__ cf gf_spec(const float* __restrict__ S, const cf* __restrict__ cur, const cf* __restrict__ prev, size_t e, int mode,
                                      float alpha) {
#pragma clang fp contract(off)
    cf a = cur[e];
    if (mode != 0) {
        if (mode == 2) {
            const cf p = prev[e];
            a.x -= alpha * p.x;
            a.y -= alpha * p.y;
        }
        const float d = hypotf(a.x, a.y) + 1e-16f;
        a.x /= d;
        a.y /= d;
    }
    const float s = S[e];
    return {s * a.x, s * a.y};
}

// seg[s - s_lo] = librosa.istft's sample s (trimmed coordinates) of row b for s_lo <= s < s_hi, 0 < s_hi - s_lo <= GF_SEG.  Returns with
// the run complete (a barrier is the last thing it does); img is free again.
template <int M>
__device__ __forceinline__ void gf_segment(cf* img, float* seg, const float* wtab, const GfGeom& g, int b, int s_lo, int s_hi,
                                           const float* __restrict__ S, const cf* __restrict__ cur, const cf* __restrict__ prev, int mode,
                                           float alpha) {
#pragma clang fp contract(off)
    constexpr int TG = M / 8, IMG = GF_IMG / M;
    const int tid = threadIdx.x, grp = tid / TG, t = tid % TG;
    const int hop = g.hop;
    // the frames whose non-zero taps reach the padded positions [s_lo + M, s_hi + M): from the first of its first to the last of its last
    int g_lo, g_hi, other;
    stft_frame_range<false>(s_lo + M, g.n_lo, g.win, hop, g.n_frames, g_lo, other);
    stft_frame_range<false>(s_hi - 1 + M, g.n_lo, g.win, hop, g.n_frames, other, g_hi);
    for (int s = s_lo + tid; s < s_hi; s += GF_T) seg[s - s_lo] = 0.f;
    cf* buf = img + grp * M;
    for (int p0 = g_lo; p0 <= g_hi; p0 += IMG) {
        __syncthreads();                                             // img is no longer read; first pass: the zeros of seg, wtab
        const int f = p0 + grp;
        const size_t row = ((size_t)b * g.n_frames + (f <= g_hi ? f : g_hi)) * (M + 1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = t + TG * e;
            cf v = {0.f, 0.f};
            if (f <= g_hi) {
                if (i == 0) v = {gf_spec(S, cur, prev, row, mode, alpha).x, gf_spec(S, cur, prev, row + M, mode, alpha).x};
                else v = gf_spec(S, cur, prev, row + i, mode, alpha);
            }
            buf[fl_swz(i)] = v;
        }
        __syncthreads();
        fl_split_inv<M>(buf, t, TG);
        __syncthreads();
        fl_fft<M, 1>(buf, t);
        const int p1 = p0 + IMG - 1 < g_hi ? p0 + IMG - 1 : g_hi;
        for (int s = s_lo + tid; s < s_hi; s += GF_T) {
            const int q = s + M;
            int a, z;
            stft_frame_range<false>(q, g.n_lo, g.win, hop, g.n_frames, a, z);
            if (a < p0) a = p0;
            if (z > p1) z = p1;
            float acc = seg[s - s_lo];
            for (int gi = a; gi <= z; ++gi) {
                const int m = q - hop * gi;                          // tap of frame gi, in [n_lo, n_hi)
                const cf c = img[(gi - p0) * M + fl_swz(m >> 1)];
                acc += wtab[m] * ((m & 1) ? c.y : c.x);
            }
            seg[s - s_lo] = acc;
        }
    }
    // a thread finishes the samples it has summed itself
    const float inv_n = 1.f / (float)(2 * M);
    for (int s = s_lo + tid; s < s_hi; s += GF_T) {
        const int q = s + M;
        int a, z;
        stft_frame_range<false>(q, g.n_lo, g.win, hop, g.n_frames, a, z);
        float wss = 0.f;
        for (int gi = a; gi <= z; ++gi) {
            const float w = wtab[q - hop * gi];
            wss += w * w;
        }
        const float y = seg[s - s_lo] * inv_n;
        seg[s - s_lo] = wss > GF_TINY32 ? y / wss : y;
    }
    __syncthreads();
}

template <int M>
__device__ __forceinline__ void gf_iterate(cf* img, float* seg, float* wtab, const GfGeom& g, int b, int tile, const float* __restrict__ S,
                                           const cf* __restrict__ cur, const cf* __restrict__ prev, int mode, float alpha,
                                           cf* __restrict__ out) {
#pragma clang fp contract(off)
    constexpr int TG = M / 8;
    const int tid = threadIdx.x, grp = tid / TG, t = tid % TG;
    const int n_hi = g.n_lo + g.win, T = g.T_out;
    const int f0 = tile * g.own;
    const int nown = g.n_frames - f0 < g.own ? g.n_frames - f0 : g.own;
    for (int n = tid; n < 2 * M; n += GF_T) wtab[n] = stft_hann<float>(n, 2 * M, g.win);
    // the samples the taps of frames f0 ... f0 + nown - 1 reach: lo <= s < hi before the padding, then what the reflection maps to
    const int lo = g.hop * f0 + g.n_lo - M, hi = g.hop * (f0 + nown - 1) + n_hi - M;
    int s_lo = lo < 0 ? 0 : lo, s_hi = hi > T ? T : hi;
    if (g.pad_mode == 0) {
        if (lo < 0 && 1 - lo > s_hi) s_hi = 1 - lo;                  // s < 0 reads -s: samples 1 ... -lo
        const long long back = 2LL * (T - 1) - (hi - 1);             // s >= T reads 2 (T - 1) - s (T may be close to 2^31)
        if (hi > T && back < s_lo) s_lo = (int)back;
    }
    if (s_lo < 0 || s_hi > T || s_hi - s_lo > GF_SEG || s_hi <= s_lo) return;            // not reached: the host chose `own` for it
    gf_segment<M>(img, seg, wtab, g, b, s_lo, s_hi, S, cur, prev, mode, alpha);
    const int f = f0 + grp;
    cf* buf = img + grp * M;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int i = t + TG * e;
        float v[2] = {0.f, 0.f};
        if (grp < nown) {
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int n = 2 * i + s;
                if (n >= g.n_lo && n < n_hi) {
                    int j = g.hop * f + n - M;                       // in [-N/2, T + N/2): one reflection reaches [0, T) as T > N/2
                    bool inside = j >= 0 && j < T;
                    if (!inside && g.pad_mode == 0) {
                        j = j < 0 ? -j : (int)(2LL * (T - 1) - j);
                        inside = true;
                    }
                    if (inside) v[s] = wtab[n] * seg[j - s_lo];
                }
            }
        }
        buf[fl_swz(i)] = {v[0], v[1]};
    }
    __syncthreads();
    fl_fft<M, -1>(buf, t);
    fl_split_fwd<M>(buf, t, TG);
    __syncthreads();
    for (int q = tid; q < nown * M; q += GF_T) {
        const int lf = q / M, i = q % M;
        const cf c = img[lf * M + fl_swz(i)];
        const size_t row = ((size_t)b * g.n_frames + f0 + lf) * (M + 1);
        if (i == 0) {
            out[row] = {c.x, 0.f};
            out[row + M] = {c.y, 0.f};
        } else {
            out[row + i] = c;
        }
    }
}

__global__ __launch_bounds__(GF_T) void gf_iterate_kernel(GfGeom g, const float* __restrict__ S, const cf* __restrict__ cur,
                                                          const cf* __restrict__ prev, int mode, float alpha, cf* __restrict__ out) {
    __shared__ cf img[GF_IMG];
    __shared__ float seg[GF_SEG];
    __shared__ float wtab[GF_MAX_NFFT];
    const int b = blockIdx.y, tile = blockIdx.x;
    switch (g.n_fft) {
        case 128: gf_iterate<64>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, out); break;
        case 256: gf_iterate<128>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, out); break;
        case 512: gf_iterate<256>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, out); break;
        default: gf_iterate<512>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, out); break;
    }
}

template <int M>
__device__ __forceinline__ void gf_final(cf* img, float* seg, float* wtab, const GfGeom& g, int b, int tile, const float* __restrict__ S,
                                         const cf* __restrict__ cur, const cf* __restrict__ prev, int mode, float alpha,
                                         float* __restrict__ wav) {
    const int tid = threadIdx.x;
    for (int n = tid; n < 2 * M; n += GF_T) wtab[n] = stft_hann<float>(n, 2 * M, g.win);
    const long long lo = (long long)tile * g.chunk;
    const int s_lo = (int)lo, s_hi = lo + g.chunk > g.T_out ? g.T_out : s_lo + g.chunk;
    if (s_hi - s_lo > GF_SEG || s_hi <= s_lo) return;                // not reached
    gf_segment<M>(img, seg, wtab, g, b, s_lo, s_hi, S, cur, prev, mode, alpha);
    for (int s = s_lo + tid; s < s_hi; s += GF_T) wav[(size_t)b * g.T_out + s] = seg[s - s_lo];
}

__global__ __launch_bounds__(GF_T) void gf_final_kernel(GfGeom g, const float* __restrict__ S, const cf* __restrict__ cur,
                                                        const cf* __restrict__ prev, int mode, float alpha, float* __restrict__ wav) {
    __shared__ cf img[GF_IMG];
    __shared__ float seg[GF_SEG];
    __shared__ float wtab[GF_MAX_NFFT];
    const int b = blockIdx.y, tile = blockIdx.x;
    switch (g.n_fft) {
        case 128: gf_final<64>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, wav); break;
        case 256: gf_final<128>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, wav); break;
        case 512: gf_final<256>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, wav); break;
        default: gf_final<512>(img, seg, wtab, g, b, tile, S, cur, prev, mode, alpha, wav); break;
    }
}

// The rule of include/unetrir.h.  4 hop >= win bounds the frames that reach one sample (at most 4); the length rule is what a single
// reflection needs and is asked of both pad modes, so that one rule answers for a geometry.
bool gf_supported(int n_bins, int n_frames, int n_fft, int win, int hop) {
    if (n_fft != 128 && n_fft != 256 && n_fft != 512 && n_fft != 1024) return false;
    if (n_bins != n_fft / 2 + 1 || n_frames < 2 || win < 2 || win > n_fft || hop < 1 || 4LL * hop < win) return false;
    if ((long long)hop * n_frames + n_fft > 0x7fffffffLL) return false;
    return (long long)hop * (n_frames - 1) > n_fft / 2;
}

// frames per workgroup: what leaves room for the halo in one batch of 4096 / n_fft images if that is at least half of them, else
// all of them (the synthesis then takes more batches); fewer where a long hop would outgrow the run held in LDS, whose length is at
// most hop (own - 1) + win plus n_fft / 2 + 1 reflected samples at either end
int gf_own(int n_fft, int win, int hop) {
    const int images = 2 * GF_IMG / n_fft, halo = (win + hop - 1) / hop - 1;
    int own = images - 2 * halo >= images / 2 ? images - 2 * halo : images;
    while (own > 1 && (long long)hop * (own - 1) + win + n_fft + 2 > GF_SEG) --own;
    return own;
}

size_t gf_plane(int B, int n_bins, int n_frames) { return (size_t)B * n_frames * n_bins; }

}  // namespace

extern "C" {

int unetrir_griffinlim_fft_supported(int n_bins, int n_frames, int n_fft, int win_length, int hop_length) {
    return gf_supported(n_bins, n_frames, n_fft, win_length, hop_length) ? 1 : 0;
}

size_t unetrir_griffinlim_fft_ws_bytes(int B, int n_bins, int n_frames, int n_fft, int win_length, int hop_length) {
    if (B <= 0 || B > 65535 || !gf_supported(n_bins, n_frames, n_fft, win_length, hop_length)) return 0;
    return ((7 * gf_plane(B, n_bins, n_frames) + 1) / 2) * 2 * sizeof(float);
}

int unetrir_griffinlim_fft_f32(const float* feat, int B, int H, int W, int n_bins, int n_frames, int n_fft, int win_length, int hop_length,
                               int pad_mode, int denormalize, int n_iter, float momentum, const float* init_phase, unsigned long long seed,
                               unsigned long long draw, float* wav, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!feat || !wav || !ws || ((uintptr_t)ws & 7) || B <= 0 || B > 65535 ||
        !gf_supported(n_bins, n_frames, n_fft, win_length, hop_length) || n_bins > H || n_frames > W || n_iter < 0 || !(momentum >= 0.f) ||
        !isfinite(momentum) || (pad_mode != 0 && pad_mode != 1) ||
        ws_bytes < unetrir_griffinlim_fft_ws_bytes(B, n_bins, n_frames, n_fft, win_length, hop_length))
        return UNETRIR_EINVAL;
    GfGeom g = {B, H, W, n_bins, n_frames, n_fft, win_length, hop_length, hop_length * (n_frames - 1)};
    g.n_lo = (n_fft - win_length) / 2;
    g.pad_mode = pad_mode;
    g.own = gf_own(n_fft, win_length, hop_length);
    g.tiles = (n_frames + g.own - 1) / g.own;
    const long long chunk = (long long)hop_length * g.own;
    g.chunk = chunk > GF_SEG ? GF_SEG : (int)chunk;
    g.chunks = (int)(((long long)g.T_out + g.chunk - 1) / g.chunk);
    const size_t P = gf_plane(B, n_bins, n_frames);
    GfWs w;
    w.plane[0] = (cf*)ws;
    w.plane[1] = w.plane[0] + P;
    w.plane[2] = w.plane[1] + P;
    w.S = (float*)(w.plane[2] + P);
    hipStream_t s = (hipStream_t)stream;
    const double m = gl_decimal(momentum);
    const float alpha = (float)(m / (1.0 + m));
    long long blocks = ((long long)P + 255) / 256;
    if (blocks > 4096) blocks = 4096;

    hipLaunchKernelGGL(gf_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, feat, g, denormalize, init_phase, seed, draw, w.S, w.plane[0]);
    for (int j = 0; j <= n_iter; ++j) {                              // launch j reads plane j mod 3 (and the one before), writes the next
        const int mode = j < 2 ? j : 2;
        const cf* cur = w.plane[j % 3];
        const cf* prev = w.plane[(j + 2) % 3];
        if (j < n_iter)
            hipLaunchKernelGGL(gf_iterate_kernel, dim3((unsigned)g.tiles, (unsigned)B), dim3(GF_T), 0, s, g, w.S, cur, prev, mode, alpha,
                               w.plane[(j + 1) % 3]);
        else
            hipLaunchKernelGGL(gf_final_kernel, dim3((unsigned)g.chunks, (unsigned)B), dim3(GF_T), 0, s, g, w.S, cur, prev, mode, alpha, wav);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
