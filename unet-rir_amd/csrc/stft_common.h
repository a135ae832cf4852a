// stft_common.h - what every kernel of the centred Hann STFT pair must agree on to the bit: features.hip (the transforms), waveloss.hip and
// istft_bwd.hip (their gradients), griffinlim.hip and griffinlim_fft.hip (the loop between them), spectralloss.hip and
// spectralloss_fft.hip (the analysis at other resolutions).  A waveform one of them makes is read by another, a loss one of them forms is
// differentiated by another, and the tests hold each to the same fp64 restatement - so the window tap, the twiddle table and the frames
// that reach a sample are written once, here.
//
// None of these carries `#pragma clang fp contract(off)`: none of the bodies they replace did, and the pragma is lexical - a caller's
// does not reach in here.
#pragma once
#include <hip/hip_runtime.h>

// Tap n of the periodic Hann window of win samples centred in n_fft zeros (left pad (n_fft - win) / 2, librosa's pad_center).  The value
// is formed in fp64; T = float is its one rounding, so an fp32 consumer's window is the fp64 consumers' window rounded.
template <typename T>
__device__ __forceinline__ T stft_hann(int n, int n_fft, int win) {
    const int m = n - (n_fft - win) / 2;
    if (m < 0 || m >= win) return (T)0.0;
    return (T)(0.5 - 0.5 * cospi(2.0 * (double)m / (double)win));
}

// The twiddles of one turn, tw_c[n] + i tw_s[n] = exp(2 pi i n / n_fft) from sincospi (exact at the quarter turns), and, where wtab is
// given, the padded window.  Every thread of the workgroup calls it with the workgroup's size as `stride` - a constant where the launch
// fixes it, blockDim.x (taken as the unsigned it is) where not; the caller's next barrier stands behind the tables.
template <typename S>
__device__ __forceinline__ void stft_tables(double* tw_c, double* tw_s, double* wtab, int n_fft, int win, S stride) {
    for (int n = threadIdx.x; n < n_fft; n += stride) {
        double sn, cs;
        sincospi(2.0 * (double)n / (double)n_fft, &sn, &cs);
        tw_c[n] = cs; tw_s[n] = sn;
        if (wtab) wtab[n] = stft_hann<double>(n, n_fft, win);
    }
}

// The frames f_lo ... f_hi (none where f_hi < f_lo) of F whose non-zero taps [n_lo, n_lo + win) reach the padded position j (= sample
// index + n_fft / 2): n_lo <= j - hop f < n_lo + win.  Every overlap-add here is a gather over this range in ascending order.  A
// position left of every window, j < n_lo, has no frame, but the division would round its f_hi up to 0, so it is looked for - unless
// the caller says LEFT_PAD = false: it only asks for positions of output samples, j >= n_fft / 2 > n_lo (the Griffin-Lim kernels,
// which pay the range per tap and per sample).  Who folds the left padding back (sl_ola) does go there.
template <bool LEFT_PAD = true>
__device__ __forceinline__ void stft_frame_range(int j, int n_lo, int win, int hop, int F, int& f_lo, int& f_hi) {
    const int num = j - (n_lo + win) + 1;
    f_lo = num <= 0 ? 0 : (num + hop - 1) / hop;
    f_hi = LEFT_PAD && j < n_lo ? -1 : (j - n_lo) / hop;
    if (f_hi > F - 1) f_hi = F - 1;
}
