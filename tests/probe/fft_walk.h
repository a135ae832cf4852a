// fft_walk.h - csrc/fft_lds.h walked thread by thread on the host: the arithmetic of the device transform, one "thread" after the other.
// Test-only (tests/probe/fft_probe.hip and tests/probe/fft_walk_main.cpp); includes fft_lds.h and nothing else of the product.
//
// A pass is fl_pass_load for every thread t of M / 8 into saved registers (everything is read before the barrier), then fl_pass_store
// for every t; the real split is fl_split_fwd / fl_split_inv for every t.  `order` chooses the order in which the threads of the
// store half and of the split are walked: 0 ascending, 1 descending, 2 a fixed shuffle.  The header claims that the stores of a pass
// are disjoint and that a thread owns the pairs of the split it touches, so the three must give the same bits.
//
// Modes (images in natural order, M float2 in and out; a packed real spectrum has (A[0], A[M]) in slot 0):
//   0  complex forward                      fl_fft<M, -1>
//   1  complex inverse, unnormalised        fl_fft<M, +1>
//   2  real forward of 2 M samples          fl_fft<M, -1>, fl_split_fwd<M>            -> the packed spectrum
//   3  real inverse of a packed spectrum    fl_split_inv<M>, barrier, fl_fft<M, +1>   -> the signal times 2 M
// `stop` >= 0 ends the walk after pass `stop` (the split counts as a pass, in the place the mode gives it) and returns the image as it
// stands; `stop` < 0 runs everything.
#pragma once
#include "fft_lds.h"

namespace fftwalk {

using fftlds::cf;

constexpr int N_MODES = 4, N_ORDERS = 3;

inline bool valid_m(int M) { return M == 64 || M == 128 || M == 256 || M == 512 || M == 1024 || M == 2048; }

// the i-th thread to be walked of T (a power of two >= 8): 5 i + 3 mod T is a bijection as 5 is odd
inline int thread_at(int i, int T, int order) { return order == 0 ? i : order == 1 ? T - 1 - i : (5 * i + 3) & (T - 1); }

struct Walk {
    int order, left;                                    // left: passes still to run
};

template <int M, int DIR, int NS = 1>
void fft(cf* buf, Walk& w) {
    if constexpr (NS < M) {
        if (w.left == 0) return;
        --w.left;
        constexpr int R = fftlds::fl_radix(M, NS), T = M / 8;
        cf v[T][8];
        for (int t = 0; t < T; ++t) fftlds::fl_pass_load<M, R>(buf, t, v[t]);
        // the barrier
        for (int i = 0; i < T; ++i) {
            const int t = thread_at(i, T, w.order);
            fftlds::fl_pass_store<M, R, NS, DIR>(buf, t, v[t]);
        }
        fft<M, DIR, NS * R>(buf, w);
    }
}

template <int M, bool INV>
void split(cf* buf, Walk& w) {
    if (w.left == 0) return;
    --w.left;
    constexpr int T = M / 8;
    for (int i = 0; i < T; ++i) {
        const int t = thread_at(i, T, w.order);
        if (INV) fftlds::fl_split_inv<M>(buf, t, T);
        else fftlds::fl_split_fwd<M>(buf, t, T);
    }
}

// one image: in and out are M elements in natural order, buf is the "LDS" image of exactly M elements
template <int M, int MODE>
void image(const cf* in, cf* out, cf* buf, int order, int stop) {
    Walk w{order, stop < 0 ? 1 << 30 : stop + 1};
    for (int i = 0; i < M; ++i) buf[fftlds::fl_swz(i)] = in[i];
    if (MODE == 0) fft<M, -1>(buf, w);
    if (MODE == 1) fft<M, 1>(buf, w);
    if (MODE == 2) {
        fft<M, -1>(buf, w);
        split<M, false>(buf, w);
    }
    if (MODE == 3) {
        split<M, true>(buf, w);
        fft<M, 1>(buf, w);
    }
    for (int i = 0; i < M; ++i) out[i] = buf[fftlds::fl_swz(i)];
}

template <int M>
void image_m(int mode, const cf* in, cf* out, cf* buf, int order, int stop) {
    switch (mode) {
        case 0: image<M, 0>(in, out, buf, order, stop); break;
        case 1: image<M, 1>(in, out, buf, order, stop); break;
        case 2: image<M, 2>(in, out, buf, order, stop); break;
        default: image<M, 3>(in, out, buf, order, stop); break;
    }
}

// n_img images [n_img][M] -> [n_img][M]; the image buffer is a heap block of exactly M elements.  0, or 1 for arguments out of range.
inline int run(int M, int mode, int order, int stop, const cf* in, cf* out, long n_img) {
    if (!valid_m(M) || mode < 0 || mode >= N_MODES || order < 0 || order >= N_ORDERS || n_img < 0) return 1;
    cf* buf = new cf[M];
    for (long n = 0; n < n_img; ++n) {
        const cf* a = in + n * M;
        cf* b = out + n * M;
        switch (M) {
            case 64: image_m<64>(mode, a, b, buf, order, stop); break;
            case 128: image_m<128>(mode, a, b, buf, order, stop); break;
            case 256: image_m<256>(mode, a, b, buf, order, stop); break;
            case 512: image_m<512>(mode, a, b, buf, order, stop); break;
            case 1024: image_m<1024>(mode, a, b, buf, order, stop); break;
            default: image_m<2048>(mode, a, b, buf, order, stop); break;
        }
    }
    delete[] buf;
    return 0;
}

// fl_w<-1>(t) in out[t] and fl_w<+1>(t) in out[4096 + t], 0 <= t < 4096
inline void table(cf* out) {
    for (int t = 0; t < 2 * fftlds::FL_TAB; ++t) {
        out[t] = fftlds::fl_w<-1>(t);
        out[2 * fftlds::FL_TAB + t] = fftlds::fl_w<1>(t);
    }
}

}  // namespace fftwalk
