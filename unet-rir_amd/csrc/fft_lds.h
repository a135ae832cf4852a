// fft_lds.h - a complex fp32 FFT of M = 64 ... 2048 points (a power of two) held in LDS and worked by ONE workgroup of M / 8 threads, and
// the packing that turns it into a real transform of 2 M points.  Self-contained; every function is __host__ __device__ so that the
// same arithmetic can be walked thread by thread on the host.  tests/probe/fft_walk.h is that walk and tests/test_fft_lds.py holds it,
// for M = 64 ... 2048, both directions and the real transform, to an fp64 DFT: relative L2 error per image of uniform data 0.7e-7
// (M = 64) to 1.2e-7 (2048) complex and 0.7e-7 to 1.2e-7 real - the figure depends on the data by +-20 % at M = 64 - which is 0.99 to
// 1.25 times that of pocketfft in complex64 on the same image; an impulse's response is within 5.3 u (complex, real forward) or 9.8 u
// (real inverse) of the closed form at every element, u = 2^-24; and the table below is the correctly rounded fp32 of cos / -sin at
// all 4096 components.  tests/test_fft_lds_gpu.py holds the device to the bits of that walk.  On the device M = 2048 is instantiated
// by auralize_fft.hip and M = 64, 128, 256, 512 by spectralloss_fft.hip, several images side by side in one workgroup: see there;
// M = 1024 by the tests' probe (tests/probe/fft_probe.hip) alone.
//
// Scheme.  Stockham autosort, decimation in time, radix 8 while 8 divides what is left and one last pass of radix 4 or 2 (M = 2048:
// 8 x 8 x 8 x 4, four passes).  A pass of radix R over sub-transforms of NS points (NS = the product of the radices before it):
//     butterfly j (0 <= j < M / R), k = j mod NS:   v[r] = buf[j + r M / R] W_{NS R}^{r k},   V = DFT_R(v),   buf[(j - k) R + k + r NS] = V[r]
// in place: every thread loads its 8 points, the workgroup meets at a barrier, then every thread multiplies, transforms and stores.
// Input and output are both in natural order; nothing is bit-reversed anywhere.  The radix-8 butterfly is three radix-2 levels in
// registers (constants 1, -i, (1 -+ i) sqrt(1/2)).
//
// Twiddles.  W_4096^t = exp(-2 pi i t / 4096), t in [0, 2048), is a table of fp32 pairs: each component is the fp32 nearest to a
// value computed in fp64 from the octant-reduced argument (t is an integer, so the reduction to [0, pi/4] is exact; sin and cos of
// it are Taylor sums to x^21 / x^20, good to ~2 ulp of fp64), evaluated by the compiler.  Every twiddle of every pass and of the real
// split is ONE entry of it (the other half of the circle by a sign): no recurrence, no fast intrinsic.  The table lives in device
// memory (16 KB, resident in the vector L1 after first touch).
//
// Banks.  The image is M float2 = 8 M bytes, not padded but swizzled: point i lives at float2 index
//     fl_swz(i) = i ^ ((i >> 4) & 7) ^ ((i >> 3) & 24)
// (bits 0-2 take bits 4-6, bit 3 takes bit 6, bit 4 takes bit 7: a bijection of every aligned block of 32).  A ds_read_b64 serves 32
// lanes per cycle over 64 4-byte banks, a ds_write_b64 16 lanes over 32: conflict-free means 32 resp. 16 different float2 indices
// modulo 32 resp. 16.  Loads of every pass are 32 consecutive, aligned points: a permutation of one block.  Stores: NS = 1 puts lane j
// at 8 j + r, NS = 8 at 64 (j >> 3) + (j & 7) + 8 r - the swizzle spreads both over all 32 (16) slots; NS >= 64 stores consecutive
// points again.  The split pass reads k and M - k: one lane of a group falls into the neighbouring block (at most 2-way).
//
// Real transform of a[0 ... 2M):  z[n] = a[2n] + i a[2n+1],  Z = FFT_M(z),  and with W = exp(-2 pi i / 2M), for 0 < k <= M / 2
//     E = (Z[k] + conj Z[M-k]) / 2,  O = -i (Z[k] - conj Z[M-k]) / 2,  A[k] = E + W^k O,  A[M-k] = conj(E - W^k O)
// A[0] = Re Z[0] + Im Z[0] and A[M] = Re Z[0] - Im Z[0] are real and share slot 0: the packed spectrum is M float2.  The inverse split
// returns 2 Z and the inverse FFT is unnormalised, so the real signal comes back times 2 M: the caller scales by the exact 1 / 2M.
#pragma once
#include <hip/hip_runtime.h>

namespace fftlds {

#define FL_HD __host__ __device__ __forceinline__

struct alignas(8) cf {
    float x, y;
};

constexpr int FL_TAB = 2048;                            // table entries: half a circle in steps of 1 / 4096 turn
constexpr int FL_MAX_M = FL_TAB;

struct FlTab {
    cf w[FL_TAB];
};

// sin(pi t / 2048) and cos(pi t / 2048) for 0 <= t <= 512 (an octant), fp64 Taylor sums, smallest terms first
constexpr double fl_sin_oct(int t) {
    const double x = 3.14159265358979323846 * t / 2048.0, x2 = x * x;
    double s = 0.0;
    for (int n = 21; n >= 3; n -= 2) s = (s + 1.0) * (-x2 / ((double)n * (n - 1)));
    return x * (s + 1.0);
}
constexpr double fl_cos_oct(int t) {
    const double x = 3.14159265358979323846 * t / 2048.0, x2 = x * x;
    double s = 0.0;
    for (int n = 20; n >= 2; n -= 2) s = (s + 1.0) * (-x2 / ((double)n * (n - 1)));
    return s + 1.0;
}
constexpr FlTab fl_make_tab() {
    FlTab T{};
    for (int t = 0; t < FL_TAB; ++t) {
        const int a = t <= 1024 ? t : 2048 - t;         // angle pi a / 2048 in the first quadrant; cos changes sign beyond it
        const double c = a <= 512 ? fl_cos_oct(a) : fl_sin_oct(1024 - a);
        const double s = a <= 512 ? fl_sin_oct(a) : fl_cos_oct(1024 - a);
        T.w[t].x = (float)(t <= 1024 ? c : -c);
        T.w[t].y = (float)-s;
    }
    return T;
}
static constexpr FlTab fl_tab_host = fl_make_tab();
static __device__ const FlTab fl_tab_dev = fl_make_tab();

// exp(DIR 2 pi i t / 4096), 0 <= t < 4096; DIR = -1 the forward transform, +1 the inverse
template <int DIR>
FL_HD cf fl_w(int t) {
#if defined(__HIP_DEVICE_COMPILE__)
    cf w = fl_tab_dev.w[t & (FL_TAB - 1)];
#else
    cf w = fl_tab_host.w[t & (FL_TAB - 1)];
#endif
    if (t & FL_TAB) w = {-w.x, -w.y};
    if (DIR > 0) w.y = -w.y;
    return w;
}

FL_HD int fl_swz(int i) { return i ^ ((i >> 4) & 7) ^ ((i >> 3) & 24); }

// a b as two products and two fused multiply-adds, whatever the compiler's contraction setting: the bits of a transform do not depend
// on how the surrounding code was compiled
FL_HD cf fl_mul(cf a, cf b) {
#pragma clang fp contract(off)
    return {fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x)};
}
FL_HD void fl_bf(cf& a, cf& b) {
    const cf s = {a.x + b.x, a.y + b.y}, d = {a.x - b.x, a.y - b.y};
    a = s;
    b = d;
}
template <int DIR>
FL_HD cf fl_mul_i(cf a) {                               // a times DIR i
    return DIR < 0 ? cf{a.y, -a.x} : cf{-a.y, a.x};
}

// v <- DFT_R(v), natural order in and out
template <int R, int DIR>
FL_HD void fl_dft(cf (&v)[8]) {
    if constexpr (R == 8) {
        constexpr float h = 0.70710678118654752440f;
        fl_bf(v[0], v[4]); fl_bf(v[1], v[5]); fl_bf(v[2], v[6]); fl_bf(v[3], v[7]);
        v[5] = fl_mul(v[5], cf{h, DIR < 0 ? -h : h});
        v[6] = fl_mul_i<DIR>(v[6]);
        v[7] = fl_mul(v[7], cf{-h, DIR < 0 ? -h : h});
        fl_bf(v[0], v[2]); fl_bf(v[1], v[3]); fl_bf(v[4], v[6]); fl_bf(v[5], v[7]);
        v[3] = fl_mul_i<DIR>(v[3]);
        v[7] = fl_mul_i<DIR>(v[7]);
        fl_bf(v[0], v[1]); fl_bf(v[2], v[3]); fl_bf(v[4], v[5]); fl_bf(v[6], v[7]);
        const cf t1 = v[1], t3 = v[3], t4 = v[4], t6 = v[6];
        v[1] = t4; v[4] = t1; v[3] = t6; v[6] = t3;
    } else if constexpr (R == 4) {
        fl_bf(v[0], v[2]); fl_bf(v[1], v[3]);
        v[3] = fl_mul_i<DIR>(v[3]);
        fl_bf(v[0], v[1]); fl_bf(v[2], v[3]);
        const cf t1 = v[1];
        v[1] = v[2]; v[2] = t1;
    } else {
        fl_bf(v[0], v[1]);
    }
}

constexpr int fl_radix(int M, int NS) { return M / NS >= 8 ? 8 : M / NS; }

// The two halves of a pass for thread t of M / 8: 8 / R butterflies each.  A barrier of the workgroup goes between them and after.
template <int M, int R>
FL_HD void fl_pass_load(const cf* buf, int t, cf (&v)[8]) {
#pragma unroll
    for (int u = 0; u < 8 / R; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r) v[u * R + r] = buf[fl_swz(t + (M / 8) * u + r * (M / R))];
}
template <int M, int R, int NS, int DIR>
FL_HD void fl_pass_store(cf* buf, int t, const cf (&v)[8]) {
#pragma unroll
    for (int u = 0; u < 8 / R; ++u) {
        const int j = t + (M / 8) * u, k = j & (NS - 1);
        cf b[8];
        b[0] = v[u * R];
#pragma unroll
        for (int r = 1; r < R; ++r) b[r] = NS > 1 ? fl_mul(v[u * R + r], fl_w<DIR>(r * k * (4096 / (NS * R)))) : v[u * R + r];
        fl_dft<R, DIR>(b);
#pragma unroll
        for (int r = 0; r < R; ++r) buf[fl_swz((j - k) * R + k + r * NS)] = b[r];
    }
}

// The real split for thread t of T: the packed spectrum A of the real signal from Z = FFT_M(z) (forward, factors 1/2 applied), and
// 2 Z from A (inverse).  A thread owns the pairs (k, M - k) it touches: no barrier inside.
template <int M>
FL_HD void fl_split_fwd(cf* buf, int t, int T) {
#pragma clang fp contract(off)
    for (int k = t; k <= M / 2; k += T) {
        if (k == 0) {
            const cf z = buf[0];                        // fl_swz(0) = 0
            buf[0] = {z.x + z.y, z.x - z.y};
            continue;
        }
        const cf a = buf[fl_swz(k)], b = buf[fl_swz(M - k)];
        const cf E = {0.5f * (a.x + b.x), 0.5f * (a.y - b.y)};
        const cf O = {0.5f * (a.y + b.y), -0.5f * (a.x - b.x)};
        const cf P = fl_mul(fl_w<-1>(k * (FL_TAB / M)), O);
        buf[fl_swz(k)] = {E.x + P.x, E.y + P.y};
        buf[fl_swz(M - k)] = {E.x - P.x, P.y - E.y};
    }
}
template <int M>
FL_HD void fl_split_inv(cf* buf, int t, int T) {
#pragma clang fp contract(off)
    for (int k = t; k <= M / 2; k += T) {
        if (k == 0) {
            const cf a = buf[0];
            buf[0] = {a.x + a.y, a.x - a.y};
            continue;
        }
        const cf a = buf[fl_swz(k)], b = buf[fl_swz(M - k)];
        const cf E = {a.x + b.x, a.y - b.y};
        const cf P = {a.x - b.x, a.y + b.y};
        const cf O = fl_mul(fl_w<1>(k * (FL_TAB / M)), P);
        buf[fl_swz(k)] = {E.x - O.y, E.y + O.x};
        buf[fl_swz(M - k)] = {E.x + O.y, O.x - E.y};
    }
}

#if defined(__HIPCC__)
// buf <- FFT_M(buf) (DIR = -1) or M times its inverse (DIR = +1), in place; called by all M / 8 threads of the workgroup with the image
// complete (the caller's barrier), returns with the result complete (a barrier is the last thing it does).
template <int M, int DIR, int NS = 1>
__device__ __forceinline__ void fl_fft(cf* buf, int t) {
    static_assert(M >= 64 && M <= FL_MAX_M && (M & (M - 1)) == 0, "M is a power of two in 64 ... 2048");
    if constexpr (NS < M) {
        constexpr int R = fl_radix(M, NS);
        cf v[8];
        fl_pass_load<M, R>(buf, t, v);
        __syncthreads();
        fl_pass_store<M, R, NS, DIR>(buf, t, v);
        __syncthreads();
        fl_fft<M, DIR, NS * R>(buf, t);
    }
}
#endif

}  // namespace fftlds
