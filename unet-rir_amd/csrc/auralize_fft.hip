// auralize_fft.hip - the FFT form of auralize: y_b = h_b * x_b by uniform partitioned overlap-save, transforms in LDS (fft_lds.h), gfx950.
//
//     y_b[n] = sum_{k=0}^{K-1} h_b[k] x_b[n - k]          0 <= n < L <= N + K - 1,   x_b[m] = 0 outside 0 <= m < N
//
// Formulation.  Block P = 2048 for every K, real transforms of 2P = 4096 samples (a 2048-point complex FFT + split: 16 KB of LDS).
// Q = ceil(K / P) partitions of h, J = ceil(L / P) output blocks anchored at n = 0:
//     H_q = rfft(h[qP ... (q+1)P) | 0_P)                              q in [0, Q)      (zeros beyond K)
//     X_i = rfft(x[(i-1)P ... (i+1)P))                                i in [0, J)      (zeros outside 0 <= m < N)
//     Y_j = sum_{q = 0}^{min(j, Q-1)} H_q X_{j-q}                     ascending q, fp32 complex, the first product added to +0
//     out[jP ... (j+1)P) = the LAST P samples of irfft(Y_j)           (the first P are the circular wrap-around)
// A spectrum is packed as fft_lds.h packs it: 2048 float2, bin 0 and bin 2048 (both real) in slot 0, multiplied separately.
//
// Launches: two.  (1) one workgroup per spectrum, B Q of h then J (x shared, dry_stride = 0: computed once for all rows) or B J of x,
// into the workspace [H: B][Q][2048] [X: 1 or B][J][2048] float2;  (2) one workgroup per row and pair of output blocks (2g, 2g + 1): the
// products of both accumulate in registers (8 bins per thread and block, spectra read 16 bytes per lane; a step q reads H_q and one new
// X, which serves block 2g now and block 2g + 1 at step q + 1: 2Q + 1 spectra for two blocks instead of 4Q), then per block inverse
// split, inverse FFT and one store per output sample, scaled by the exact 2^-12.  The pairing decides what is read when, not what is
// computed: each Y_j is the same sequence of operations whatever its place in a pair, and the complex products and the sums around them
// are written as explicit fused multiply-adds / unfused sums (contraction off), so the bits do not depend on how the loop was compiled.
// No atomics, no host synchronisation, nothing cleared; every element of out written once and nothing beyond it.
//
// Bits.  The block grid is anchored at n = 0 and P is a constant, so the bits of out[b][n] depend on (h_b, x_b, n) alone: not on B,
// the row's place, L (J only decides which blocks exist), shared or per-row x, or N beyond the samples themselves (an x window past N
// is the same zeros as explicit zeros, and every q <= min(j, Q-1) is summed whether or not its window is empty).
//
// Error.  Per element n of block j, with u = 2^-24, Q_j = min(j, Q-1) + 1 and s_j = sum_{q < Q_j} |h_q|_1 |x[(j-q-1)P ... (j-q+1)P)|_2:
//     |out[n] - y[n]| <= u (19 log2(2P) + 8 + Q_j) s_j                                                     (first order in u)
// derived (not fitted) as follows.  A transform of 2P real points is log2(P) radix-2 levels (a radix-8 pass is three of them: at most
// one complex product by a correctly rounded twiddle, |w^ - w| <= u, and one sum per element and level) plus the split, one more such
// level with a second sum: log2(2P) levels.  (a) Componentwise, every input reaches every output along one path, per level a factor
// (1 + u)(1 + sqrt(2) 2u)(1 + u) (twiddle, product [Higham, Accuracy and Stability, (3.13)], sum): |H^_q[k] - H_q[k]| <= 4.83 u
// log2(2P) |h_q|_1, hence |(H^_q - H_q) X|_2 <= 4.83 u log2(2P) |h_q|_1 |X|_2.  (b) In L2 a level costs eta = u + 4 sqrt(2) u = 6.66 u
// [Higham, Theorem 24.2]: |X^ - X|_2 <= 6.66 u log2(2P) |X|_2 and |H_q (X^ - X)|_2 <= |h_q|_1 6.66 u log2(2P) |X|_2, as |H_q[k]| <=
// |h_q|_1.  (c) The product rounds by sqrt(2) 2u = 2.83 u and the ascending sum of Q_j terms by (Q_j - 1) u of sum_q |H_q X_{j-q}|_2.
// (d) The inverse adds 6.66 u log2(2P) of |Y_j|_2 <= sum_q |h_q|_1 |X_{j-q}|_2 and carries the errors before it over unchanged
// (Parseval: |X|_2 = sqrt(2P) |x|_2 cancels the 1 / sqrt(2P) of the inverse); the scaling by 2^-12 is exact.  Sum: (4.83 + 2 x 6.66)
// log2(2P) + 2.83 + Q_j - 1 = 18.15 log2(2P) + 1.83 + Q_j, and the error of an element is at most the L2 norm of its block's: rounded
// up to c1 = 19, c2 = 8 (the slack covers the split's second sum in each of the three transforms and the second-order terms).  The
// bound is loose by two to five orders of magnitude on random data (errors add like a random walk, not in phase): the tests also hold
// integer data to round(out) == y.
//
// Not exact on integer data (the direct form is); a non-finite sample spoils the whole blocks its window feeds, not K outputs.
//
// Two more forms on the same helpers follow further down, each with its own header: auralize_path (a moving listener: crossfaded
// responses) and the stream (the stationary form block by block with its state carried between calls).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"
#include "fft_lds.h"

namespace {

using namespace fftlds;

constexpr int AF_P = 2048;                              // block; the real transform has 2 AF_P points
constexpr int AF_M = AF_P;                              // complex points of that transform
constexpr int AF_THREADS = AF_M / 8;
constexpr int AF_MAXK = 16384;
constexpr size_t AF_SPEC = AF_M * sizeof(cf);           // bytes of a packed spectrum
constexpr int AF_G = 2;                                 // consecutive output blocks per workgroup of the second launch

// The image of the real window a[m] = src[lo + m], m in [0, 2P), as z[i] = a[2i] + i a[2i+1]; zero for m >= mlim and outside [0, n)
FL_HD void af_load(cf* buf, const float* __restrict__ src, long long lo, long long n, int mlim, int t) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int i = t + AF_THREADS * e, m = 2 * i;
        const long long s = lo + m;
        cf z;
        z.x = (m < mlim && s >= 0 && s < n) ? src[s] : 0.f;
        z.y = (m + 1 < mlim && s + 1 >= 0 && s + 1 < n) ? src[s + 1] : 0.f;
        buf[fl_swz(i)] = z;
    }
}

// bins 2 i and 2 i + 1 of the image, i = t + 256 e: 16 bytes per lane
FL_HD void af_store_spec(float4* __restrict__ spec, const cf* buf, int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = t + AF_THREADS * e;
        const cf a = buf[fl_swz(2 * i)], b = buf[fl_swz(2 * i + 1)];
        spec[i] = make_float4(a.x, a.y, b.x, b.y);
    }
}

// a thread's 8 bins of one spectrum: bins 2 i and 2 i + 1, i = t + 256 e, 16 bytes per lane and load
struct AfBins {
    float4 v[4];
};
FL_HD void af_read(AfBins& d, const float4* __restrict__ S, int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) d.v[e] = S[t + AF_THREADS * e];
}

// acc += h x on the thread's 8 bins; slot 0 holds the two real bins 0 and P
FL_HD void af_mac(cf (&acc)[8], const AfBins& h, const AfBins& x, int t) {
#pragma clang fp contract(off)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        cf p0 = fl_mul(cf{h.v[e].x, h.v[e].y}, cf{x.v[e].x, x.v[e].y});
        const cf p1 = fl_mul(cf{h.v[e].z, h.v[e].w}, cf{x.v[e].z, x.v[e].w});
        if (e == 0 && t == 0) p0 = {h.v[0].x * x.v[0].x, h.v[0].y * x.v[0].y};
        acc[2 * e] = {acc[2 * e].x + p0.x, acc[2 * e].y + p0.y};
        acc[2 * e + 1] = {acc[2 * e + 1].x + p1.x, acc[2 * e + 1].y + p1.y};
    }
}

// Y_{j0 + g} = sum_q H_q X_{j0 + g - q} for g = 0 ... gmax (< G) at once, each in ascending q from +0: step q reads H_q and ONE new
// spectrum of x, X_{j0 - q}; the other G - 1 it needs are still in registers from the steps before (X_i sits in slot (i - j0) mod G, so
// the q loop is unrolled by G to keep the slots static).  H (this row's spectra) and X are indexed by spectrum, AF_M / 2 float4 each.
// slot(i): where spectrum X_i lies in X - i itself for the one-shot forms, i mod S through a stream's ring.
struct AfLinear {
    FL_HD int operator()(int i) const { return i; }
};
template <int G, class Slot = AfLinear>
FL_HD void af_accumulate(cf (&acc)[G][8], const float4* __restrict__ H, const float4* __restrict__ X, int j0, int gmax, int Q, int t,
                         Slot slot = Slot()) {
    AfBins x[G], h;
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = {0.f, 0.f};
#pragma unroll
    for (int g = 1; g < G; ++g)
        if (g <= gmax) af_read(x[g], X + (size_t)slot(j0 + g) * (AF_M / 2), t);
    const int qn = (j0 + gmax < Q - 1 ? j0 + gmax : Q - 1) + 1;
    for (int qq = 0; qq < qn; qq += G) {
#pragma unroll
        for (int s = 0; s < G; ++s) {
            const int q = qq + s;
            if (q < qn) {
                af_read(h, H + (size_t)q * (AF_M / 2), t);
                if (q <= j0) af_read(x[(G - s) % G], X + (size_t)slot(j0 - q) * (AF_M / 2), t);
#pragma unroll
                for (int g = 0; g < G; ++g)
                    if (g <= gmax && q <= j0 + g) af_mac(acc[g], h, x[(g - s + G) % G], t);
            }
        }
    }
}

FL_HD void af_store_acc(cf* buf, const cf (&acc)[8], int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = t + AF_THREADS * e;
        buf[fl_swz(2 * i)] = acc[2 * e];
        buf[fl_swz(2 * i + 1)] = acc[2 * e + 1];
    }
}

// The last P samples of the inverse: z[P/2 + i] holds samples P + 2 i and P + 2 i + 1 of the block that starts at n0, times 2 M
FL_HD void af_store_out(float* __restrict__ y, const cf* buf, long long n0, long long L, int t) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int i = t + AF_THREADS * e;
        const cf z = buf[fl_swz(AF_M / 2 + i)];
        const long long n = n0 + 2 * i;
        const float a = z.x * (1.f / (2 * AF_M)), b = z.y * (1.f / (2 * AF_M));
        if (n + 1 < L && ((uintptr_t)(y + n) & 7) == 0) {
            *reinterpret_cast<float2*>(y + n) = make_float2(a, b);
        } else {
            if (n < L) y[n] = a;
            if (n + 1 < L) y[n + 1] = b;
        }
    }
}

// The logical block of this workgroup among n, in a grid padded to a multiple of 8 (a value >= n: nothing to do).  Workgroups are dealt
// round-robin over the 8 XCDs (observed, not promised, and only speed rests on it), so XCD x works the contiguous run of blocks
// [x ceil(n / 8), (x + 1) ceil(n / 8)): consecutive blocks of one row, which read the same spectra, meet in one L2.
__device__ __forceinline__ int af_block(int n) {
    return (int)(blockIdx.x & 7) * ((n + 7) >> 3) + (int)(blockIdx.x >> 3);
}
__host__ unsigned af_grid(long long n) { return (unsigned)((n + 7) / 8 * 8); }

__global__ __launch_bounds__(AF_THREADS) void auralize_fft_spectra_kernel(const float* __restrict__ rir, const float* __restrict__ dry,
                                                                          float4* __restrict__ spec, int K, int N, long long dry_stride,
                                                                          int Q, int J, int nH, int nX) {
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(nH + nX);
    if (blk >= nH + nX) return;
    int id = blk;
    if (id < nH) {
        const int b = id / Q, q = id - b * Q;
        af_load(buf, rir + (size_t)b * K, (long long)q * AF_P, K, AF_P, t);
    } else {
        id -= nH;
        const int r = id / J, i = id - r * J;
        af_load(buf, dry + (long long)r * dry_stride, (long long)(i - 1) * AF_P, N, 2 * AF_P, t);
    }
    __syncthreads();
    fl_fft<AF_M, -1>(buf, t);
    fl_split_fwd<AF_M>(buf, t, AF_THREADS);
    __syncthreads();
    af_store_spec(spec + (size_t)blk * (AF_M / 2), buf, t);
}

template <int G>
__global__ __launch_bounds__(AF_THREADS) void auralize_fft_render_kernel(const float4* __restrict__ spec, float* __restrict__ out, int Q,
                                                                         int J, int JG, int L, int nH, int xrows, int B) {
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(B * JG);
    if (blk >= B * JG) return;
    const int b = blk / JG, j0 = (blk - b * JG) * G;
    const int gmax = J - 1 - j0 < G - 1 ? J - 1 - j0 : G - 1;
    const float4* __restrict__ H = spec + (size_t)b * Q * (AF_M / 2);
    const float4* __restrict__ X = spec + ((size_t)nH + (xrows > 1 ? (size_t)b * J : 0)) * (AF_M / 2);
    cf acc[G][8];
    af_accumulate<G>(acc, H, X, j0, gmax, Q, t);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if (g > gmax) break;
        if (g) __syncthreads();                         // the stores of block g - 1 have read the image
        af_store_acc(buf, acc[g], t);
        __syncthreads();
        fl_split_inv<AF_M>(buf, t, AF_THREADS);
        __syncthreads();
        fl_fft<AF_M, 1>(buf, t);
        af_store_out(out + (size_t)b * L, buf, (long long)(j0 + g) * AF_P, L, t);
    }
}

// Q, J, the spectra of h and of x; false for arguments the kernels do not take
bool af_plan(int B, int K, int N, long long dry_stride, int L, long long& Q, long long& J, long long& nH, long long& nX) {
    if (B < 1 || K < 1 || K > AF_MAXK || N < 1) return false;
    if (L < 1 || (long long)L > (long long)N + K - 1) return false;
    if (dry_stride != 0 && dry_stride < N) return false;
    Q = (K + AF_P - 1) / AF_P;
    J = ((long long)L + AF_P - 1) / AF_P;
    nH = (long long)B * Q;
    nX = (dry_stride == 0 ? 1 : (long long)B) * J;
    return nH + nX <= 0x7ffffff8LL && (long long)B * J <= 0x7ffffff8LL;          // grids are padded to a multiple of 8
}

// ---- auralize_path: a listener that moves past R responses h_0 ... h_{R-1}, node r reached at output sample tau_r (strictly increasing):
//
//     out[n] = sum_r g_r[n] y_r[n],   y_r = h_r * x,   g_r the hat function over the nodes: 1 at tau_r, 0 at tau_{r-1} and tau_{r+1}, linear
//     between; g_0 = 1 for n <= tau_0 and g_{R-1} = 1 for n >= tau_{R-1}.  The gains of a sample sum to 1 and at most two are not 0.
//
// Launches: two.  (1) the spectra kernel above over the B R responses and x.  (2) one workgroup per row b and output block j: it finds
// r_lo (the last node with tau <= jP, else 0) and r_hi (the first with tau >= (j+1)P - 1, else R - 1) by two bisections of `times` that
// every thread makes alike (the outcome is clamped into [0, R) and r_hi >= r_lo whatever the table holds), and for r = r_lo ... r_hi forms
// Y_j^(r) = sum_q H^(r)_q X_{j-q} by af_mac in ascending q from +0 - the stationary kernel's sequence of operations - runs the same inverse
// split, inverse FFT and 2^-12 scaling in the one image, multiplies the thread's 8 samples by the node's gains and adds them up in
// registers; one store per output sample after the last node.  No y_r reaches memory, no atomics, nothing cleared.  Forming the
// products of two neighbouring nodes from one reading of every X_{j-q} (two accumulators) gave the same bits and measured no faster
// for B = 1 and 27 - 41 % SLOWER for B = 8 (profiles/auralize_path.json, nodes_ab; 256 VGPRs against 228): it is not here.
//
// Gains, fp32, per sample n and node r, contraction off:
//     n <  tau_r:  r = 0 ? 1 : n < tau_{r-1} ? 0 : a,          a = float(n - tau_{r-1}) / float(tau_r - tau_{r-1})   (IEEE division)
//     n >= tau_r:  r = R - 1 ? 1 : n >= tau_{r+1} ? 0 : 1 - a,   a = float(n - tau_r) / float(tau_{r+1} - tau_r)
// A gain of 0 adds nothing (the node is skipped for that sample); the first node that counts gives o = g y, the second o = fmaf(g, y, o),
// in ascending r.  A gain of 1 multiplies exactly, so wherever one node has gain 1 - n <= tau_0, n >= tau_{R-1}, every n = tau_r, all of
// R = 1 - out[n] is the bits of the stationary form for that response.
//
// Bits: out[b][n] depends on (h_{b,.}, x_b, times, n) alone - not on the run, B, the row's place, shared or per-row x, L or the workspace.
//
// Error.  With E_r[n] the stationary bound above for h_r and u = 2^-24:
//     |out[n] - sum_r g_r[n] y_r[n]| <= sum_r g_r[n] E_r[n] + 4 u sum_r g_r[n] |y_r[n]|
// The differences n - tau and tau' - tau are exact in fp32 below 2^24 (beyond it each conversion rounds once more, covered by the 4), so
// a^ = a (1 + d), |d| <= u.  The rising node's term a^ y^ then carries the division, the product and the sum: 3 u.  The falling node's
// 1 - a^ is exact for a^ >= 1/2 (Sterbenz) and rounds by u / 2 below; with the product and the sum again 3 u; 4 covers the second order.
// The falling gain also inherits the error of a^: |a d| |y_r| <= u g_{r+1} |y_r|, at most 2^-25 |y_r| - not proportional to g_r; where
// g_r >= 1 / 237 it is below g_r E_r itself (E_r >= 237 u |y_r|, as |y_r[n]| <= s_j), and it is 0 wherever the spacing is a power of two.
//
// Precondition: times strictly increasing, |tau| <= 2^30.  Otherwise the result is unspecified; nothing outside out and ws is touched.
// Cost: one product chain (Q_j spectra of h, Q_j of x) and one inverse transform per node that touches a block.
FL_HD float ap_gain(long long n, int r, int R, long long tp, long long tc, long long tn) {
#pragma clang fp contract(off)
    if (n < tc) {
        if (r == 0) return 1.f;
        if (n < tp) return 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
        return __fdiv_rn((float)(n - tp), (float)(tc - tp));
#else
        return (float)(n - tp) / (float)(tc - tp);
#endif
    }
    if (r == R - 1) return 1.f;
    if (n >= tn) return 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
    return 1.f - __fdiv_rn((float)(n - tc), (float)(tn - tc));
#else
    return 1.f - (float)(n - tc) / (float)(tn - tc);
#endif
}

__global__ __launch_bounds__(AF_THREADS) void auralize_path_render_kernel(const float4* __restrict__ spec, const int* __restrict__ times,
                                                                          float* __restrict__ out, int R, int Q, int J, int L, int nH,
                                                                          int xrows, int B) {
#pragma clang fp contract(off)
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(B * J);
    if (blk >= B * J) return;
    const int b = blk / J, j = blk - b * J;
    const long long n0 = (long long)j * AF_P, n1 = n0 + AF_P - 1;
    int lo = 0, hi = R;                                 // the first node with tau > n0
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (times[mid] <= n0) lo = mid + 1; else hi = mid;
    }
    const int r_lo = lo > 0 ? lo - 1 : 0;
    lo = 0, hi = R;                                     // the first node with tau >= n1
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (times[mid] < n1) lo = mid + 1; else hi = mid;
    }
    int r_hi = lo < R ? lo : R - 1;
    if (r_hi < r_lo) r_hi = r_lo;
    const size_t node_stride = (size_t)Q * (AF_M / 2);
    const float4* __restrict__ H = spec + (size_t)b * R * node_stride;
    const float4* __restrict__ X = spec + ((size_t)nH + (xrows > 1 ? (size_t)b * J : 0)) * (AF_M / 2);
    float o[8];
    unsigned have = 0;                                  // bit s: sample s of the thread has its first term
#pragma unroll
    for (int s = 0; s < 8; ++s) o[s] = 0.f;
    for (int r = r_lo; r <= r_hi; ++r) {
        cf acc[1][8];
        af_accumulate<1>(acc, H + (size_t)r * node_stride, X, j, 0, Q, t);     // Y_j of node r: the stationary kernel's own chain
        if (r > r_lo) __syncthreads();                  // the blend of the node before has read the image
        af_store_acc(buf, acc[0], t);
        __syncthreads();
        fl_split_inv<AF_M>(buf, t, AF_THREADS);
        __syncthreads();
        fl_fft<AF_M, 1>(buf, t);
        const long long tp = times[r > 0 ? r - 1 : 0], tc = times[r], tn = times[r < R - 1 ? r + 1 : r];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = t + AF_THREADS * e;
            const cf z = buf[fl_swz(AF_M / 2 + i)];
            const long long n = n0 + 2 * i;
            const float y[2] = {z.x * (1.f / (2 * AF_M)), z.y * (1.f / (2 * AF_M))};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float gn = ap_gain(n + k, r, R, tp, tc, tn);
                const unsigned bit = 1u << (2 * e + k);
                if (gn != 0.f) {
                    o[2 * e + k] = (have & bit) ? fmaf(gn, y[k], o[2 * e + k]) : gn * y[k];
                    have |= bit;
                }
            }
        }
    }
    float* __restrict__ yrow = out + (size_t)b * L;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long n = n0 + 2 * (t + AF_THREADS * e);
        if (n + 1 < L && ((uintptr_t)(yrow + n) & 7) == 0) {
            *reinterpret_cast<float2*>(yrow + n) = make_float2(o[2 * e], o[2 * e + 1]);
        } else {
            if (n < L) yrow[n] = o[2 * e];
            if (n + 1 < L) yrow[n + 1] = o[2 * e + 1];
        }
    }
}

// af_plan for B R responses; false in addition for R < 1 and for more responses than an int counts
bool ap_plan(int B, int R, int K, int N, long long dry_stride, int L, long long& Q, long long& J, long long& nH, long long& nX) {
    if (B < 1 || R < 1 || (long long)B * R > 0x7fffffffLL) return false;
    if (!af_plan(B, K, N, dry_stride, L, Q, J, nH, nX)) return false;
    nH = (long long)B * R * Q;
    return nH + nX <= 0x7ffffff8LL;
}

// ---- AuralizeStream: the stationary form block by block, its state carried between calls, and a response exchanged while audio runs.
//
// Partitioned overlap-save is a streaming algorithm: output block j needs X_j ... X_{j-Q+1} and nothing else of x.  A stream keeps
//     state = [control: 64 bytes] [H: 2][B][Q] spectra [X: xrows][S] spectra [carry: xrows][P] floats,     S = Q + max_blocks - 1
// X_i in ring slot i mod S (a push of at most max_blocks blocks writes X_c ... X_{c+blocks-1} and reads back to X_{c-Q+1}: at most S
// distinct spectra), the carry = the last P dry samples, the first half of the next window.  Control, on the device so that a push has
// the same launch arguments every time (capturable): count c of blocks rendered (64-bit), the current H slot, whether a fade is pending.
//
// push = three launches.  (a) X_{c+i} = rfft(carry | new) for i = 0, rfft(new[(i-1)P ... (i+1)P)) beyond: the spectra kernel's transform
// on the same sample values, so the same bits.  (b) one workgroup per row and pair of blocks (c + 2g, c + 2g + 1): af_accumulate<2> -
// the stationary render's own chain, reading X through the ring - inverse split, inverse FFT, 2^-12 scaling, store.  With a fade pending
// the first workgroup of a row renders block c through the old and then the new response by af_accumulate<1> and blends them with
// ap_gain for the two nodes (old at cP, new at (c+1)P) and the path kernel's accumulate sequence, then block c + 1 through the new
// response alone; every other workgroup uses the new response.  (c) the last P new samples into the carry, c += blocks, and after a
// fade the new slot becomes current.  (c) cannot be folded into (a) or (b): their other workgroups still read carry and control.
// An index into the ring never needs j itself: the chain sees j clamped to AS_JCLAMP >= Q - 1 (it only compares j with q < Q) and the
// ring's base makes up the difference.
//
// Tried: the fade in a kernel of its own chosen on the host - that needs the flag on the host, a synchronisation or a second set of
// launch arguments, and a captured push could no longer follow an update.  It is a branch of the one kernel, uniform over the grid.
// Registers (the compiler's report): the stationary branch alone 168 VGPRs, as the one-shot render; with the fade written out as three
// chains 272 - 276; as ONE loop of three passes over one copy of the chain 252, no spills: two waves per SIMD for both branches.
// Holding it to 256 by an occupancy attribute instead spilled 14 registers.
struct AsCtrl {
    long long count;                                    // blocks rendered since init
    int cur;                                            // the H slot that is heard
    int pending;                                        // 1: the other slot holds a response to fade in at the next block
    int pad[12];
};
static_assert(sizeof(AsCtrl) == 64, "the control words take the first 64 bytes of a stream's state");
constexpr int AS_MAXBLOCKS = 64;
constexpr int AS_JCLAMP = 16;                           // >= AF_MAXK / AF_P - 1 + AF_G

struct AsRing {
    int base, S;                                        // base = (j - min(j, AS_JCLAMP)) mod S
    FL_HD int operator()(int i) const { return (base + i) % S; }
};

struct AsPlan {
    long long Q, S, nH, nX;
    size_t bytes;
};

bool as_plan(int B, int K, int dry_rows, int max_blocks, AsPlan& p) {
    if (B < 1 || K < 1 || K > AF_MAXK || max_blocks < 1 || max_blocks > AS_MAXBLOCKS) return false;
    if (dry_rows != 1 && dry_rows != B) return false;
    p.Q = (K + AF_P - 1) / AF_P;
    p.S = p.Q + max_blocks - 1;
    p.nH = (long long)B * p.Q;
    p.nX = (long long)dry_rows * p.S;
    if (2 * p.nH + p.nX > 0x7ffffff8LL || (long long)B * max_blocks > 0x7ffffff8LL) return false;          // grids are padded to 8
    p.bytes = sizeof(AsCtrl) + (size_t)(2 * p.nH + p.nX) * AF_SPEC + (size_t)dry_rows * AF_P * sizeof(float);
    return true;
}

// The spectra of rir [B][K] into H slot 0 (init) or the slot that is not current (update, which also marks the fade)
__global__ __launch_bounds__(AF_THREADS) void auralize_stream_response_kernel(const float* __restrict__ rir, AsCtrl* ctrl,
                                                                              float4* __restrict__ Hs, int K, int Q, int nH, int update) {
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(nH);
    if (blk >= nH) return;
    const int slot = update ? 1 - (ctrl->cur & 1) : 0;
    const int b = blk / Q, q = blk - b * Q;
    af_load(buf, rir + (size_t)b * K, (long long)q * AF_P, K, AF_P, t);
    __syncthreads();
    fl_fft<AF_M, -1>(buf, t);
    fl_split_fwd<AF_M>(buf, t, AF_THREADS);
    __syncthreads();
    af_store_spec(Hs + ((size_t)slot * nH + blk) * (AF_M / 2), buf, t);
    if (update && blk == 0 && t == 0) ctrl->pending = 1;         // nobody reads this word in this launch
}

// (a): X_{c+i}, i in [0, blocks), per dry row; dry null: zeros
__global__ __launch_bounds__(AF_THREADS) void auralize_stream_spectra_kernel(const float* __restrict__ dry, long long dry_stride,
                                                                             const AsCtrl* __restrict__ ctrl,
                                                                             const float* __restrict__ carry, float4* __restrict__ X,
                                                                             int S, int blocks, int xrows) {
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(xrows * blocks);
    if (blk >= xrows * blocks) return;
    const int r = blk / blocks, i = blk - r * blocks;
    const float* __restrict__ row = dry ? dry + (long long)r * dry_stride : nullptr;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = t + AF_THREADS * e, m = 2 * k;                // m and m + 1 lie in the same half of the window
        cf z = {0.f, 0.f};
        if (m < AF_P && i == 0) {
            z = {carry[(size_t)r * AF_P + m], carry[(size_t)r * AF_P + m + 1]};
        } else if (row) {
            const long long s = (long long)(i - 1) * AF_P + m;
            z = {row[s], row[s + 1]};
        }
        buf[fl_swz(k)] = z;
    }
    __syncthreads();
    fl_fft<AF_M, -1>(buf, t);
    fl_split_fwd<AF_M>(buf, t, AF_THREADS);
    __syncthreads();
    const int slot = (int)((ctrl->count + i) % S);
    af_store_spec(X + ((size_t)r * S + slot) * (AF_M / 2), buf, t);
}

// The inverse of one accumulated block, as the stationary render does it; the image holds the samples afterwards
FL_HD void as_inverse(cf* buf, const cf (&acc)[8], int t) {
    af_store_acc(buf, acc, t);
    __syncthreads();
    fl_split_inv<AF_M>(buf, t, AF_THREADS);
    __syncthreads();
    fl_fft<AF_M, 1>(buf, t);
}

// (b): one workgroup per row and pair of push-local blocks (2g, 2g + 1)
__global__ __launch_bounds__(AF_THREADS) void auralize_stream_render_kernel(const AsCtrl* __restrict__ ctrl, const float4* __restrict__ Hs,
                                                                            const float4* __restrict__ Xs, float* __restrict__ out,
                                                                            long long out_stride, int Q, int S, int blocks, int NG,
                                                                            int xrows, int B) {
#pragma clang fp contract(off)
    __shared__ cf buf[AF_M];
    const int t = threadIdx.x;
    const int blk = af_block(B * NG);
    if (blk >= B * NG) return;
    const int b = blk / NG, i0 = (blk - b * NG) * AF_G;
    const int gmax = blocks - 1 - i0 < AF_G - 1 ? blocks - 1 - i0 : AF_G - 1;
    const long long j = ctrl->count + i0;               // the stream's block index of this workgroup's first block
    const int cur = ctrl->cur & 1, pending = ctrl->pending;
    const int jq = j < AS_JCLAMP ? (int)j : AS_JCLAMP;
    const AsRing ring{(int)((j - jq) % S), S};
    const size_t row_spec = (size_t)Q * (AF_M / 2);
    const float4* __restrict__ Hold = Hs + ((size_t)cur * B + b) * row_spec;
    const float4* __restrict__ Hnew = Hs + ((size_t)(1 - cur) * B + b) * row_spec;
    const float4* __restrict__ X = Xs + (xrows > 1 ? (size_t)b * S : 0) * (AF_M / 2);
    float* __restrict__ yrow = out + (long long)b * out_stride;
    const long long L = (long long)blocks * AF_P;
    if (!(pending && i0 == 0)) {
        cf acc[AF_G][8];
        af_accumulate<AF_G>(acc, pending ? Hnew : Hold, X, jq, gmax, Q, t, ring);
#pragma unroll
        for (int g = 0; g < AF_G; ++g) {
            if (g > gmax) break;
            if (g) __syncthreads();                     // the stores of block g - 1 have read the image
            as_inverse(buf, acc[g], t);
            af_store_out(yrow, buf, (long long)(i0 + g) * AF_P, L, t);
        }
        return;
    }
    // the fade: block j through the old response (node 0 at jP) and the new one (node 1 at (j+1)P), the path kernel's blend; then
    // (pass 2) its neighbour through the new response alone.  One loop, so that one copy of the chain serves all three passes.
    const long long n0 = j * AF_P, tau[2] = {n0, n0 + AF_P};
    float o[8];
    unsigned have = 0;
#pragma unroll
    for (int s = 0; s < 8; ++s) o[s] = 0.f;
#pragma unroll 1
    for (int pass = 0; pass < 2 + gmax; ++pass) {
        const int r = pass & 1;                         // the node of passes 0 and 1: old, new
        cf acc[1][8];
        af_accumulate<1>(acc, pass ? Hnew : Hold, X, jq + (pass >> 1), 0, Q, t, ring);
        if (pass) __syncthreads();                      // the pass before has read the image
        as_inverse(buf, acc[0], t);
        if (pass == 2) {
            af_store_out(yrow, buf, (long long)AF_P, L, t);
            break;
        }
        const long long tp = tau[0], tc = tau[r], tn = tau[1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = t + AF_THREADS * e;
            const cf z = buf[fl_swz(AF_M / 2 + i)];
            const long long n = n0 + 2 * i;
            const float y[2] = {z.x * (1.f / (2 * AF_M)), z.y * (1.f / (2 * AF_M))};
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float gn = ap_gain(n + k, r, 2, tp, tc, tn);
                const unsigned bit = 1u << (2 * e + k);
                if (gn != 0.f) {
                    o[2 * e + k] = (have & bit) ? fmaf(gn, y[k], o[2 * e + k]) : gn * y[k];
                    have |= bit;
                }
            }
        }
        if (pass == 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float* __restrict__ p = yrow + 2 * (t + AF_THREADS * e);          // block 0 of the push: always whole
                if (((uintptr_t)p & 7) == 0) {
                    *reinterpret_cast<float2*>(p) = make_float2(o[2 * e], o[2 * e + 1]);
                } else {
                    p[0] = o[2 * e];
                    p[1] = o[2 * e + 1];
                }
            }
        }
    }
}

// (c): what the next push starts from
__global__ __launch_bounds__(AF_THREADS) void auralize_stream_advance_kernel(const float* __restrict__ dry, long long dry_stride,
                                                                             AsCtrl* ctrl, float* __restrict__ carry, int blocks) {
    const int t = threadIdx.x, r = blockIdx.x;
    const float* __restrict__ last = dry ? dry + (long long)r * dry_stride + (long long)(blocks - 1) * AF_P : nullptr;
#pragma unroll
    for (int e = 0; e < AF_P / AF_THREADS; ++e) {
        const int m = t + AF_THREADS * e;
        carry[(size_t)r * AF_P + m] = last ? last[m] : 0.f;
    }
    if (r == 0 && t == 0) {
        ctrl->count += blocks;
        if (ctrl->pending) {
            ctrl->cur = 1 - (ctrl->cur & 1);
            ctrl->pending = 0;
        }
    }
}

struct AsState {
    AsCtrl* ctrl;
    float4 *H, *X;
    float* carry;
};

// The parts of a state that passed the checks every entry point makes; false: refuse
bool as_state(void* state, size_t state_bytes, int B, int K, int dry_rows, int max_blocks, AsPlan& p, AsState& s) {
    if (!state || ((uintptr_t)state & 15) || !as_plan(B, K, dry_rows, max_blocks, p) || state_bytes < p.bytes) return false;
    char* base = static_cast<char*>(state);
    s.ctrl = reinterpret_cast<AsCtrl*>(base);
    s.H = reinterpret_cast<float4*>(base + sizeof(AsCtrl));
    s.X = s.H + (size_t)(2 * p.nH) * (AF_M / 2);
    s.carry = reinterpret_cast<float*>(s.X + (size_t)p.nX * (AF_M / 2));
    return true;
}

}  // namespace

extern "C" {

int unetrir_auralize_stream_supported(int K) { return K >= 1 && K <= AF_MAXK ? 1 : 0; }

size_t unetrir_auralize_stream_state_bytes(int B, int K, int dry_rows, int max_blocks) {
    AsPlan p;
    return as_plan(B, K, dry_rows, max_blocks, p) ? p.bytes : 0;
}

int unetrir_auralize_stream_init(void* state, size_t state_bytes, const float* rir, int B, int K, int dry_rows, int max_blocks,
                                 unetrir_stream_t stream) {
    AsPlan p;
    AsState s;
    if (!rir || !as_state(state, state_bytes, B, K, dry_rows, max_blocks, p, s)) return UNETRIR_EINVAL;
    hipError_t e = hipMemsetAsync(state, 0, p.bytes, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(auralize_stream_response_kernel, dim3(af_grid(p.nH)), dim3(AF_THREADS), 0, (hipStream_t)stream, rir, s.ctrl, s.H, K,
                       (int)p.Q, (int)p.nH, 0);
    return (int)hipGetLastError();
}

int unetrir_auralize_stream_update(void* state, size_t state_bytes, const float* rir, int B, int K, int dry_rows, int max_blocks,
                                   unetrir_stream_t stream) {
    AsPlan p;
    AsState s;
    if (!rir || !as_state(state, state_bytes, B, K, dry_rows, max_blocks, p, s)) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(auralize_stream_response_kernel, dim3(af_grid(p.nH)), dim3(AF_THREADS), 0, (hipStream_t)stream, rir, s.ctrl, s.H, K,
                       (int)p.Q, (int)p.nH, 1);
    return (int)hipGetLastError();
}

int unetrir_auralize_stream_push(void* state, size_t state_bytes, int B, int K, int dry_rows, int max_blocks, const float* dry,
                                 long long dry_stride, float* out, long long out_stride, int blocks, unetrir_stream_t stream) {
    AsPlan p;
    AsState s;
    if (!out || !as_state(state, state_bytes, B, K, dry_rows, max_blocks, p, s)) return UNETRIR_EINVAL;
    if (blocks < 1 || blocks > max_blocks) return UNETRIR_EINVAL;
    const long long n = (long long)blocks * AF_P;
    if (out_stride < n || (dry && !(dry_stride >= n || (dry_stride == 0 && dry_rows == 1)))) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(auralize_stream_spectra_kernel, dim3(af_grid((long long)dry_rows * blocks)), dim3(AF_THREADS), 0,
                       (hipStream_t)stream, dry, dry_stride, (const AsCtrl*)s.ctrl, (const float*)s.carry, s.X, (int)p.S, blocks, dry_rows);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const int NG = (blocks + AF_G - 1) / AF_G;
    hipLaunchKernelGGL(auralize_stream_render_kernel, dim3(af_grid((long long)B * NG)), dim3(AF_THREADS), 0, (hipStream_t)stream,
                       (const AsCtrl*)s.ctrl, (const float4*)s.H, (const float4*)s.X, out, out_stride, (int)p.Q, (int)p.S, blocks, NG,
                       dry_rows, B);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(auralize_stream_advance_kernel, dim3(dry_rows), dim3(AF_THREADS), 0, (hipStream_t)stream, dry, dry_stride, s.ctrl,
                       s.carry, blocks);
    return (int)hipGetLastError();
}

int unetrir_auralize_path_supported(int K) { return K >= 1 && K <= AF_MAXK ? 1 : 0; }

size_t unetrir_auralize_path_ws_bytes(int B, int R, int K, int N, long long dry_stride, int L) {
    long long Q, J, nH, nX;
    return ap_plan(B, R, K, N, dry_stride, L, Q, J, nH, nX) ? (size_t)(nH + nX) * AF_SPEC : 0;
}

int unetrir_auralize_path_f32(const float* rir, const int* times, const float* dry, float* out, int B, int R, int K, int N,
                              long long dry_stride, int L, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    long long Q, J, nH, nX;
    if (!rir || !times || !dry || !out || !ws || !ap_plan(B, R, K, N, dry_stride, L, Q, J, nH, nX)) return UNETRIR_EINVAL;
    if (ws_bytes < (size_t)(nH + nX) * AF_SPEC || ((uintptr_t)ws & 15)) return UNETRIR_EINVAL;
    float4* spec = static_cast<float4*>(ws);
    hipLaunchKernelGGL(auralize_fft_spectra_kernel, dim3(af_grid(nH + nX)), dim3(AF_THREADS), 0, (hipStream_t)stream, rir, dry, spec, K,
                       N, dry_stride, (int)Q, (int)J, (int)nH, (int)nX);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(auralize_path_render_kernel, dim3(af_grid((long long)B * J)), dim3(AF_THREADS), 0, (hipStream_t)stream,
                       (const float4*)spec, times, out, R, (int)Q, (int)J, L, (int)nH, dry_stride == 0 ? 1 : B, B);
    return (int)hipGetLastError();
}

int unetrir_auralize_fft_supported(int K) { return K >= 1 && K <= AF_MAXK ? 1 : 0; }

int unetrir_auralize_fft_block(int K) { return unetrir_auralize_fft_supported(K) ? AF_P : 0; }

size_t unetrir_auralize_fft_ws_bytes(int B, int K, int N, long long dry_stride, int L) {
    long long Q, J, nH, nX;
    return af_plan(B, K, N, dry_stride, L, Q, J, nH, nX) ? (size_t)(nH + nX) * AF_SPEC : 0;
}

int unetrir_auralize_fft_f32(const float* rir, const float* dry, float* out, int B, int K, int N, long long dry_stride, int L, void* ws,
                             size_t ws_bytes, unetrir_stream_t stream) {
    long long Q, J, nH, nX;
    if (!rir || !dry || !out || !ws || !af_plan(B, K, N, dry_stride, L, Q, J, nH, nX)) return UNETRIR_EINVAL;
    if (ws_bytes < (size_t)(nH + nX) * AF_SPEC || ((uintptr_t)ws & 15)) return UNETRIR_EINVAL;
    float4* spec = static_cast<float4*>(ws);
    hipLaunchKernelGGL(auralize_fft_spectra_kernel, dim3(af_grid(nH + nX)), dim3(AF_THREADS), 0, (hipStream_t)stream, rir, dry, spec, K,
                       N, dry_stride, (int)Q, (int)J, (int)nH, (int)nX);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    const long long JG = (J + AF_G - 1) / AF_G;
    hipLaunchKernelGGL(auralize_fft_render_kernel<AF_G>, dim3(af_grid((long long)B * JG)), dim3(AF_THREADS), 0, (hipStream_t)stream,
                       (const float4*)spec, out, (int)Q, (int)J, (int)JG, L, (int)nH, dry_stride == 0 ? 1 : B, B);
    return (int)hipGetLastError();
}

}  // extern "C"
