// resample.hip - sample-rate conversion by a polyphase FIR: y = the rational resampling of x by L / M (gfx950).
//
//     y_b[m] = sum_{i=0}^{T-1} table[p][i] x_b[q - T/2 + 1 + i]        (q, p) = divmod(m M, L),   x_b[n] = 0 outside 0 <= n < N
//
// x fp32 [B][N], table fp32 [L][T] in device memory (resample_table.h builds the Kaiser-windowed sinc one; the kernel does not interpret
// it), y fp32 [B][Nout], 1 <= Nout <= ceil(N L / M).
//
// Tiling.  Write m = j L + r (period j, residue r).  Then q = j M + o(r) and p = (r M) mod L with o(r) = (r M) div L: the table row and
// the offset into x depend on r alone, and a period on moves the window of x by M.  A workgroup (256 threads) owns PT consecutive
// residues x JT consecutive periods.  It stages ONCE, in LDS,
//   - the PT table rows of its residues (row stride S = T rounded up to 4 floats, then to an odd number of float4s: the float4 reads of
//     lanes in different rows fall into different banks), and
//   - the window of x its outputs can reach: (JT - 1) M + (o(r_last) - o(r_first)) + T samples, zeros where x ends.
// Thread t owns residue t % PT and the R periods g + k G (g = t / PT, G = 256 / PT, k < R): consecutive lanes write consecutive outputs
// (runs of PT floats; the whole period where L <= 64), and a table value read from LDS is held in a register for R periods.  Per 4 taps
// a thread issues one 16-byte read of its row and 4 R 4-byte reads of the window for 4 R fmaf: the kernel is bound by LDS reads of x,
// not by arithmetic.  Where fewer than 32 residues leave lanes of one read a multiple of M apart and M is even, the window is
// stored at q + (q >> 5) (PAD) so that strides of 2, 4, ... 32 samples fall into different banks: L = 1 (decimation by an even factor).
// PT, JT and R are chosen on the host from (L, M, T) alone (rs_plan): PT = L up to 64 residues, else 32, halved while the rows do not
// fit; JT as many periods as R = 8 allows, fewer where the window would not fit in LDS.
//
// Order.  Every output is ONE fp32 chain in ascending tap order, starting from +0:
//     y[m] = fmaf(table[p][T-1], x[q + T/2], ... fmaf(table[p][1], x[q - T/2 + 2], fmaf(table[p][0], x[q - T/2 + 1], +0)) ...)
// with x[n] = +0 outside the signal (for finite inputs such a term changes nothing), contraction off.  The chain is a function of
// (x_b, table, L, M, T, m) alone: not of the run, B, the row's place in the batch, Nout or the tiling; no atomics, no workspace, one
// store per output.  On integer data whose partial sums stay below 2^24 the result is exact.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "kernels.h"
#include "resample_table.h"

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_RMAX = 8;                              // periods (accumulators) per thread
constexpr int RS_XR = 8;                                // window samples a lane loads before it writes them to LDS
constexpr int RS_ROWS_MAX = 20480;                      // floats of LDS the staged table rows may take
constexpr int RS_SMALL = 16000;                         // floats: a tile within 64 KB, where three workgroups share a CU
constexpr int RS_LARGE = 40000;                         // floats: the most a tile takes (160 000 of the 163 840 bytes)

struct RsPlan {
    int PT, JT, R, pad, S;
    int wmax;                                           // window samples staged at most (unpadded)
    size_t smem;
};

__host__ __device__ constexpr int rs_stride(int T) { return 4 * ((((T + 3) >> 2)) | 1); }
__host__ __device__ constexpr int rs_xidx(int q, bool pad) { return pad ? q + (q >> 5) : q; }

// The tile of a geometry: a function of (L, M, T) alone.  The bound on the span of o() over PT consecutive residues:
// floor((r + PT - 1) M / L) - floor(r M / L) <= floor((PT - 1) M / L) + 1.
RsPlan rs_plan(int L, int M, int T) {
    RsPlan pl;
    pl.S = rs_stride(T);
    pl.PT = L <= 64 ? L : 32;
    while (pl.PT > 1 && pl.PT * pl.S > RS_ROWS_MAX) pl.PT >>= 1;
    const int G = RS_THREADS / pl.PT;
    pl.pad = pl.PT < 32 && !(M & 1);
    const int span = (int)(((long long)(pl.PT - 1) * M) / L) + 1;
    auto periods = [&](int budget) {                    // the most periods whose window fits budget floats beside the rows
        long long room = budget - pl.PT * pl.S;
        if (pl.pad) room = room * 32 / 33 - 1;
        room -= span + T;
        return room < 0 ? 0LL : room / M + 1;
    };
    long long jt = periods(RS_SMALL);
    if (jt < (long long)G * RS_RMAX / 2) jt = periods(RS_LARGE);     // fewer than 4 periods per thread: take the larger tile
    if (jt > (long long)G * RS_RMAX) jt = (long long)G * RS_RMAX;
    if (jt < 1) jt = 1;                                  // rows <= 20480, span + T <= 2049 + 8192: one period always fits RS_LARGE
    pl.JT = (int)jt;
    pl.R = pl.JT > 4 * G ? 8 : pl.JT > 2 * G ? 4 : pl.JT > G ? 2 : 1;
    pl.wmax = (pl.JT - 1) * M + span + T;
    pl.smem = (size_t)(pl.PT * pl.S + rs_xidx(pl.wmax, pl.pad)) * sizeof(float);
    return pl;
}

#pragma clang fp contract(off)
template <int R, bool PAD>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const float* __restrict__ x, const float* __restrict__ table,
                                                              float* __restrict__ out, long long N, int L, int M, int T,
                                                              long long Nout, int PT, int JT, int nrt, long long njt) {
    extern __shared__ __attribute__((aligned(16))) float rs_smem[];
    const int S = rs_stride(T);
    float* ts = rs_smem;                                // [PT][S]
    float* xs = rs_smem + PT * S;                       // the window
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // blockIdx.x = (b njt + jt) nrt + rt: the residue tiles of one run of periods, which read the same window, are neighbours
    const long long bj = blockIdx.x / nrt;
    const int rt = (int)(blockIdx.x - bj * nrt);
    const long long b = bj / njt;
    const long long j0 = (bj - b * njt) * JT;
    const int r0 = rt * PT;
    const int rows = L - r0 < PT ? L - r0 : PT;
    const int o0 = (int)(((long long)r0 * M) / L);
    const int span = (int)(((long long)(r0 + rows - 1) * M) / L) - o0;
    // the periods of this tile that hold an output: m = j L + r0 < Nout
    const long long jleft = (Nout - r0 + L - 1) / L - j0;
    if (jleft < 1) return;                                           // the last run of periods may end before this tile's residues
    const int jt = jleft < JT ? (int)jleft : JT;
    const int wlen = (jt - 1) * M + span + T;
    const long long wb = j0 * M + o0 - T / 2 + 1;                    // window sample q is x[wb + q]
    const float* __restrict__ xb = x + b * N;

    for (int qb = tid; qb < wlen; qb += RS_XR * RS_THREADS) {        // RS_XR loads in flight per lane, then their LDS writes
        float v[RS_XR];
#pragma unroll
        for (int e = 0; e < RS_XR; ++e) {
            const int q = qb + RS_THREADS * e;
            const long long n = wb + q;
            v[e] = (q < wlen && n >= 0 && n < N) ? xb[n] : 0.f;
        }
#pragma unroll
        for (int e = 0; e < RS_XR; ++e) {
            const int q = qb + RS_THREADS * e;
            if (q < wlen) xs[rs_xidx(q, PAD)] = v[e];
        }
    }
    for (int rl = wave; rl < rows; rl += RS_THREADS / 64) {          // a wave per table row: coalesced
        const float* __restrict__ tr = table + (size_t)(((long long)(r0 + rl) * M) % L) * T;
        for (int i = lane; i < T; i += 64) ts[rl * S + i] = tr[i];
    }
    __syncthreads();

    const int G = RS_THREADS / PT;
    const int rl = tid % PT, g = tid / PT;
    if (rl >= rows || g >= G) return;
    const int r = r0 + rl;
    const int o = (int)(((long long)r * M) / L) - o0;
    int qk[R];
    bool ok[R];
    float acc[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        const int jl = g + k * G;
        ok[k] = jl < jt && (j0 + jl) * L + r < Nout;
        qk[k] = ok[k] ? jl * M + o : 0;                  // a period without an output reads the head of the window and stores nothing
        acc[k] = 0.f;
    }
    const float* tr = ts + rl * S;
    const int T4 = T & ~3;
    for (int i = 0; i < T4; i += 4) {
        const float4 h = *reinterpret_cast<const float4*>(tr + i);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            acc[k] = fmaf(h.x, xs[rs_xidx(qk[k] + i, PAD)], acc[k]);
            acc[k] = fmaf(h.y, xs[rs_xidx(qk[k] + i + 1, PAD)], acc[k]);
            acc[k] = fmaf(h.z, xs[rs_xidx(qk[k] + i + 2, PAD)], acc[k]);
            acc[k] = fmaf(h.w, xs[rs_xidx(qk[k] + i + 3, PAD)], acc[k]);
        }
    }
    if (T & 2) {                                         // T is even: the last two taps
        const float2 h = *reinterpret_cast<const float2*>(tr + T4);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            acc[k] = fmaf(h.x, xs[rs_xidx(qk[k] + T4, PAD)], acc[k]);
            acc[k] = fmaf(h.y, xs[rs_xidx(qk[k] + T4 + 1, PAD)], acc[k]);
        }
    }
    float* __restrict__ y = out + b * Nout;
#pragma unroll
    for (int k = 0; k < R; ++k)
        if (ok[k]) y[(j0 + g + k * G) * L + r] = acc[k];
}

template <int R, bool PAD>
int rs_launch(const RsPlan& pl, unsigned grid, hipStream_t stream, const float* x, const float* table, float* out, long long N, int L,
              int M, int T, long long Nout, int nrt, long long njt) {
    if (pl.smem > (64 << 10)) {
        // Dynamic LDS above 64 KB has to be asked for, per device and kernel: asked once, for the most any tile takes, and remembered
        // in an append-only flag per device (a race sets it twice: harmless).  A property of the function, not a stream operation.
        static std::atomic<bool> asked[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return UNETRIR_EINVAL;
        if (!asked[dev].load(std::memory_order_acquire)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&resample_kernel<R, PAD>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, RS_LARGE * (int)sizeof(float));
            if (e != hipSuccess) return (int)e;
            asked[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((resample_kernel<R, PAD>), dim3(grid), dim3(RS_THREADS), pl.smem, stream, x, table, out, N, L, M, T, Nout, pl.PT,
                       pl.JT, nrt, njt);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int unetrir_resample_supported(int L, int M, int zeros) { return resample_table::taps(L, M, zeros) ? 1 : 0; }

int unetrir_resample_taps(int L, int M, int zeros) { return resample_table::taps(L, M, zeros); }

long long unetrir_resample_out_length(long long N, int L, int M) { return resample_table::out_length(N, L, M); }

int unetrir_resample_table_f32(float* table, int L, int M, int zeros, double rolloff, double beta) {
    return resample_table::build(table, L, M, zeros, rolloff, beta) ? 0 : UNETRIR_EINVAL;
}

int unetrir_resample_f32(const float* x, const float* table, float* out, int B, long long N, int L, int M, int T, long long Nout,
                         unetrir_stream_t stream) {
    if (!x || !table || !out || B < 1 || N < 1 || Nout < 1 || !resample_table::geometry_ok(L, M, T)) return UNETRIR_EINVAL;
    // every index stays within 63 bits: N (L + M) bounds m M and q, B (N + Nout) the elements addressed
    if (N > (1LL << 49)) return UNETRIR_EINVAL;
    const long long full = resample_table::out_length(N, L, M);
    if (!full || Nout > full || (Nout > N ? Nout : N) > (1LL << 60) / B) return UNETRIR_EINVAL;
    const RsPlan pl = rs_plan(L, M, T);
    const int nrt = (L + pl.PT - 1) / pl.PT;
    const long long periods = (Nout + L - 1) / L;
    const long long njt = (periods + pl.JT - 1) / pl.JT;
    // the last run of periods may hold outputs of the first residues only: its other residue tiles are launched and return at once
    if (njt > 0x7fffffffLL / nrt || njt * nrt > 0x7fffffffLL / B) return UNETRIR_EINVAL;
    const unsigned grid = (unsigned)(njt * nrt * B);
    hipStream_t s = (hipStream_t)stream;
#define RS_CASE(R_, PAD_) \
    if (pl.R == R_ && pl.pad == PAD_) return rs_launch<R_, PAD_>(pl, grid, s, x, table, out, N, L, M, T, Nout, nrt, njt);
    RS_CASE(8, false) RS_CASE(4, false) RS_CASE(2, false) RS_CASE(1, false)
    RS_CASE(8, true) RS_CASE(4, true) RS_CASE(2, true) RS_CASE(1, true)
#undef RS_CASE
    return UNETRIR_EINVAL;
}

}  // extern "C"
