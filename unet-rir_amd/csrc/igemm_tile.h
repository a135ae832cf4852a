// igemm_tile.h - what the three tap-table implicit-GEMM forward kernels share (igemm.hip fp32, igemm_bf16.hip, igemm2_bf16.hip):
// the XCD remap, the per-row prologue, the register-stage loader, the staged bf16 epilogue with column statistics and the host
// ladder that picks an instantiation.  The K loops are NOT here: one chunk in flight in one LDS buffer (igemm.hip,
// igemm_bf16.hip) against two chunks in two buffers (igemm2_bf16.hip).  Internal to csrc/.
#pragma once
#include "kernels.h"
#include "mfma_types.h"

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    // Blocks are dealt round-robin over the 8 XCDs; give each XCD a contiguous run of tiles so
    // neighbouring pixel tiles (shared halo rows, shared weight panel) meet in one L2.
    const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
    const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return base + (bid >> 3);
}

// Pixel arithmetic of a launch.  PIX = long long: the general kernels (any M).  PIX = unsigned: igemm2, whose launcher checks
// M < 2^31 - the 64-bit divisions of the general form cost ~1 us of a 10 us launch.
template <typename PIX> struct PixIdx;
template <> struct PixIdx<long long> { typedef int idx; typedef long long wide; };
template <> struct PixIdx<unsigned> { typedef unsigned idx; typedef size_t wide; };

// The row prologue and the stage loader are macros: as __forceinline__ templates the same statements reached the scheduler in
// another order and every tap-table kernel came out with a different instruction stream (one with another register count).  They
// paste into the kernel body and use its names: a (arguments: .g, .in, .w), s_tap, m0, M, plane, n0, lrow, quad, kt, kc and
// the copies C, ntaps, IH, IW, ldi, ldw of the geometry.  T = float | __bf16.

// IGEMM_ROW_PROLOGUE declares, per staged row of a loader thread (32 rows per pass: NA passes of pixels, NB of weight rows):
// a_ptr / a_mask, the pointer to the row's centre pixel (tap offset 0) and the bit mask of the taps that fall inside the image;
// b_ptr / b_ok, the weight row.
#define IGEMM_ROW_PROLOGUE(T, NA, NB, PIX)                                                                              \
    const T* a_ptr[NA];                                                                                                 \
    unsigned long long a_mask[NA];                                                                                      \
    _Pragma("unroll") for (int j = 0; j < NA; ++j) {                                                                    \
        typedef PixIdx<PIX>::idx I_;                                                                                    \
        const PIX p = m0 + lrow + 32 * j;                                                                               \
        a_ptr[j] = a.in;                                                                                                \
        a_mask[j] = 0ull;                                                                                               \
        if (p < M) {                                                                                                    \
            const I_ n = (I_)(p / plane);                                                                               \
            const I_ rem = (I_)(p - (PIX)n * plane);                                                                    \
            const I_ py = rem / (I_)a.g.PW, px = rem - py * (I_)a.g.PW;                                                 \
            const int by = (int)py * a.g.SI, bx = (int)px * a.g.SI;                                                     \
            a_ptr[j] = a.in + ((PixIdx<PIX>::wide)((PIX)n * (I_)IH + (I_)by) * IW + bx) * ldi;                          \
            unsigned long long m = 0ull;                                                                                \
            for (int t = 0; t < ntaps; ++t) {                                                                           \
                const uint32_t e = s_tap[t];                                                                            \
                const int iy = by + (int)(int8_t)(e & 0xff), ix = bx + (int)(int8_t)((e >> 8) & 0xff);                  \
                if ((unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW) m |= 1ull << t;                         \
            }                                                                                                           \
            a_mask[j] = m;                                                                                              \
        }                                                                                                               \
    }                                                                                                                   \
    const T* b_ptr[NB];                                                                                                 \
    bool b_ok[NB];                                                                                                      \
    _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                                                    \
        const int n = n0 + lrow + 32 * j;                                                                               \
        b_ok[j] = n < a.g.N;                                                                                            \
        b_ptr[j] = a.w + (size_t)(b_ok[j] ? n : 0) * ldw;                                                               \
    }

// IGEMM_LOAD_STAGE: one K chunk (Elem<T>::KE values of every row) from global memory into the registers RA[NA] / RB[NB], by
// masked 16-byte loads at (tap kt, channel kc).  UNIFORM (C % KE == 0): a chunk never straddles a tap, so the tap and the
// channel base are wave-uniform scalars and only quad * EPS is per lane.  Advancing kt / kc - and a split-K start - is the
// caller's business.
#define IGEMM_LOAD_STAGE(T, NA, NB, RA, RB)                                                                             \
    {                                                                                                                   \
        typedef Elem<T>::Vec V_;                                                                                        \
        int t = kt, c = kc;                                                                                             \
        if (UNIFORM) { t = __builtin_amdgcn_readfirstlane(t); c = __builtin_amdgcn_readfirstlane(c); }                  \
        const bool kok = t < ntaps;                                                                                     \
        uint32_t e = kok ? s_tap[t] : 0u;                                                                               \
        if (UNIFORM) e = __builtin_amdgcn_readfirstlane(e);                                                             \
        const int dy = (int)(int8_t)(e & 0xff), dx = (int)(int8_t)((e >> 8) & 0xff);                                    \
        const int wi = (int)((e >> 16) & 0xff);                                                                         \
        const int aoff = (dy * IW + dx) * ldi + c + (UNIFORM ? quad * Elem<T>::EPS : 0);                                \
        const int boff = wi * C + c + (UNIFORM ? quad * Elem<T>::EPS : 0);                                              \
        _Pragma("unroll") for (int j = 0; j < NA; ++j) {                                                                \
            V_ v = Elem<T>::zero();                                                                                     \
            if (kok && ((a_mask[j] >> t) & 1ull)) v = *reinterpret_cast<const V_*>(a_ptr[j] + aoff);                    \
            RA[j] = v;                                                                                                  \
        }                                                                                                               \
        _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                                                \
            V_ v = Elem<T>::zero();                                                                                     \
            if (kok && b_ok[j]) v = *reinterpret_cast<const V_*>(b_ptr[j] + boff);                                      \
            RB[j] = v;                                                                                                  \
        }                                                                                                               \
    }

// ---- IGEMM_BF16_EPILOGUE: the bf16 epilogue through LDS, for 4 waves as 2 (pixels) x 2 (channels), each WM pixels x BN_/2
// channels.  A macro for the same reason; it uses a (IgemmArgsH), smem_h (the K loop's LDS, free again: every wave has passed a
// barrier after its last fragment read), acc, tid, lane, wave, wm, wn, m0, M, plane, mt, n0.
// The weight fragment is the MFMA A operand, so acc[i][j] holds D[n = 32j + (r&3) + 8(r>>2) + 4h][pixel = 32i + (lane&31)]: a
// lane owns 4 consecutive channels per register quad.
//  (1) + bias, pack 4 channels -> ds_write_b64 into this wave's [WM px][BN_/2 ch] staging tile (row stride SROW: 16-byte pad);
//  (2) read back 16-byte channel runs of one pixel (LPP lanes per pixel, PPP pixels per pass), add the optional addend, store
//      16 B per lane (2-byte stores straight from the MFMA layout cost a third of the kernel).  A pixel the output map drops is
//      not stored and not part of the column statistics either: its staging row is zeroed.  With an addend the sums go back
//      into the staging tile: the statistics are those of what is stored.  The ragged channel tail (N not a multiple of 8)
//      never happens for activations; kept for safety;
//  (3) fused column statistics (BatchNormalization batch statistics without re-reading the tensor), after a barrier because
//      of (2)'s write-backs: per-channel (sum, sum of squares) of the bf16 values this pixel tile stores, one colstat row per
//      pixel tile, in a fixed order: each wave sums the WM pixel rows of its staging tile (BN_ = 64: two lanes per channel,
//      half the rows each, combined by one cross-lane add), the two waves that share a channel range are added through LDS.
#define IGEMM_BF16_EPILOGUE(WM, BN_, PIX)                                                                                                             \
    {                                                                                                                                                 \
        typedef PixIdx<PIX>::idx I_;                                                                                                                  \
        constexpr int WN = BN_ / 2;                                                                                                                   \
        constexpr int SROW = WN + 8;                                                                                                                  \
        __bf16* stage = smem_h + wave * (WM * SROW);                                                                                                  \
        const int hq = lane >> 5, l31 = lane & 31;                                                                                                    \
        _Pragma("unroll") for (int j = 0; j < BN_ / 64; ++j) {                                                                                        \
            _Pragma("unroll") for (int qd = 0; qd < 4; ++qd) {                                                                                        \
                const int nl = 32 * j + 8 * qd + 4 * hq;                                                                                              \
                const int n = n0 + wn * WN + nl;                                                                                                      \
                float bv[4] = {0.f, 0.f, 0.f, 0.f};                                                                                                   \
                if (a.bias) {                                                                                                                         \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) if (n + e < a.g.N) bv[e] = a.bias[n + e];                                           \
                }                                                                                                                                     \
                _Pragma("unroll") for (int i = 0; i < WM / 32; ++i) {                                                                                 \
                    bf16x4 o;                                                                                                                         \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) o[e] = (__bf16)(acc[i][j][4 * qd + e] + bv[e]);                                     \
                    *reinterpret_cast<bf16x4*>(stage + (32 * i + l31) * SROW + nl) = o;                                                               \
                }                                                                                                                                     \
            }                                                                                                                                         \
        }                                                                                                                                             \
        __syncthreads();                                                                                                                              \
        const bool simple = (a.g.SO == 1 && a.g.ooy == 0 && a.g.oox == 0 && a.g.OH == a.g.PH && a.g.OW == a.g.PW);                                    \
        constexpr int LPP = WN / 8;                                                                                                                   \
        constexpr int PPP = 64 / LPP;                                                                                                                 \
        const int cq = lane % LPP, pl = lane / LPP;                                                                                                   \
        const int n = n0 + wn * WN + cq * 8;                                                                                                          \
        _Pragma("unroll") for (int ps = 0; ps < WM / PPP; ++ps) {                                                                                     \
            const int prow = ps * PPP + pl;                                                                                                           \
            const PIX p = m0 + wm * WM + prow;                                                                                                        \
            if (p >= M || n >= a.g.N) continue;                                                                                                       \
            PixIdx<PIX>::wide opix;                                                                                                                   \
            if (simple) {                                                                                                                             \
                opix = p;                                                                                                                             \
            } else {                                                                                                                                  \
                const I_ nimg = (I_)(p / plane);                                                                                                      \
                const I_ rem = (I_)(p - (PIX)nimg * plane);                                                                                           \
                const I_ py = rem / (I_)a.g.PW, px = rem - py * (I_)a.g.PW;                                                                           \
                const int oy = (int)py * a.g.SO + a.g.ooy, ox = (int)px * a.g.SO + a.g.oox;                                                           \
                if (oy >= a.g.OH || ox >= a.g.OW) {                                                                                                   \
                    if (a.colstat != nullptr) *reinterpret_cast<uint4*>(stage + prow * SROW + cq * 8) = make_uint4(0u, 0u, 0u, 0u);                   \
                    continue;                                                                                                                         \
                }                                                                                                                                     \
                opix = ((PixIdx<PIX>::wide)nimg * a.g.OH + oy) * a.g.OW + ox;                                                                         \
            }                                                                                                                                         \
            bf16x8 v = *reinterpret_cast<const bf16x8*>(stage + prow * SROW + cq * 8);                                                                \
            if (n + 7 < a.g.N) {                                                                                                                      \
                if (a.addend != nullptr) {                                                                                                            \
                    const bf16x8 ad = *reinterpret_cast<const bf16x8*>(a.addend + opix * a.ldadd + n);                                                \
                    _Pragma("unroll") for (int e = 0; e < 8; ++e) v[e] = (__bf16)((float)v[e] + (float)ad[e]);                                        \
                    if (a.colstat != nullptr) *reinterpret_cast<bf16x8*>(stage + prow * SROW + cq * 8) = v;                                           \
                }                                                                                                                                     \
                *reinterpret_cast<bf16x8*>(a.out + opix * a.g.ldo + n) = v;                                                                           \
            } else {                                                                                                                                  \
                for (int e = 0; e < 8 && n + e < a.g.N; ++e) {                                                                                        \
                    float f = (float)v[e];                                                                                                            \
                    if (a.addend != nullptr) f += (float)a.addend[opix * a.ldadd + n + e];                                                            \
                    a.out[opix * a.g.ldo + n + e] = (__bf16)f;                                                                                        \
                }                                                                                                                                     \
            }                                                                                                                                         \
        }                                                                                                                                             \
        if (a.colstat != nullptr) {                                                                                                                   \
            __syncthreads();                                                                                                                          \
            __shared__ float s_cs[4][64][2];                                                                                                          \
            constexpr int LPC = 64 / WN, RPL = WM / LPC;                                                                                              \
            const int ch = lane % WN, half = lane / WN;                                                                                               \
            float cs = 0.f, css = 0.f;                                                                                                                \
            _Pragma("unroll 8") for (int r = 0; r < RPL; ++r) {                                                                                       \
                const int prow = half * RPL + r;                                                                                                      \
                if (m0 + wm * WM + prow < M) { const float v = (float)stage[prow * SROW + ch]; cs += v; css += v * v; }                               \
            }                                                                                                                                         \
            if (LPC == 2) { cs += __shfl_xor(cs, 32); css += __shfl_xor(css, 32); }                                                                   \
            if (lane < WN) { s_cs[wave][ch][0] = cs; s_cs[wave][ch][1] = css; }                                                                       \
            __syncthreads();                                                                                                                          \
            if (tid < BN_) {                                                                                                                          \
                const int wn_ = tid / WN, c = tid % WN, nn = n0 + wn_ * WN + c;                                                                       \
                if (nn < a.g.N) {                                                                                                                     \
                    float* row = a.colstat + ((size_t)mt * a.g.N + nn) * 2;                                                                           \
                    row[0] = s_cs[wn_][c][0] + s_cs[2 + wn_][c][0];                                                                                   \
                    row[1] = s_cs[wn_][c][1] + s_cs[2 + wn_][c][1];                                                                                   \
                }                                                                                                                                     \
            }                                                                                                                                         \
        }                                                                                                                                             \
    }

// ---- host: the uniform x channel tile x (1 | 4 classes) ladder of one bf16 kernel family.  K names the kernels:
// K::k1<BN_, UNIFORM> takes IgemmArgsH, K::k4<BN_, UNIFORM> takes IgemmArgsH4 (blockIdx.y = parity class of a stride-2
// transposed layer: four launches of the same shape in one grid).  nwg: workgroups per class.
struct IgemmArgsH4 { IgemmArgsH a[4]; };
template <typename K>
int launch_tap_table_bf16(const IgemmArgsH* a, int ncls, bool bn128, unsigned nwg, hipStream_t s) {
    const bool uniform = (a[0].g.C % Elem<__bf16>::KE) == 0;
    if (ncls == 4) {
        IgemmArgsH4 a4;
        for (int i = 0; i < 4; ++i) a4.a[i] = a[i];
        const auto k = bn128 ? (uniform ? K::template k4<128, true> : K::template k4<128, false>)
                             : (uniform ? K::template k4<64, true> : K::template k4<64, false>);
        hipLaunchKernelGGL(k, dim3(nwg, 4), dim3(256), 0, s, a4);
    } else {
        const auto k = bn128 ? (uniform ? K::template k1<128, true> : K::template k1<128, false>)
                             : (uniform ? K::template k1<64, true> : K::template k1<64, false>);
        hipLaunchKernelGGL(k, dim3(nwg), dim3(256), 0, s, a[0]);
    }
    return (int)hipGetLastError();
}
