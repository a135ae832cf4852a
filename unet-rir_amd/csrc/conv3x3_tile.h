// conv3x3_tile.h - what the 3x3 stride-1 tile kernels have in common.  conv3x3g.hip (one workgroup per tile) and conv3x3p.hip
// (persistent): the DMA source tables and one K step of the v_mfma_f32_16x16x32_bf16 body; conv3x3g.hip's header describes the
// pipeline around them.  conv3x3g.hip, conv3x3r.hip and conv3x3h.hip: the staged epilogue.  Internal to csrc/; device-only.
#pragma once
#include "kernels.h"
#include "lds_dma.h"

// LDS images.  A patch is rows of PC pixels x 64 B (32 input channels), a kernel tile [3 vertical taps][BN channels] rows of
// 64 B; both are written by wave-instructions of 16 rows x 64 B, lane = (row sub = lane >> 2, 16-byte slot = lane & 3).  The
// four granules of a row are XOR-swizzled with bit 2 of the row's position (patch: pixel column, kernel: channel) on the DMA
// SOURCE address, and again on the fragment read, so that the 16 rows of a ds_read_b128 meet 16 different bank groups.

// The two source tables are macros (SUB = lane >> 2, SLOT = lane & 3; the kernel's also uses the caller's n0, C, ldw = 9 C and
// Conv3Args a): through inlined functions the same arithmetic is simplified in another order and the kernels come out with
// other code in front of the loop.

// source granule of LDS slot SLOT in the row at position POS (patch: pixel column, kernel: channel)
#define DMA_GRANULE(SLOT, POS) ((SLOT) ^ (((POS) & 4) >> 1))

// patch pixel P = (row PR, column PCOL) of a PC_-column patch that wave-instruction I stages in this lane
#define PATCH_LANE(I, SUB, PC_, P, PR, PCOL) const int P = 16 * (I) + (SUB); const int PR = P / (PC_), PCOL = P - PR * (PC_)

// WP = byte offset into the [N][9][C] kernel of what wave-instruction I of a kernel tile stages in lane (SUB, SLOT), for chunk 0 and
// dx 0: LDS row dy * BN_ + nl (BN_ = 128 or 64) holds output channel n0 + CH_OF (an expression in nl); channels past N read
// zeros.  a.flip & 1: the data gradient's flipped taps.
#define KERNEL_LANE(WP, I, SUB, SLOT, BN_, CH_OF) do {                                \
    const int row = 16 * (I) + (SUB);                                                 \
    const int dy = row >> ((BN_) == 128 ? 7 : 6), nl = row & ((BN_) - 1);             \
    const int gs = DMA_GRANULE(SLOT, nl);                                             \
    const int n = n0 + (CH_OF);                                                       \
    const int tap0 = (a.flip & 1) ? 8 - 3 * dy : 3 * dy;                              \
    WP = n < a.N ? (uint32_t)((n * ldw + tap0 * C + gs * 8) * 2) : OOB;               \
} while (0)

// One K step (32 input channels, one horizontal tap dx) of a wave: RPW_ tile rows x 32 pixels x 64 channels into
// f32x4 ACC[RPW_][2][4] ([tile row][16-pixel half][16-channel tile]).  BA: the wave's kernel fragment address in the ring slot
// of dx (row l15 of its 64 channels, granule lq swizzled), WROW_ bytes (BN * 64) between vertical taps; AA: its patch fragment
// address (patch row RPW_ * wm, column l15 + dx), RP_ bytes between patch rows, HO_ to the second 16-pixel half.  Patch row r
// feeds tile row r - dy with vertical tap dy: a patch fragment pair is read once for its three taps and a kernel fragment once
// for every tile row.  The reads return in issue order, so each MFMA group starts behind a counted wait as soon as its own
// fragments are in.  Ends at s_setprio(0); the caller pins the schedule with sched_barrier(0).
// (A macro, not a function: through an inlined function the same statements come out in another register assignment and
//  another order around the loop.)
#define K3_RDW(dy, BA, WROW_) DSR128(wf[dy][0], BA, dy * (WROW_) + 0); DSR128(wf[dy][1], BA, dy * (WROW_) + 1024); \
                              DSR128(wf[dy][2], BA, dy * (WROW_) + 2048); DSR128(wf[dy][3], BA, dy * (WROW_) + 3072)
#define K3_RDP(r, AA, RP_, HO_) DSR128(pf[r][0], AA, r * (RP_) + 0); DSR128(pf[r][1], AA, r * (RP_) + (HO_))
#define K3_ROWS(r, ACC, RPW_)                                                                  \
    _Pragma("unroll") for (int dy = 0; dy < 3; ++dy) {                                         \
        if (r - dy < 0 || r - dy > (RPW_) - 1) continue;                                       \
        _Pragma("unroll") for (int h = 0; h < 2; ++h)                                          \
            _Pragma("unroll") for (int t = 0; t < 4; ++t) MMA16(ACC[r - dy][h][t], wf[dy][t], pf[r][h]); \
    }
#define CONV3X3_KSTEP(ACC, BA, AA, RPW_, WROW_, RP_, HO_) do {                                                                   \
    u32x4 wf[3][4], pf[6][2];                                                                                                    \
    if constexpr ((RPW_) == 4) {                                                                                                 \
        K3_RDW(0, BA, WROW_); K3_RDP(0, AA, RP_, HO_); K3_RDW(1, BA, WROW_); K3_RDP(1, AA, RP_, HO_);                            \
        K3_RDW(2, BA, WROW_); K3_RDP(2, AA, RP_, HO_);                       /* 18 reads in flight */                            \
        __builtin_amdgcn_s_setprio(1);                                                                                           \
        LGKM_WAIT(12); K3_ROWS(0, ACC, RPW_);                                                                                    \
        K3_RDP(3, AA, RP_, HO_);                                                                                                 \
        LGKM_WAIT(8); K3_ROWS(1, ACC, RPW_);                                                                                     \
        K3_RDP(4, AA, RP_, HO_);                                                                                                 \
        LGKM_WAIT(4); K3_ROWS(2, ACC, RPW_);                                                                                     \
        K3_RDP(5, AA, RP_, HO_);                                                                                                 \
        LGKM_WAIT(4); K3_ROWS(3, ACC, RPW_);                                                                                     \
        LGKM_WAIT(2); K3_ROWS(4, ACC, RPW_);                                                                                     \
        LGKM_WAIT(0); K3_ROWS(5, ACC, RPW_);                                                                                     \
    } else {                                                                 /* two tile rows: patch rows 0..3 */                \
        K3_RDW(0, BA, WROW_); K3_RDP(0, AA, RP_, HO_); K3_RDW(1, BA, WROW_); K3_RDP(1, AA, RP_, HO_);                            \
        K3_RDW(2, BA, WROW_); K3_RDP(2, AA, RP_, HO_); K3_RDP(3, AA, RP_, HO_);   /* 20 reads in flight */                       \
        __builtin_amdgcn_s_setprio(1);                                                                                           \
        LGKM_WAIT(14); K3_ROWS(0, ACC, RPW_);                                                                                    \
        LGKM_WAIT(8); K3_ROWS(1, ACC, RPW_);                                                                                     \
        LGKM_WAIT(2); K3_ROWS(2, ACC, RPW_);                                                                                     \
        LGKM_WAIT(0); K3_ROWS(3, ACC, RPW_);                                                                                     \
    }                                                                                                                            \
    __builtin_amdgcn_s_setprio(0);                                                                                               \
} while (0)

// ---- The staged epilogue of the kernels that write through a per-wave LDS tile (conv3x3g, conv3x3r, conv3x3h).  The MFMA
// result has 4 consecutive channels of one pixel per lane; a wave puts (accumulator + bias) as bf16 into its private tile
// [pixel][64 channels + pad], then reads it back with 8 lanes per pixel - 16 bytes = 8 channels each - adds the addend,
// gathers the fused column statistics of what it stores, and stores 16 bytes per lane.  WAVE_LDS_FENCE() between the phases.
// Macros for the reason given above; they use the caller's Conv3Args a, `out`, `addend`, cs_s[8] / cs_q[8], tid and lane.

// float4 BV = bias of channels N_ .. N_ + 3 (zeros without a bias and past a.N)
#define STAGE_BIAS4(BV, N_)                                                                                              \
    float4 BV = make_float4(0.f, 0.f, 0.f, 0.f);                                                                         \
    if (a.bias && (N_) + 3 < a.N) BV = *reinterpret_cast<const float4*>(a.bias + (N_));                                  \
    else if (a.bias) { float* bp = &BV.x; for (int e = 0; e < 4; ++e) if ((N_) + e < a.N) bp[e] = a.bias[(N_) + e]; }

// four accumulators + bias -> 8 bytes of the staging tile at DST
#define STAGE4(DST, C0, C1, C2, C3, BV) do {                                         \
    bf16x4 o;                                                                        \
    o[0] = (__bf16)((C0) + BV.x); o[1] = (__bf16)((C1) + BV.y);                      \
    o[2] = (__bf16)((C2) + BV.z); o[3] = (__bf16)((C3) + BV.w);                      \
    *reinterpret_cast<bf16x4*>(DST) = o;                                             \
} while (0)

// 16 bytes of the staging tile at SRC -> channels NQ .. NQ + 7 of pixel PIX (size_t): + addend, rounded to bf16 as it is stored;
// into this lane's column statistics when the launch asks for them; out
#define DRAIN8(SRC, PIX, NQ) do {                                                                                        \
    uint4 v = *reinterpret_cast<const uint4*>(SRC);                                                                      \
    const size_t pix = (PIX);                                                                                            \
    if (addend) {                                                                                                        \
        const bf16x8 ad = *reinterpret_cast<const bf16x8*>(addend + pix * a.ldadd + (NQ));                               \
        bf16x8 vv = __builtin_bit_cast(bf16x8, v);                                                                       \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) vv[e] = (__bf16)((float)vv[e] + (float)ad[e]);                     \
        v = __builtin_bit_cast(uint4, vv);                                                                               \
    }                                                                                                                    \
    if (a.colstat) {                                                                                                     \
        const bf16x8 sv = __builtin_bit_cast(bf16x8, v);                                                                 \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) { const float f = (float)sv[e]; cs_s[e] += f; cs_q[e] += f * f; }  \
    }                                                                                                                    \
    *reinterpret_cast<uint4*>(out + pix * a.ldo + (NQ)) = v;                                                             \
} while (0)

// Column statistics of a tile -> row ROW (a size_t expression, evaluated by the writing threads only) of a.colstat.  Lanes
// pl = 0 .. 7 of a wave hold the same 8 channels (from WN_ * 64 + 8 * (lane & 7) of the tile's BN_): fold them, leave the sums of
// row group WM_ in RED ([G_ row groups][BN_ channels][2] floats of LDS that nobody else uses any more), then 2 BN_ threads add
// the G_ = 4 or 8 row groups in a FIXED order - the same bits whoever ran first.  N0_: first channel of the tile.
#define COLSTAT_FOLD(G_, BN_, RED, WM_, WN_, ROW, N0_) do {                                                              \
    _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                      \
        _Pragma("unroll") for (int off = 8; off < 64; off <<= 1) { cs_s[e] += __shfl_xor(cs_s[e], off); cs_q[e] += __shfl_xor(cs_q[e], off); } \
    }                                                                                                                    \
    float* red = reinterpret_cast<float*>(RED);                                                                          \
    if (lane < 8) {                                                                                                      \
        _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                                                  \
            red[(((WM_) * (BN_)) + (WN_) * 64 + lane * 8 + e) * 2 + 0] = cs_s[e];                                        \
            red[(((WM_) * (BN_)) + (WN_) * 64 + lane * 8 + e) * 2 + 1] = cs_q[e];                                        \
        }                                                                                                                \
    }                                                                                                                    \
    __syncthreads();                                                                                                     \
    if (tid < 2 * (BN_)) {                                                                                               \
        const int ch = tid >> 1, st = tid & 1;                                                                           \
        float t = ((red[(0 * (BN_) + ch) * 2 + st] + red[(1 * (BN_) + ch) * 2 + st]) + red[(2 * (BN_) + ch) * 2 + st]) + \
                  red[(3 * (BN_) + ch) * 2 + st];                                                                        \
        if constexpr ((G_) == 8)                                                                                         \
            t = (((t + red[(4 * (BN_) + ch) * 2 + st]) + red[(5 * (BN_) + ch) * 2 + st]) + red[(6 * (BN_) + ch) * 2 + st]) + \
                red[(7 * (BN_) + ch) * 2 + st];                                                                          \
        const size_t row = (ROW);                                                                                        \
        if ((N0_) + ch < a.N) a.colstat[(row * a.N + (N0_) + ch) * 2 + st] = t;                                          \
    }                                                                                                                    \
} while (0)
