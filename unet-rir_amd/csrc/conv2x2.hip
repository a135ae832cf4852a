// conv2x2.hip - the 2x2 stride-2 layers of AENet (dl_models/ae_net.py:273-279 Conv2D(k=2, strides=2, 'same'), :301-307
// Conv2DTranspose(k=2, strides=2, 'same'); gfx950, bf16).
//
// On even sizes the four windows of a 2 x 2 cell do not overlap: no halo, no padding, no crop.  Each of the three passes is a
// plain GEMM with an index map, so none of them needs a tap table, index arithmetic per tap or activations in LDS:
//
//   * gather-GEMM (Conv2D forward, Conv2DTranspose data gradient): M = coarse pixels, K = 4 C, N output channels.  The K run of a
//     coarse pixel is four contiguous C-segments of the fine grid (two per fine row);
//   * scatter-GEMM (Conv2DTranspose forward, Conv2D data gradient): M = coarse pixels, K = C, N = 4 x output channels.  A
//     workgroup owns one tap of a channel tile, so every fine pixel is written exactly once: no read-modify-write, no atomics;
//   * weight gradient (both layer kinds): dW[coarse channel][kh][kw][fine channel] = sum over coarse pixels p of coarse[p] x
//     fine[2 p + (kh, kw)]: all four taps in one launch, the coarse tile staged once per pixel block.
//
// The two GEMMs are one kernel template (pw1x1.hip's scheme with a K loop): the kernel tile [32 ... 128 output channels][K] sits in
// LDS for the whole launch (<= 132 KB), each of the 8 waves owns strips of 32 coarse pixels whose MFMA operand comes straight from global memory in fragment
// layout (lane l: pixel l & 31, 8 consecutive channels, one 16-byte load per 16 values of K), K is walked in groups of 128 (64) values
// through two register buffers: the loads of the next group - of the next strip after the last group - are issued before the
// current group is computed.  Bias and addend in the register epilogue of pw1x1.hip (v_permlane32_swap, two 16-byte stores per 32
// channels), with the library's addend rule (include/unetrir.h): bf16(bf16(sum + bias) + addend).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include "kernels.h"
#include "mfma_types.h"

// (kernels outside an anonymous namespace: profilers print their names)
// NB = 32-channel blocks of the workgroup's channel tile.  SCATTER = false: the input pixel of K-segment t = 2 kh + kw is
// (2 py + kh, 2 px + kw), the output pixel (py, px).  SCATTER = true: input pixel (py, px), output pixel (2 py + kh, 2 px + kw)
// for the workgroup's tap.  Kernel rows: row (n, t) holds C contiguous values at ((n * 4 + t) * C) - the gather form reads the four
// rows of a channel as one run of K = 4 C, the scatter form the row of its tap.
#define C22_THREADS 512
template <int NB, bool SCATTER>
__global__ __launch_bounds__(C22_THREADS) void conv2x2s2_bf16_kernel(const C22Args a) {
    constexpr int NT = NB * 32;
    constexpr int G = NB == 1 ? 8 : NB == 2 ? 4 : 2;                     // 16-value k-blocks per group (two blocks of accumulators: K <= 256, registers for 4)
    constexpr int WAVES = C22_THREADS / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char c22_smem[];
    const int K = SCATTER ? a.C : 4 * a.C;
    const int LDW = K + 8;                                 // LDS row stride of the kernel tile (16-byte pad: rows 16 bytes apart mod 128)
    __bf16* Ws = reinterpret_cast<__bf16*>(c22_smem);      // [NT][LDW]
    float* s_bias = reinterpret_cast<float*>(c22_smem + (size_t)NT * LDW * 2);      // [NB][2][16]: [block][h][4 q + e] = channel 8 q + 4 h + e

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5, l31 = lane & 31;
    const int ntN = (a.N + NT - 1) / NT;                   // N = 16: half a block, the rows beyond N are zero and never stored
    const int ntiles = SCATTER ? ntN * 4 : ntN;
    // workgroups that read the same pixels (the channel tiles - and taps - of one strip group) sit on one XCD (blockIdx.x % 8)
    const int xcd = blockIdx.x & 7, q8 = blockIdx.x >> 3;
    const int tile = q8 % ntiles, wg = (q8 / ntiles) * 8 + xcd, nwg = gridDim.x / ntiles;       // gridDim.x = nwg * ntiles, nwg a multiple of 8
    const int tap = SCATTER ? (tile & 3) : 0;
    const int n0 = (SCATTER ? (tile >> 2) : tile) * NT;

    {   // ---- the kernel tile -> LDS, the bias as the accumulators want it
        const int pieces_row = K >> 3;                     // 16-byte pieces per row
        const int pieces = NT * pieces_row;
        for (int i = tid; i < pieces; i += C22_THREADS) {
            const int r = i / pieces_row, q = i - r * pieces_row;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (n0 + r < a.N) v = *reinterpret_cast<const u32x4*>(a.w + ((size_t)(n0 + r) * 4 + tap) * a.C + q * 8);
            *reinterpret_cast<u32x4*>(&Ws[r * LDW + q * 8]) = v;
        }
        if (tid < NT) {
            const int nb = tid >> 5, hh = (tid >> 4) & 1, r = tid & 15;
            const int n = n0 + 32 * nb + 8 * (r >> 2) + 4 * hh + (r & 3);
            s_bias[tid] = (a.bias && n < a.N) ? a.bias[n] : 0.f;
        }
    }
    __syncthreads();

    const unsigned M = (unsigned)a.B * a.PH * a.PW;       // < 2^31 (checked by the launcher), as are the fine-grid pixel counts
    const unsigned nstrip = (M + 31u) / 32u;
    const unsigned plane = (unsigned)a.PH * a.PW;
    const int FW = 2 * a.PW;                               // fine grid: 2 PH x 2 PW
    const int nkb = K >> 4, ngroups = (nkb + G - 1) / G;

    // pixel l31 of strip st: its input pixel (the cell's first one in the gather form), its output pixel, whether it exists
    auto decode = [&](unsigned st, unsigned& ipix, unsigned& opix, bool& ok) {
        const unsigned p = st * 32u + (unsigned)l31;
        ok = st < nstrip && p < M;
        ipix = 0; opix = 0;
        if (ok) {
            const unsigned b = p / plane, rem = p - b * plane;
            const unsigned py = rem / (unsigned)a.PW, px = rem - py * (unsigned)a.PW;
            const unsigned fine = (b * 2u * (unsigned)a.PH + 2u * py + (unsigned)(tap >> 1)) * (unsigned)FW + 2u * px + (unsigned)(tap & 1);
            ipix = SCATTER ? p : fine;
            opix = SCATTER ? fine : p;
        }
    };

    const unsigned sstep = (unsigned)nwg * WAVES;
    // the loading side runs one group ahead of the computing side; each keeps its own place (strip, group)
    unsigned ld_st = (unsigned)wg * WAVES + (unsigned)wave, cp_st = ld_st;
    int ld_grp = 0, cp_grp = 0;
    unsigned ld_ipix, cp_opix, scratch_u;
    bool ld_ok, cp_ok;
    decode(ld_st, ld_ipix, scratch_u, ld_ok);
    decode(cp_st, scratch_u, cp_opix, cp_ok);

    auto issue = [&](bf16x8 (&f)[G]) {
        const __bf16* src = a.in + (size_t)ld_ipix * a.ldi + 8 * h;
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int kb = ld_grp * G + j;
            u32x4 v = {0u, 0u, 0u, 0u};
            if (ld_ok && kb < nkb) {
                const int k0 = kb * 16;
                size_t off = (size_t)k0;
                if (!SCATTER) {
                    const int t = k0 >> a.cshift;
                    off = (size_t)((t >> 1) * FW + (t & 1)) * a.ldi + (size_t)(k0 & (a.C - 1));
                }
                v = *reinterpret_cast<const u32x4*>(src + off);
            }
            f[j] = __builtin_bit_cast(bf16x8, v);
        }
        if (++ld_grp == ngroups) {
            ld_grp = 0;
            ld_st += sstep;
            decode(ld_st, ld_ipix, scratch_u, ld_ok);
        }
    };

    f32x16 acc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

    // the strip is complete: + bias, round, exchange so that a lane owns 16 CONSECUTIVE channels (pw1x1.hip), (+ addend), store
    auto epilogue = [&]() {
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            unsigned P[4][2], o[8];
            const float4* bp = reinterpret_cast<const float4*>(&s_bias[(nb * 2 + h) * 16]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b4 = bp[q];
                P[q][0] = pack2(acc[nb][4 * q + 0] + b4.x, acc[nb][4 * q + 1] + b4.y);
                P[q][1] = pack2(acc[nb][4 * q + 2] + b4.z, acc[nb][4 * q + 3] + b4.w);
            }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const auto r = __builtin_amdgcn_permlane32_swap(P[jj][e], P[jj + 2][e], false, false);
                    o[4 * jj + e] = r[0];              // channels 16 h + 8 jj + {2 e, 2 e + 1}
                    o[4 * jj + 2 + e] = r[1];          // channels 16 h + 8 jj + 4 + {2 e, 2 e + 1}
                }
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;
            const int cbase = n0 + 32 * nb + 16 * h;
            if (!cp_ok || cbase >= a.N) continue;
            if (a.addend) {
                const __bf16* ad = a.addend + (size_t)cp_opix * a.ldadd + cbase;
                const u32x4 a0 = *reinterpret_cast<const u32x4*>(ad), a1 = *reinterpret_cast<const u32x4*>(ad + 8);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = pack2(lo16(o[i]) + lo16(a0[i]), hi16(o[i]) + hi16(a0[i]));
                    o[4 + i] = pack2(lo16(o[4 + i]) + lo16(a1[i]), hi16(o[4 + i]) + hi16(a1[i]));
                }
            }
            __bf16* dst = a.out + (size_t)cp_opix * a.ldo + cbase;
            const u32x4 v0 = {o[0], o[1], o[2], o[3]}, v1 = {o[4], o[5], o[6], o[7]};
            *reinterpret_cast<u32x4*>(dst) = v0;
            *reinterpret_cast<u32x4*>(dst + 8) = v1;
        }
    };

    auto compute = [&](const bf16x8 (&f)[G]) {
#pragma unroll
        for (int j = 0; j < G; ++j) {
            const int kb = cp_grp * G + j;
            if (kb < nkb) {
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const bf16x8 fb = *reinterpret_cast<const bf16x8*>(&Ws[(nb * 32 + l31) * LDW + kb * 16 + 8 * h]);
                    acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fb, f[j], acc[nb], 0, 0, 0);
                }
            }
        }
        if (++cp_grp == ngroups) {
            epilogue();
            cp_grp = 0;
            cp_st += sstep;
            decode(cp_st, scratch_u, cp_opix, cp_ok);
        }
    };

    bf16x8 f0[G], f1[G];
    issue(f0);
    while (cp_st < nstrip) {
        issue(f1);
        compute(f0);
        if (cp_st >= nstrip) break;
        issue(f0);
        compute(f1);
    }
}

// ---- weight gradient: workgroup = a 64 x 64 tile of (coarse channels S, fine channels L) for all four taps and one split-K slice of
// the coarse pixels; wave (wr, wc) owns 32 x 32 of it: four accumulators.  K = pixels is the STRIDED dimension of NHWC, so the
// operands come out of LDS through ds_read_b64_tr_b16 as in wgrad3x3.hip.  A K block is 32 consecutive coarse pixels of the flat
// B x PH x PW grid (no halo: a block needs no shape) - 16 bytes of the coarse tile and 4 x 16 bytes of the fine tiles per thread,
// fetched for the next block while the current one is multiplied.
#define C22_WG_PIX 32
__global__ __launch_bounds__(256, 2) void conv2x2s2_wgrad_bf16_kernel(const C22WgradArgs a) {
    constexpr int LD = 96;      // 192-byte LDS rows: 4 consecutive pixel rows start 64 B apart modulo 256 (the transposed reads)
    __shared__ __attribute__((aligned(16))) __bf16 Ss[C22_WG_PIX * LD];
    __shared__ __attribute__((aligned(16))) __bf16 Ls[4][C22_WG_PIX * LD];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;
    const int ntL = (a.L + 63) / 64;
    const int rt = blockIdx.x / ntL, ct = blockIdx.x - rt * ntL;
    const int s0 = rt * 64, l0 = ct * 64;
    const long long M = (long long)a.B * a.PH * a.PW;
    const long long nblk = (M + C22_WG_PIX - 1) / C22_WG_PIX;
    const long long b0 = (long long)blockIdx.y * a.blocks_per_split;
    long long b1 = b0 + a.blocks_per_split;
    if (b1 > nblk) b1 = nblk;

    const int q8 = tid & 7, pix = tid >> 3;                // this thread's 8 channels and its pixel of the block
    const bool sok = (s0 + q8 * 8) < a.S, lok = (l0 + q8 * 8) < a.L;
    const unsigned plane = (unsigned)a.PH * a.PW;
    const unsigned FW = 2u * (unsigned)a.PW;

    uint4 rs, rl[4];
    auto load_block = [&](long long blk) {
        const long long p = blk * C22_WG_PIX + pix;
        rs = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
        for (int t = 0; t < 4; ++t) rl[t] = make_uint4(0u, 0u, 0u, 0u);
        if (p < M) {
            const unsigned pu = (unsigned)p;
            const unsigned b = pu / plane, rem = pu - b * plane;
            const unsigned py = rem / (unsigned)a.PW, px = rem - py * (unsigned)a.PW;
            if (sok) rs = *reinterpret_cast<const uint4*>(a.small + (size_t)pu * a.lds + s0 + q8 * 8);
            if (lok) {
                const size_t fine = (size_t)(b * 2u * (unsigned)a.PH + 2u * py) * FW + 2u * px;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    rl[t] = *reinterpret_cast<const uint4*>(a.large + (fine + (size_t)((t >> 1) * FW + (t & 1))) * a.ldl + l0 + q8 * 8);
            }
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // ds_read_b64_tr_b16: inside each 16-lane group lane 4 q + p supplies the address of row q (a pixel), columns 4 p .. 4 p + 3
    // (channels); lane i of the group receives column i of the 4 rows.  Operand lane l wants channel (l & 31) and pixels
    // 8 (l >> 5) + j of the 16-pixel K step.
    const int grp = lane >> 4, li = lane & 15;
    const int tq = li >> 2, tp = li & 3;
    const int chan = (grp & 1) * 16 + tp * 4;
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const int slane = (h * 8 + tq) * LD + wr * 32 + chan;          // + (16 s + 4 rd) * LD
    const int llane = (h * 8 + tq) * LD + wc * 32 + chan;

    if (b0 < b1) load_block(b0);
    for (long long blk = b0; blk < b1; ++blk) {
        if (blk != b0) __syncthreads();
        *reinterpret_cast<uint4*>(&Ss[pix * LD + q8 * 8]) = rs;
#pragma unroll
        for (int t = 0; t < 4; ++t) *reinterpret_cast<uint4*>(&Ls[t][pix * LD + q8 * 8]) = rl[t];
        __syncthreads();
        if (blk + 1 < b1) load_block(blk + 1);
#pragma unroll
        for (int s = 0; s < C22_WG_PIX / 16; ++s) {
            const bf16x4 alo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ss + slane + (s * 16) * LD));
            const bf16x4 ahi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ss + slane + (s * 16 + 4) * LD));
            const bf16x8 fa = __builtin_shufflevector(alo, ahi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ls[t] + llane + (s * 16) * LD));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ls[t] + llane + (s * 16 + 4) * LD));
                const bf16x8 fb = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
            }
        }
    }

    // slab [S][4][L]: a lane holds fine channel l & 31 of coarse channels 8 q + 4 h + e
    float* part = a.part + (size_t)blockIdx.y * a.S * 4 * a.L;
    const int c = l0 + wc * 32 + (lane & 31);
    if (c < a.L) {
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = s0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < a.S) part[((size_t)n * 4 + t) * a.L + c] = acc[t][r];
            }
    }
}

namespace {
inline bool pow2_16_to(int c, int hi) { return c >= 16 && c <= hi && (c & (c - 1)) == 0; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// channel tile (32-channel blocks) and workgroups per tile of a GEMM launch: the widest tile whose rows fit LDS (128 channels at
// K = 256 and 512, 64 up to K = 1024, 32 at K = 2048: <= 132 KB) - every tile re-reads the pixels; per tile a multiple of 8 workgroups
// (XCD mapping), about 256 workgroups of 8 waves in all, never more than there are groups of 8 strips
void gemm_plan(const C22Args& a, bool scatter, int* nb, unsigned* per_tile, size_t* smem) {
    const int K = scatter ? a.C : 4 * a.C;
    *nb = (a.N % 128 == 0 && K >= 256 && K <= 512) ? 4 : (a.N % 64 == 0 && K <= 1024) ? 2 : 1;
    const int NT = 32 * *nb;
    const int ntiles = (a.N + NT - 1) / NT * (scatter ? 4 : 1);
    const long long M = (long long)a.B * a.PH * a.PW;
    const long long groups = (M + 32 * (C22_THREADS / 64) - 1) / (32 * (C22_THREADS / 64));
    long long g = 256 / ntiles;
    if (g < 8) g = 8;
    if (g > groups) g = groups;
    g = (g + 7) / 8 * 8;
    *per_tile = (unsigned)g;
    *smem = (size_t)NT * (K + 8) * 2 + (size_t)NT * sizeof(float);
}

template <int NB, bool SCATTER>
int launch_gemm(const C22Args& a, unsigned grid, size_t smem, hipStream_t s) {
    if (smem > (64 << 10)) {
        // Dynamic LDS above 64 KB has to be asked for, per device and kernel: asked ONCE, for the most any launch needs (160 KB), and
        // remembered in an append-only flag per device (a race sets it twice: harmless).  hipFuncSetAttribute is a property of the
        // function, not a stream operation, so it is not captured into a HIP graph; the trainer also runs one ordinary step before
        // it captures, so under capture the flag is already set.
        static std::atomic<bool> asked[16];
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return UNETRIR_EINVAL;
        if (!asked[dev].load(std::memory_order_acquire)) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2x2s2_bf16_kernel<NB, SCATTER>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 160 << 10);
            if (e != hipSuccess) return (int)e;
            asked[dev].store(true, std::memory_order_release);
        }
    }
    hipLaunchKernelGGL((conv2x2s2_bf16_kernel<NB, SCATTER>), dim3(grid), dim3(C22_THREADS), smem, s, a);
    return (int)hipGetLastError();
}
}  // namespace

// Shape rules of the two GEMM forms.  C = channels of one K segment (a power of two: the segment of a k-block is a shift), N output
// channels; the kernel tile of 32 channels must fit LDS: K = 4 C <= 2048 (gather), K = C <= 1024 (scatter).
bool conv2x2s2_gemm_applies(const C22Args& a, bool scatter) {
    const long long M = (long long)a.B * a.PH * a.PW;
    if (a.B <= 0 || a.PH <= 0 || a.PW <= 0 || 4 * M >= (1ll << 31)) return false;
    if (!pow2_16_to(a.C, scatter ? 1024 : 512) || !pow2_16_to(a.N, 1024)) return false;
    if (a.ldi < a.C || (a.ldi & 7) || a.ldo < a.N || (a.ldo & 7) || (a.addend && (a.ldadd < a.N || (a.ldadd & 7)))) return false;
    return true;
}

int launch_conv2x2s2_gemm_bf16(C22Args a, bool scatter, hipStream_t s) {
    if (!conv2x2s2_gemm_applies(a, scatter) || !a.in || !a.w || !a.out) return UNETRIR_EINVAL;
    if (!aligned16(a.in) || !aligned16(a.w) || !aligned16(a.out) || !aligned16(a.addend)) return UNETRIR_EINVAL;
    a.cshift = __builtin_ctz((unsigned)a.C);
    int nb; unsigned g; size_t smem;
    gemm_plan(a, scatter, &nb, &g, &smem);
    const unsigned grid = g * (unsigned)((a.N + 32 * nb - 1) / (32 * nb)) * (scatter ? 4u : 1u);
    if (scatter) return nb == 4 ? launch_gemm<4, true>(a, grid, smem, s) : nb == 2 ? launch_gemm<2, true>(a, grid, smem, s) : launch_gemm<1, true>(a, grid, smem, s);
    return nb == 4 ? launch_gemm<4, false>(a, grid, smem, s) : nb == 2 ? launch_gemm<2, false>(a, grid, smem, s) : launch_gemm<1, false>(a, grid, smem, s);
}

// Split of the weight gradient: about 512 workgroups over the 64 x 64 channel tiles, at least 4 pixel blocks per slice.
void conv2x2s2_wgrad_plan(int B, int PH, int PW, int S, int L, int* nslabs, long long* blocks_per_split) {
    const long long nblk = ((long long)B * PH * PW + C22_WG_PIX - 1) / C22_WG_PIX;
    const long long tiles = (long long)((S + 63) / 64) * ((L + 63) / 64);
    long long want = (512 + tiles - 1) / tiles;
    long long maxs = (nblk + 3) / 4;
    if (maxs < 1) maxs = 1;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    *blocks_per_split = (nblk + want - 1) / want;
    *nslabs = (int)((nblk + *blocks_per_split - 1) / *blocks_per_split);
}

bool conv2x2s2_wgrad_applies(const C22WgradArgs& a) {
    const long long M = (long long)a.B * a.PH * a.PW;
    if (a.B <= 0 || a.PH <= 0 || a.PW <= 0 || 4 * M >= (1ll << 31)) return false;
    if (!pow2_16_to(a.S, 1024) || !pow2_16_to(a.L, 512)) return false;
    return a.lds >= a.S && !(a.lds & 7) && a.ldl >= a.L && !(a.ldl & 7);
}

int launch_conv2x2s2_wgrad_bf16(const C22WgradArgs& a, int nslabs, hipStream_t s) {
    if (!conv2x2s2_wgrad_applies(a) || !a.small || !a.large || !a.part || !aligned16(a.small) || !aligned16(a.large)) return UNETRIR_EINVAL;
    const unsigned tiles = (unsigned)(((a.S + 63) / 64) * ((a.L + 63) / 64));
    hipLaunchKernelGGL(conv2x2s2_wgrad_bf16_kernel, dim3(tiles, nslabs), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
