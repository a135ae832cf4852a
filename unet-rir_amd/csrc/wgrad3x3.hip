// wgrad3x3.hip - weight gradient of the 3x3 Conv2D layers (stride 1 or 2, TF 'same'): the patch-walking kernel in fp32 MFMA and,
// further down, its bf16 twin (which also serves the 1x1 layers).
//
// dw[n][t][c] = sum_p dy[p][n] * x[p*S + off_t][c].  The generic kernel (igemm.hip) gathers one x tile per tap,
// so every staged byte feeds 1/9 of the taps.  Here the K dimension is walked in 4x8-pixel patches: the x patch
// WITH HALO ((3S+3) x (7S+3) pixels) is staged once in LDS and all 9 taps read it at shifted addresses, and the dy
// patch is staged once for all 9 taps.  One workgroup owns a 64 (Cout) x 64 (Cin) x 9 (taps) slab of dw: each of
// its 4 waves keeps 9 accumulator tiles of 32x32 (144 AGPRs) and issues 9 MFMAs per 10 LDS reads.
// Staged bytes per MFMA fall ~5x against the gathered form; partial slabs + fixed-order reduce keep it deterministic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "kernels.h"
#include "mfma_types.h"

#define TPW WG_TPW       // patch width (output pixels); patch height TPH_ is 4 (stride 1) or 2 (stride 2)
#define W3_LD 68          // 64 channels + 4 pad (floats)

template <int SI, int TPH>
__global__ __launch_bounds__(256, 2) void wgrad3x3_kernel(const Wgrad3Args a) {
    constexpr int XH = (TPH - 1) * SI + 3, XW = (TPW - 1) * SI + 3;
    constexpr int DJ = TPH * TPW * 16 / 256;         // dy float4 rounds per thread
    constexpr int XN = XH * XW * 16;                 // float4 slots of the x patch (16 quads per pixel)
    constexpr int XJ = (XN + 255) / 256;
    __shared__ __attribute__((aligned(16))) float Xs[XH * XW * W3_LD];
    __shared__ __attribute__((aligned(16))) float Ds[TPH * TPW * W3_LD];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    const int ntC = (a.C + 63) / 64;
    const int rt = blockIdx.x / ntC, ct = blockIdx.x - rt * ntC;
    const int n0 = rt * 64, c0 = ct * 64;
    const int per_img = a.npy * a.npx;
    const int G = a.B * per_img;
    const int g0 = blockIdx.y * a.patches_per_split;
    int g1 = g0 + a.patches_per_split;
    if (g1 > G) g1 = G;

    float4 rx[XJ], rd[DJ];
    const int q = tid & 15;
    const bool cok = (c0 + q * 4) < a.C, nok = (n0 + q * 4) < a.N;

    auto load_patch = [&](int g) {
        const int img = g / per_img;
        const int rem = g - img * per_img;
        const int pyi = rem / a.npx, pxi = rem - pyi * a.npx;
        const int py0 = pyi * TPH, px0 = pxi * TPW;
        const int iy0 = py0 * SI - a.pad_t, ix0 = px0 * SI - a.pad_l;
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int i = tid + 256 * j;
            const int pp = i >> 4;
            const int pr = pp / XW, pc = pp - pr * XW;
            const int iy = iy0 + pr, ix = ix0 + pc;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (i < XN && cok && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = *reinterpret_cast<const float4*>(a.x + ((size_t)((long long)img * a.IH + iy) * a.IW + ix) * a.ldx + c0 + q * 4);
            rx[j] = v;
        }
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            const int pix = (tid + 256 * j) >> 4;
            const int oy = py0 + (pix >> 3), ox = px0 + (pix & 7);
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (nok && oy < a.OH && ox < a.OW)
                v = *reinterpret_cast<const float4*>(a.dy + ((size_t)((long long)img * a.OH + oy) * a.OW + ox) * a.lddy + n0 + q * 4);
            rd[j] = v;
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const float* dbase = &Ds[h * W3_LD + wr * 32 + l31];
    const float* xbase = &Xs[h * SI * W3_LD + wc * 32 + l31];

    if (g0 < g1) load_patch(g0);
    for (int g = g0; g < g1; ++g) {
        if (g != g0) __syncthreads();
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int i = tid + 256 * j;
            if (i < XN) *reinterpret_cast<float4*>(&Xs[(i >> 4) * W3_LD + q * 4]) = rx[j];
        }
#pragma unroll
        for (int j = 0; j < DJ; ++j) *reinterpret_cast<float4*>(&Ds[((tid + 256 * j) >> 4) * W3_LD + q * 4]) = rd[j];
        __syncthreads();
        if (g + 1 < g1) load_patch(g + 1);
#pragma unroll
        for (int s = 0; s < TPH * TPW / 2; ++s) {
            const int k0 = 2 * s, r = k0 >> 3, cc = k0 & 7;      // pixel k0 + h = (r, cc + h) inside the patch
            const float fa = dbase[k0 * W3_LD];
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int kh = t / 3, kw = t - kh * 3;
                const float fb = xbase[((r * SI + kh) * XW + cc * SI + kw) * W3_LD];
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[t], 0, 0, 0);
            }
        }
    }

    // epilogue: rows (registers) = output channel n, cols (lanes) = input channel c
    float* part = a.part + (size_t)blockIdx.y * a.N * 9 * a.C;
    const int c = c0 + wc * 32 + l31;
    if (c < a.C) {
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < a.N) part[((size_t)n * 9 + t) * a.C + c] = acc[t][r];
            }
    }
}

int launch_wgrad3x3(const Wgrad3Args& a, int stride, int nslabs, hipStream_t s) {
    const unsigned tiles = (unsigned)(((a.N + 63) / 64) * ((a.C + 63) / 64));
    if (stride == 1) hipLaunchKernelGGL((wgrad3x3_kernel<1, WG_F32_TPH_S1>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wgrad3x3_kernel<2, WG_F32_TPH_S2>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// the same patch scheme with bf16 operands and fp32 partial slabs: K = pixels is the STRIDED dimension of NHWC tiles, so the
// operands come out of LDS through ds_read_b64_tr_b16 (hardware 4x16 transpose), two reads per operand
// ------------------------------------------------------------------------------------------------

// KS = 3: the 3x3 layers.  KS = 1: the 1x1 layers of the residual graphs (dl_models/res_ae.py:455-512) - the same patch scheme
// with one tap and no halo (pad_t = pad_l = 0).
template <int SI, int TPH, int PADV = 1, int KS = 3>
__global__ __launch_bounds__(256, 2) void wgrad3x3_bf16_kernel(const Wgrad3ArgsH a) {
    constexpr int NT = KS * KS;
    constexpr int XH = (TPH - 1) * SI + KS, XW = (TPW - 1) * SI + KS;
    constexpr int XN = XH * XW * 8;                  // 16-byte slots of the x patch (8 per pixel: 64 channels)
    constexpr int XJ = (XN + 255) / 256;
    constexpr int DN = TPH * TPW * 8;                // 16-byte slots of the dy patch
    constexpr int DJ = (DN + 255) / 256;
    // Row strides (elements) chosen for the transposed reads: a 16-lane group of ds_read_b64_tr_b16 touches 4 pixel rows x
    // 64 B (two groups share a 32-lane conflict domain), so 4 consecutive rows - SI rows apart in the x patch - must start
    // 64 B apart modulo the 256-B bank row: 192 B for stride-1 rows, 160 B for the stride-2 x patch (144 B is 2-way).
    constexpr int LDD = PADV ? 96 : 72, LDX = PADV ? (SI == 1 ? 96 : 80) : 72;
    __shared__ __attribute__((aligned(16))) __bf16 Xs[XH * XW * LDX];
    __shared__ __attribute__((aligned(16))) __bf16 Ds[TPH * TPW * LDD];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int h = lane >> 5;
    const int wr = wave >> 1, wc = wave & 1;

    const int ntC = (a.C + 63) / 64;
    const int rt = blockIdx.x / ntC, ct = blockIdx.x - rt * ntC;
    const int n0 = rt * 64, c0 = ct * 64;
    const int per_img = a.npy * a.npx;
    const int G = a.B * per_img;
    const int g0 = blockIdx.y * a.patches_per_split;
    int g1 = g0 + a.patches_per_split;
    if (g1 > G) g1 = G;

    uint4 rx[XJ], rd[DJ];
    const int q8 = tid & 7;
    const bool cok = (c0 + q8 * 8) < a.C, nok = (n0 + q8 * 8) < a.N;

    auto load_patch = [&](int g) {
        const int img = g / per_img;
        const int rem = g - img * per_img;
        const int pyi = rem / a.npx, pxi = rem - pyi * a.npx;
        const int py0 = pyi * TPH, px0 = pxi * TPW;
        const int iy0 = py0 * SI - a.pad_t, ix0 = px0 * SI - a.pad_l;
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int i = tid + 256 * j;
            const int pp = i >> 3;
            const int pr = pp / XW, pc = pp - pr * XW;
            const int iy = iy0 + pr, ix = ix0 + pc;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (i < XN && cok && (unsigned)iy < (unsigned)a.IH && (unsigned)ix < (unsigned)a.IW)
                v = *reinterpret_cast<const uint4*>(a.x + ((size_t)((long long)img * a.IH + iy) * a.IW + ix) * a.ldx + c0 + q8 * 8);
            rx[j] = v;
        }
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            const int i = tid + 256 * j;
            const int pix = i >> 3;
            const int oy = py0 + (pix >> 3), ox = px0 + (pix & 7);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (i < DN && nok && oy < a.OH && ox < a.OW)
                v = *reinterpret_cast<const uint4*>(a.dy + ((size_t)((long long)img * a.OH + oy) * a.OW + ox) * a.lddy + n0 + q8 * 8);
            rd[j] = v;
        }
    };

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    // ds_read_b64_tr_b16: inside each 16-lane group lane 4q+p supplies the address of LDS-matrix row q (a pixel),
    // columns 4p..4p+3 (channels); lane i of the group receives column i of the 4 rows.  Operand lane l wants
    // channel (l&31) and pixels 8*(l>>5)+j: groups 0/1 cover channels 0-15/16-31 of the low k half, 2/3 the high half.
    const int grp = lane >> 4, li = lane & 15;
    const int tq = li >> 2, tp = li & 3;
    const int chan = (grp & 1) * 16 + tp * 4;
    // pixel (inside a 16-pixel K step = 2 patch rows of 8) supplied by this lane for read rd: row h, col 4*rd + tq
    typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
    const int dlane = (h * 8 + tq) * LDD + wr * 32 + chan;                       // + (s*16 + 4*rd) * LDD
    const int xlane = ((h * SI) * XW + tq * SI) * LDX + wc * 32 + chan;          // + ((2s*SI + kh) * XW + 4*rd*SI + kw) * LDX

    if (g0 < g1) load_patch(g0);
    for (int g = g0; g < g1; ++g) {
        if (g != g0) __syncthreads();
#pragma unroll
        for (int j = 0; j < XJ; ++j) {
            const int i = tid + 256 * j;
            if (i < XN) *reinterpret_cast<uint4*>(&Xs[(i >> 3) * LDX + q8 * 8]) = rx[j];
        }
#pragma unroll
        for (int j = 0; j < DJ; ++j) {
            const int i = tid + 256 * j;
            if (i < DN) *reinterpret_cast<uint4*>(&Ds[(i >> 3) * LDD + q8 * 8]) = rd[j];
        }
        __syncthreads();
        if (g + 1 < g1) load_patch(g + 1);
#pragma unroll
        for (int s = 0; s < TPH / 2; ++s) {
            bf16x8 fa;
            {
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ds + dlane + (s * 16) * LDD));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Ds + dlane + (s * 16 + 4) * LDD));
                fa = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int kh = t / KS, kw = t - kh * KS;
                const int off0 = ((2 * s * SI + kh) * XW + kw) * LDX;
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Xs + xlane + off0));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(Xs + xlane + off0 + 4 * SI * LDX));
                const bf16x8 fb = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
            }
        }
    }

    float* part = a.part + (size_t)blockIdx.y * a.N * NT * a.C;
    const int c = c0 + wc * 32 + (lane & 31);
    if (c < a.C) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wr * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (n < a.N) part[((size_t)n * NT + t) * a.C + c] = acc[t][r];
            }
    }
}

int launch_wgrad3x3_bf16(const Wgrad3ArgsH& a, int stride, int nslabs, hipStream_t s) {
    const unsigned tiles = (unsigned)(((a.N + 63) / 64) * ((a.C + 63) / 64));
    if (stride == 1) hipLaunchKernelGGL((wgrad3x3_bf16_kernel<1, WG_BF16_TPH_S1>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wgrad3x3_bf16_kernel<2, WG_BF16_TPH_S2>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}

// 1x1 weight gradient (stride 1 or 2): the KS = 1 instance of the patch kernel
int launch_wgrad1x1_bf16(const Wgrad3ArgsH& a, int stride, int nslabs, hipStream_t s) {
    const unsigned tiles = (unsigned)(((a.N + 63) / 64) * ((a.C + 63) / 64));
    if (stride == 1) hipLaunchKernelGGL((wgrad3x3_bf16_kernel<1, WG_1X1_TPH_S1, 1, 1>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    else hipLaunchKernelGGL((wgrad3x3_bf16_kernel<2, WG_1X1_TPH_S2, 1, 1>), dim3(tiles, nslabs), dim3(256), 0, s, a);
    return (int)hipGetLastError();
}
