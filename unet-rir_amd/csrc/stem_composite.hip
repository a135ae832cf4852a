// stem_composite.hip - the stem's gradients (enc1.down: Conv2D(64, 3x3) on the 2-channel input) taken THROUGH the next layer
// (enc1.cb1: Conv2D(64 -> 64, 3x3)) without forming the data gradient between them (bf16 storage, stride 1).
//
// The two convolutions are linear with nothing in between, so with G = dL/d(enc1.cb1 output), x = the network input (both zero
// outside the image), W1 the enc1.cb1 kernel and taps t0, t1 in {0,1,2}^2:
//     dW0[co0][t0][ci] = sum_{t1,co1} W1[co1][t1][co0] * (S[t0 + t1 - 2][ci][co1] - E[t0][t1][ci][co1])
//     db0[co0]         = sum_{t1,co1} W1[co1][t1][co0] * (T[co1] - F[t1][co1])
//     S[d][ci][co1] = sum_p x[p + d][ci] * G[p][co1]  (d in {-2..2}^2),   T[co1] = sum_p G[p][co1]
// E and F are the same sums over the pixels p whose neighbour p + t1 - 1 lies outside the image: the intermediate tensor is
// zero-padded at its own border, not computed from x there.  That pixel set is the union of at most one frame row and one frame
// column, so E and F come from sums over the four frame lines and the four corner pixels: row + column - corner.
//
// Launches: (1) the 5 x 5 correlation S and T on the matrix cores - head_mfma.hip's weight-gradient kernel with x in the role
// of dy and G in the role of the 64-channel tensor, G read once; (2) the frame sums, one workgroup per image and frame line;
// (3) a fixed-order fp64 reduction of both sets of partials; (4) the contraction with W1, which writes the two gradients in the
// flat buffer's layouts.  No atomics: every sum has a fixed order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "kernels.h"

#define SC_C 64                       // channels of G and of the stem (co1, co0)
#define SC_SROWS 73                   // rows of one correlation partial: (ci, kh, kw) of a 6 x 6 table + the pixel sums
#define SC_BSLOTS 51                  // frame sums per line: 25 offsets x 2 input channels + the plain sum of G
#define SC_LINES 8                    // top, bottom, left, right, then the corners TL, TR, BL, BR
#define SC_CORR_BLOCKS 512

#define SC_CHUNK 256                  // frame pixels per staging step of the frame kernel

__device__ __forceinline__ float sc_bf16(const __bf16* p) { return (float)*p; }

// Frame sums.  Block (img, line) with line 0 = row 0, 1 = row H-1, 2 = column 0, 3 = column W-1; lane = channel co1.
// out[img][line][slot][co1]; the blocks of the two rows also write the corner pixels' own terms (lines 4..7).  Slot
// (5 (dy + 2) + (dx + 2)) * 2 + ci holds sum x[p + d][ci] * G[p][co1], slot 50 sum G[p][co1].
// The line runs in chunks of 256 pixels: the five lines of x around it (offset a across the line, 2 pixels of halo along it,
// zero outside the image) are staged in LDS once, wave w takes the chunk's pixels w, w + 8, ... - its 32 loads of G in flight
// beside the staging, then 25 broadcast LDS reads and 50 FMAs per pixel.  The accumulators are indexed (across, along); the store
// turns that into (dy, dx).
__global__ __launch_bounds__(512) void stem_frame_kernel(const __bf16* __restrict__ g, int ldg, const __bf16* __restrict__ x, int ldx,
                                                         int H, int W, float* __restrict__ out) {
    __shared__ float2 xs[5][SC_CHUNK + 4];
    __shared__ float sum[SC_BSLOTS][SC_C];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int img = blockIdx.x, line = blockIdx.y;
    const bool row = line < 2;
    const int fix = (line & 1) ? (row ? H : W) - 1 : 0;       // the line's own row / column
    const __bf16* gi = g + (size_t)img * H * W * ldg + lane;
    const __bf16* xi = x + (size_t)img * H * W * ldx;
    const int n = row ? W : H;

    float acc[SC_BSLOTS];
#pragma unroll
    for (int s = 0; s < SC_BSLOTS; ++s) acc[s] = 0.f;
    for (int j0 = 0; j0 < n; j0 += SC_CHUNK) {
        float gg[SC_CHUNK / 8];                            // this wave's pixels of the chunk: all loads in flight beside the staging
#pragma unroll
        for (int u = 0; u < SC_CHUNK / 8; ++u) {
            const int j = j0 + wave + 8 * u;
            gg[u] = 0.f;                                   // past the end of the line: contributes nothing
            if (j < n) gg[u] = sc_bf16(gi + (row ? (size_t)fix * W + j : (size_t)j * W + fix) * ldg);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 5 * (SC_CHUNK + 4); i += 512) {
            const int a = i / (SC_CHUNK + 4), t = i - a * (SC_CHUNK + 4);
            const int across = fix + a - 2, along = j0 + t - 2;
            const int qy = row ? across : along, qx = row ? along : across;
            float2 v = make_float2(0.f, 0.f);
            if ((unsigned)qy < (unsigned)H && (unsigned)qx < (unsigned)W) {
                const __bf16* xp = xi + ((size_t)qy * W + qx) * ldx;
                v = make_float2(sc_bf16(xp), sc_bf16(xp + 1));
            }
            xs[a][t] = v;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < SC_CHUNK / 8; ++u) {
            const int t = wave + 8 * u;                    // position in the chunk; t + b <= 259
            if (j0 + t < n) {
#pragma unroll
                for (int a = 0; a < 5; ++a)
#pragma unroll
                    for (int b = 0; b < 5; ++b) {
                        const float2 xv = xs[a][t + b];
                        acc[(a * 5 + b) * 2] += xv.x * gg[u];
                        acc[(a * 5 + b) * 2 + 1] += xv.y * gg[u];
                    }
                acc[50] += gg[u];
            }
        }
    }
    // the eight waves' sums in wave order
    for (int w = 0; w < 8; ++w) {
        if (wave == w) {
#pragma unroll
            for (int s = 0; s < SC_BSLOTS; ++s) sum[s][lane] = (w == 0 ? 0.f : sum[s][lane]) + acc[s];
        }
        __syncthreads();
    }
    float* o = out + ((size_t)img * SC_LINES + line) * SC_BSLOTS * SC_C;
    for (int i = threadIdx.x; i < SC_BSLOTS * SC_C; i += 512) {
        const int s = i / SC_C, c = i - s * SC_C;
        int src = s;
        if (s < 50 && !row) {                              // (dy, dx) = (along, across) on a column
            const int d = s >> 1, dy = d / 5, dx = d - dy * 5;
            src = (dx * 5 + dy) * 2 + (s & 1);
        }
        o[i] = sum[src][c];
    }
    if (row && wave < 2) {                 // corner pixels of this row: line 4 + 2 * line + wave
        const int py = fix, px = wave == 0 ? 0 : W - 1;
        const float gv = sc_bf16(gi + ((size_t)py * W + px) * ldg);
        float* oc = out + ((size_t)img * SC_LINES + 4 + 2 * line + wave) * SC_BSLOTS * SC_C;
#pragma unroll
        for (int d = 0; d < 25; ++d) {
            const int qy = py + d / 5 - 2, qx = px + d % 5 - 2;
            float x0 = 0.f, x1 = 0.f;
            if ((unsigned)qy < (unsigned)H && (unsigned)qx < (unsigned)W) {
                const __bf16* xp = xi + ((size_t)qy * W + qx) * ldx;
                x0 = sc_bf16(xp); x1 = sc_bf16(xp + 1);
            }
            oc[(size_t)(2 * d) * SC_C + lane] = x0 * gv;
            oc[(size_t)(2 * d + 1) * SC_C + lane] = x1 * gv;
        }
        oc[(size_t)50 * SC_C + lane] = gv;
    }
}

// Fixed-order fp64 sums of the partials: sf[73][64] over the nblk correlation workgroups (rows of the unused sixth vertical tap:
// 0), rf[8][51][64] over the B images.  A block is 16 outputs x 16 partial-row classes (rows r = class, class + 16, ...), the
// classes then added in order.
__global__ __launch_bounds__(256) void stem_finalize_kernel(const float* __restrict__ ps, int nblk, const float* __restrict__ pb, int B,
                                                            double* __restrict__ sf, double* __restrict__ rf) {
    __shared__ double red[16][17];
    const int o16 = threadIdx.x & 15, cls = threadIdx.x >> 4;
    constexpr int NS = SC_SROWS * SC_C, NB = SC_LINES * SC_BSLOTS * SC_C;
    const int i = blockIdx.x * 16 + o16;
    const bool is_s = i < NS;
    const float* p = is_s ? ps + i : pb + (i - NS);
    const int np = is_s ? nblk : B;
    const size_t stride = is_s ? (size_t)NS : (size_t)NB;
    bool live = i < NS + NB;
    if (is_s) {
        const int row = i / SC_C;
        if (row < 72 && (row % 36) / 6 == 5) live = false;
    }
    double a = 0.0;
    if (live)
        for (int r = cls; r < np; r += 16) a += (double)p[(size_t)r * stride];
    red[cls][o16] = a;
    __syncthreads();
    if (cls == 0 && i < NS + NB) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][o16];
        if (is_s) sf[i] = t; else rf[i - NS] = t;
    }
}

// dW0 / db0 of output channel co0 = blockIdx.x; thread = co1.  w1t: the bf16 work copy [co0][t1][co1] of the enc1.cb1 kernel (what
// the data gradient multiplied by).  dw0 [64][9][ldw] (channels >= 2: the zero padding of the 2-channel end) = sum + reg * w0.
__global__ __launch_bounds__(64) void stem_contract_kernel(const double* __restrict__ sf, const double* __restrict__ rf,
                                                           const __bf16* __restrict__ w1t, float reg, const float* __restrict__ w0,
                                                           float* __restrict__ dw0, int ldw, float* __restrict__ db0) {
    __shared__ double red[19][SC_C];
    const int co0 = blockIdx.x, co1 = threadIdx.x;
    double acc[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) acc[k] = 0.0;
    auto frame = [&](int line, int slot) { return rf[((size_t)line * SC_BSLOTS + slot) * SC_C + co1]; };
#pragma unroll
    for (int t1 = 0; t1 < 9; ++t1) {
        const int t1y = t1 / 3, t1x = t1 % 3;
        const double w = (double)(float)w1t[((size_t)co0 * 9 + t1) * SC_C + co1];
        // the frame lines tap t1 looks across: the pixels there see the zero padding of the intermediate tensor
        const int lr = t1y == 0 ? 0 : t1y == 2 ? 1 : -1, lc = t1x == 0 ? 2 : t1x == 2 ? 3 : -1;
        const int corner = (lr >= 0 && lc >= 0) ? 4 + 2 * lr + (lc - 2) : -1;
        auto border = [&](int slot) {
            double e = 0.0;
            if (lr >= 0) e += frame(lr, slot);
            if (lc >= 0) e += frame(lc, slot);
            if (corner >= 0) e -= frame(corner, slot);
            return e;
        };
#pragma unroll
        for (int t0 = 0; t0 < 9; ++t0) {
            const int dy = t0 / 3 + t1y - 2, dx = t0 % 3 + t1x - 2;
#pragma unroll
            for (int ci = 0; ci < 2; ++ci) {
                const double s = sf[(size_t)(ci * 36 + (2 - dy) * 6 + (2 - dx)) * SC_C + co1];
                acc[2 * t0 + ci] += w * (s - border(((dy + 2) * 5 + dx + 2) * 2 + ci));
            }
        }
        acc[18] += w * (sf[(size_t)72 * SC_C + co1] - border(50));
    }
#pragma unroll
    for (int k = 0; k < 19; ++k) red[k][co1] = acc[k];
    __syncthreads();
    if (co1 < 19) {
        double t = 0.0;
        for (int c = 0; c < SC_C; ++c) t += red[co1][c];
        if (co1 == 18) db0[co0] = (float)t;
        else {
            const size_t o = ((size_t)co0 * 9 + (co1 >> 1)) * ldw + (co1 & 1);
            dw0[o] = (float)t + (reg != 0.f ? reg * w0[o] : 0.f);
        }
    }
    for (int k = co1; k < 9 * (ldw - 2); k += SC_C) {      // the padding channels, as the direct weight gradient leaves them
        const size_t o = ((size_t)co0 * 9 + k / (ldw - 2)) * ldw + 2 + k % (ldw - 2);
        dw0[o] = reg != 0.f ? reg * w0[o] : 0.f;
    }
}

namespace {

struct ScLayout { size_t ps, pb, sf, rf, end; };
ScLayout sc_layout(int B) {
    ScLayout l;
    l.ps = 0;
    l.pb = l.ps + (size_t)SC_CORR_BLOCKS * SC_SROWS * SC_C * sizeof(float);
    l.sf = l.pb + (size_t)B * SC_LINES * SC_BSLOTS * SC_C * sizeof(float);
    l.rf = l.sf + (size_t)SC_SROWS * SC_C * sizeof(double);
    l.end = l.rf + (size_t)SC_LINES * SC_BSLOTS * SC_C * sizeof(double);
    return l;
}

}  // namespace

bool stem_composite_applies(int B, int H, int W, int C0, int C1) {
    return B > 0 && B <= 65535 && H > 0 && W > 0 && W <= 4096 && C0 == SC_C && C1 == SC_C;
}

size_t stem_composite_ws_bytes(int B) { return sc_layout(B).end; }

int launch_stem_composite(const void* g, int ldg, const void* x, int ldx, int B, int H, int W, const void* w1t, float reg, const float* w0,
                          float* dw0, int ldw, float* db0, void* ws, hipStream_t s) {
    const ScLayout l = sc_layout(B);
    char* base = (char*)ws;
    float* ps = (float*)(base + l.ps);
    float* pb = (float*)(base + l.pb);
    double* sf = (double*)(base + l.sf);
    double* rf = (double*)(base + l.rf);
    int nblk = 0;
    int err = launch_stem_corr_mfma(g, ldg, B, H, W, x, ldx, ps, SC_CORR_BLOCKS, &nblk, s);
    if (err) return err;
    hipLaunchKernelGGL(stem_frame_kernel, dim3(B, 4), dim3(512), 0, s, (const __bf16*)g, ldg, (const __bf16*)x, ldx, H, W, pb);
    constexpr int NOUT = SC_SROWS * SC_C + SC_LINES * SC_BSLOTS * SC_C;
    hipLaunchKernelGGL(stem_finalize_kernel, dim3((NOUT + 15) / 16), dim3(256), 0, s, ps, nblk, pb, B, sf, rf);
    hipLaunchKernelGGL(stem_contract_kernel, dim3(SC_C), dim3(64), 0, s, sf, rf, (const __bf16*)w1t, reg, w0, dw0, ldw, db0);
    return (int)hipGetLastError();
}
