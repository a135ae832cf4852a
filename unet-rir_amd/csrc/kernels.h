// kernels.h - internal declarations shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "../../include/unetrir.h"

#define UNETRIR_MAX_TAPS 36

// Kernel-selection switches (include/unetrir.h: unetrir_config): read once from the environment, replaceable through
// unetrir_set_config (tests, A/B scripts).  No other environment variable is read by the library.
const unetrir_config& unetrir_cfg();

// Timing ablations (results invalid: a kernel with a stage switched off) exist only in the separate build that
// scripts/ use (build.py --ablations -> libunetrir_abl.so, -DUNETRIR_ABLATIONS); in the product library UNETRIR_ABL(...) is
// a compile-time false and the code behind it is not emitted.
#ifdef UNETRIR_ABLATIONS
extern int g_unetrir_abl;                 // set through unetrir_abl_set()
#define UNETRIR_ABL_HOST() g_unetrir_abl
#define UNETRIR_ABL(v, bit) (((v) & (bit)) != 0)
#else
#define UNETRIR_ABL_HOST() 0
#define UNETRIR_ABL(v, bit) false
#endif

// Geometry of one implicit-GEMM launch.  The iteration grid is B x PH x PW "tile pixels" p;
// the input pixel of tap t is (py*SI + dy_t, px*SI + dx_t) and the output pixel is
// (py*SO + ooy, px*SO + oox).  tap[t] packs dy (int8) | dx (int8) << 8 | weight-tap index << 16.
struct IgemmGeom {
    int B, PH, PW;
    int IH, IW, C, ldi;
    int OH, OW, N, ldo;
    int SI, SO, ooy, oox;
    int ntaps, wtaps;
    uint32_t tap[UNETRIR_MAX_TAPS];
};

struct IgemmArgs {
    IgemmGeom g;
    const float* in;
    const float* w;        // [N][wtaps][C]
    const float* bias;     // nullable
    const float* addend;   // nullable, indexed like out with ldadd
    int ldadd;
    float* out;
    int ksplit;            // > 1: blockIdx.y owns a K slice and writes raw partial sums to part[slice][pixel][N]
    float* part;
};

struct WgradArgs {
    IgemmGeom g;           // uses B,PH,PW (= dy grid), IH,IW,C,ldi (x), N, SI, taps
    const float* x;
    const float* dy;
    int lddy;
    float* part;           // [nsplit][N][wtaps*C]
    long long chunks_per_split;
};

int launch_igemm_fwd(const IgemmArgs& a, hipStream_t s);                                                              // igemm.hip
int launch_transpose_weight(const float* w, float* wt, int N, int T, int C, hipStream_t s);                          // weights.hip
int launch_splitk_reduce(const float* part, int nsplit, size_t n, float* out, float reg, const float* w, hipStream_t s);   // splitk_reduce.hip

// ---- weight gradients.  Every kernel below writes fp32 partial slabs [slab][N][taps][C] (grid.y = slab) that a fixed-order split-K
// reduction sums - or, with one slab and no l2 term, dw itself.  Which kernel serves a layer, how it splits K and what becomes of the
// slabs is decided in ONE place, plan_wgrad / run_wgrad (api.hip); the launchers only launch the partial-sum kernel into `part` with
// the plan's numbers.
// Patch shapes (output pixels, rows x columns) in which the patch-walking kernels walk K; plan_wgrad splits K into whole patches.
#define WG_TPW 8                  // wgrad3x3_kernel (fp32) and wgrad3x3_bf16_kernel (bf16 3x3 and 1x1): 8 columns; rows:
#define WG_F32_TPH_S1 4           //   fp32 3x3, stride 1 / 2
#define WG_F32_TPH_S2 2
#define WG_BF16_TPH_S1 8          //   bf16 3x3: one barrier pair and one global round trip are amortised over TPH*8 pixels of MFMA work
#define WG_BF16_TPH_S2 4
#define WG_1X1_TPH_S1 16          //   bf16 1x1: one tap of MFMA work per 16-pixel K step, so taller patches
#define WG_1X1_TPH_S2 8           //     (stride 2: the x patch is (2 TPH - 1) x 15 pixels)
#define WG_ROW_TPH 8              // wgrad3x3g and wgrad3x3r: 8 x 16
#define WG_ROW_TPW 16
int wgrad_plan(const IgemmGeom& g, int* nsplit, long long* chunks_per_split);       // the tap-table kernel's own split
int launch_igemm_wgrad(const WgradArgs& a, int nsplit, hipStream_t s, int bf16_operands);

// 3x3 weight gradient with a halo-staged x patch (wgrad3x3.hip: fp32 here, the bf16 twin Wgrad3ArgsH / launch_wgrad3x3_bf16 below)
struct Wgrad3Args {
    const float* x; int ldx; int IH, IW;      // layer input  [B,IH,IW,C]
    const float* dy; int lddy; int OH, OW;    // output grad  [B,OH,OW,N]
    int B, C, N;
    int pad_t, pad_l;                         // TF 'same' pad_before per axis
    float* part;                              // [nsplit][N][9][C]
    int patches_per_split, npy, npx;
};
int launch_wgrad3x3(const Wgrad3Args& a, int stride, int nslabs, hipStream_t s);

// ---- bf16-storage variants: activations / weight work copies bf16, accumulate fp32.  Tap-table forward kernel: igemm_bf16.hip ----
struct IgemmArgsH {
    IgemmGeom g;
    const __bf16* in;
    const __bf16* w;       // [N][wtaps][C] bf16
    const float* bias;     // nullable, fp32
    const __bf16* addend;  // nullable
    int ldadd;
    __bf16* out;
    float* colstat;        // nullable: [pixel tile][N][2] per-channel (sum, sum of squares) of the stored bf16 output, one row per
                           // 128-pixel tile of the launch (row = tile index); requires addend == nullptr
};
// The tap-table launch for small problems (igemm2_bf16.hip): pixel-tile height it would use for an iteration grid of M pixels, N
// output channels and ncls launches sharing one grid (1, or the 4 parity classes of a stride-2 transposed layer); 0 = not taken
// (switch off / too large): the general kernel with 128-pixel tiles.
int igemm_bf16_tile_m(long long M, int N, int ncls);
int launch_igemm2_fwd_bf16(const IgemmArgsH* a, int ncls, hipStream_t s);
// rows of column statistics one tap-table launch writes (= its pixel tiles)
inline long long igemm_colstat_rows(long long M, int N, int ncls = 1) {
    const int bm = igemm_bf16_tile_m(M, N, ncls);
    return (M + (bm ? bm : 128) - 1) / (bm ? bm : 128);
}
struct Wgrad3ArgsH {
    const __bf16* x; int ldx; int IH, IW;
    const __bf16* dy; int lddy; int OH, OW;
    int B, C, N;
    int pad_t, pad_l;
    float* part;                              // fp32 partial slabs [nsplit][N][9][C]
    int patches_per_split, npy, npx;
    int xcd_remap;                            // wgrad3x3g: workgroups that share x / dy patches (one split, all tiles) on one XCD
};
int launch_igemm_fwd_bf16(const IgemmArgsH& a, hipStream_t s);
int launch_igemm_fwd_bf16_x4(const IgemmArgsH* a, hipStream_t s);
int launch_wgrad3x3_bf16(const Wgrad3ArgsH& a, int stride, int nslabs, hipStream_t s);     // the generic patch kernel (wgrad3x3.hip)
int launch_wgrad1x1_bf16(const Wgrad3ArgsH& a, int stride, int nslabs, hipStream_t s);
// Shape rules of the bf16 3x3 weight-gradient kernels.  with_ld = false (the workspace query, which has no pixel strides): the limits
// that depend on ldx / lddy are left out.
bool wgrad3x3g_applies(const Wgrad3ArgsH& a, bool with_ld);        // stride 1: LDS-DMA kernel with register reuse of patch rows
int launch_wgrad3x3g_bf16(Wgrad3ArgsH a, int ns, hipStream_t s);
bool wgrad3x3r_applies(const Wgrad3ArgsH& a);                     // stride 1: register-staged twin of wgrad3x3g
int launch_wgrad3x3r_bf16(const Wgrad3ArgsH& a, int nslabs, hipStream_t s);
bool wgrad3x3d_applies(const Wgrad3ArgsH& a, bool with_ld);        // stride 2, even sizes: LDS-DMA kernel with the de-interleaved x patch
void wgrad3x3d_plan(int B, int OH, int OW, int N, int C, int* nsplit, int* per_split, int* npy, int* npx);     // its own split
int launch_wgrad3x3d_bf16(Wgrad3ArgsH a, int nslabs, hipStream_t s);
// bf16 work copies of the fp32 masters (weights.hip)
int launch_cast_weight(const float* w, void* o, int N, int T, int C, int Cp, hipStream_t s);
int launch_cast_weights_batched(const unetrir_cast_desc* desc_dev, int n_layers, hipStream_t s);
int launch_transpose_cast_weight(const float* w, void* wt, int N, int T, int C, int Np, hipStream_t s);

// 3x3 stride-1 conv / data gradient with the halo patch staged once in LDS (conv3x3.hip); T = float or __bf16
struct Conv3Args {
    const void* in; int ldi;
    const void* w;            // [N][9][C], element type T
    const float* bias;        // nullable
    const void* addend; int ldadd;
    void* out; int ldo;
    int B, H, W, C, N;
    int flip;                 // 0: forward (weight tap t at offset t); 1: data gradient (weight tap 8-t at offset t)
    const void* wpk;          // nullable; conv3x3d only: the packed copy of w (unetrir_conv3x3s2_packed_elems)
    float* colstat;           // nullable; the kernels with a *_colstat_rows function only: [row][N][2] per-channel (sum, sum of squares)
                              // of the stored output, that many rows (conv3x3g / h / r: one per 16 x 32 pixel tile, row =
                              // (img * tiles_y + ty) * tiles_x + tx)
};
// Which of the kernels below serves a launch - and that includes the kernel-selection switches they belong to - is decided in ONE
// place, plan_conv (api.hip), as plan_wgrad decides it for the weight gradients above.  All *_applies predicates are shape rules only.
int launch_conv3x3(const Conv3Args& a, int bf16, hipStream_t s);     // the generic patch-staged kernel (conv3x3.hip); no statistics
long long conv3x3r_colstat_rows(const Conv3Args& a);
int launch_conv3x3r_bf16(const Conv3Args& a, hipStream_t s);
bool head_mfma_applies(int W, int C);
int launch_head_fwd_mfma(const void* x, int ldx, int B, int H, int W, int C, const float* w, const float* bias, float* y, int ldy, hipStream_t s);
int launch_head_wgrad_mfma(const void* x, int ldx, int B, int H, int W, int C, const void* dy, int lddy, float* part, int max_blocks,
                           int* nblk_out, hipStream_t s);
// the stem's gradients through the next 3x3 layer (stem_composite.hip); its 5 x 5 correlation is head_wgrad_mfma_kernel<5, true>
int launch_stem_corr_mfma(const void* x, int ldx, int B, int H, int W, const void* dy, int lddy, float* part, int max_blocks,
                          int* nblk_out, hipStream_t s);
bool stem_composite_applies(int B, int H, int W, int C0, int C1);
size_t stem_composite_ws_bytes(int B);
int launch_stem_composite(const void* g, int ldg, const void* x, int ldx, int B, int H, int W, const void* w1t, float reg, const float* w0,
                          float* dw0, int ldw, float* db0, void* ws, hipStream_t s);
bool head_dgrad_mfma_applies(int W, int C);
int launch_head_dgrad_mfma(const void* dy, int lddy, int B, int H, int W, const float* w, int C, void* dx, int lddx, hipStream_t s);
bool upconv3x3g_applies(const Conv3Args& a);
bool upconv3x3q_applies(const Conv3Args& a);        // upconv3x3g's layers with >= 512 tiles: persistent form
int launch_upconv3x3q_bf16(const Conv3Args& a, hipStream_t s);
int launch_upconv3x3g_bf16(const Conv3Args& a, hipStream_t s);
bool conv3x3g_applies(const Conv3Args& a);
bool conv3x3g_pair_applies(const Conv3Args& a, bool any_size);     // images <= 16 pixels wide: two images per tile
long long conv3x3g_colstat_rows(const Conv3Args& a, bool pair);
int launch_conv3x3g_bf16(const Conv3Args& a, bool pair, hipStream_t s);
bool stem3x3_applies(const Conv3Args& a);
int launch_stem3x3_bf16(const Conv3Args& a, hipStream_t s);
bool conv3x3s_applies(const Conv3Args& a);          // 64 -> 64 channels: strip kernel with the whole 3x3 kernel resident in LDS
long long conv3x3s_colstat_rows(const Conv3Args& a);
int launch_conv3x3s_bf16(const Conv3Args& a, hipStream_t s);
// Run-time tile tickets of the persistent kernels (tile_tickets.h has the slot layout and the protocol): one slot per stream,
// zero between launches; nullptr with dyn_tiles = 0 or when more than 128 streams are in use - the kernels then keep their
// fixed assignment.
unsigned* sched_slot(hipStream_t s);
bool conv3x3p_applies(const Conv3Args& a);          // conv3x3g's layers with >= 512 tiles: persistent form, continuous K loop across tiles
long long conv3x3p_colstat_rows(const Conv3Args& a);
int launch_conv3x3p_bf16(const Conv3Args& a, hipStream_t s);
bool conv3x3d_applies(const Conv3Args& a);          // 3x3 stride 2, forward form (H, W = input size): persistent LDS-DMA kernel
int launch_conv3x3d_bf16(const Conv3Args& a, hipStream_t s);
bool conv3x3h_applies(const Conv3Args& a);
long long conv3x3h_colstat_rows(const Conv3Args& a);
int launch_conv3x3h_bf16(const Conv3Args& a, hipStream_t s);
// Dense on a small batch (dense.hip); the row-slab reduction both directions end with is in splitk_reduce.hip
int launch_dense_fwd(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B, int K, int N,
                     void* ws, size_t ws_bytes, hipStream_t s);
size_t dense_fwd_ws_bytes(int B, int K, int N);
int launch_splitk_rows_reduce(const float* part, int nsplit, long long M, int N, const float* bias, float* y, int ldy, hipStream_t s);
bool dense_dgrad_applies(int B, int K, int N);
size_t dense_dgrad_ws_bytes(int B, int K, int N);
int launch_dense_dgrad(const float* dy, int lddy, const float* w, float* dx, int lddx, int B, int K, int N, void* ws, size_t ws_bytes,
                       hipStream_t s);
int launch_upconv3x3(const Conv3Args& a, int bf16, hipStream_t s);   // the generic strided data-gradient kernel (upconv3x3.hip)

// 1x1 convolutions (pw1x1.hip): out[opix(p)][n] = sum_c in[ipix(p)][c] w[n][c] + bias[n] (+ addend) over the iteration grid
// B x PH x PW; ipix = (b, py SI, px SI) of the IH x IW input grid, opix = (b, py SO, px SO) of the OH x OW output grid; fill
// (SO = 2): the three other pixels of each 2 x 2 output cell are written with bias (+ addend).
struct PwArgs {
    const __bf16* in; int ldi; int IH, IW;
    const __bf16* w;                 // [N][C], C contiguous
    const float* bias;               // nullable
    const __bf16* addend; int ldadd; // nullable; indexed like out (may be out itself)
    __bf16* out; int ldo; int OH, OW;
    int B, PH, PW, SI, SO, fill;
    int C, N;
    float* colstat;                  // nullable: [pw1x1_colstat_rows][N][2]; not together with an addend
};
bool pw1x1_applies(const PwArgs& a);
long long pw1x1_colstat_rows(const PwArgs& a);
int launch_pw1x1_bf16(const PwArgs& a, hipStream_t s);   // H, W = coarse (input) grid; output 2H x 2W

// 2x2 stride-2 layers on even sizes (conv2x2.hip).  The iteration grid is the COARSE grid B x PH x PW, the fine grid is
// B x 2 PH x 2 PW; tap t = 2 kh + kw.  Gather form: out[coarse p][n] = sum_t sum_c in[fine(p, t)][c] w[n][t][c] + bias[n]
// (+ addend); scatter form: out[fine(p, t)][n] = sum_c in[coarse p][c] w[n][t][c] + bias[n] (+ addend).
struct C22Args {
    const __bf16* in; int ldi;
    const __bf16* w;                 // [N][4][C], C contiguous
    const float* bias;               // nullable
    const __bf16* addend; int ldadd; // nullable; indexed like out (may be out itself)
    __bf16* out; int ldo;
    int B, PH, PW;
    int C, N;
    int cshift;                      // log2(C): filled by the launcher
};
bool conv2x2s2_gemm_applies(const C22Args& a, bool scatter);
int launch_conv2x2s2_gemm_bf16(C22Args a, bool scatter, hipStream_t s);
// weight gradient: part[slab][S][4][L] = sum over the slab's coarse pixels p of small[p][s] * large[fine(p, t)][l]
struct C22WgradArgs {
    const __bf16* small; int lds; int S;      // the coarse-grid tensor [B,PH,PW,S]
    const __bf16* large; int ldl; int L;      // the fine-grid tensor [B,2PH,2PW,L]
    int B, PH, PW;
    float* part;
    long long blocks_per_split;               // 32-pixel K blocks per slab
};
bool conv2x2s2_wgrad_applies(const C22WgradArgs& a);
void conv2x2s2_wgrad_plan(int B, int PH, int PW, int S, int L, int* nslabs, long long* blocks_per_split);
int launch_conv2x2s2_wgrad_bf16(const C22WgradArgs& a, int nslabs, hipStream_t s);

// splitmix64 finaliser: the hash of the counter-based generators - dropout_mask_kernel (elementwise.hip) and normal_kernel (vae.hip,
// which also holds the sampling / KL kernels of the variational autoencoder; their entry points are in include/unetrir.h)
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// the row fetch of the scoring kernels (evalmetrics.hip, acoustics.hip):
// four consecutive floats from element i of a row of n: one 128-bit load when allowed, bounds-checked scalars otherwise (zeros
// past the end; the callers mask those lanes out)
__device__ __forceinline__ float4 ld_group(const float* __restrict__ p, long long i, long long n, bool vec) {
    if (vec && i + 4 <= n) return *reinterpret_cast<const float4*>(p + i);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i + 0 < n) v.x = p[i + 0];
    if (i + 1 < n) v.y = p[i + 1];
    if (i + 2 < n) v.z = p[i + 2];
    if (i + 3 < n) v.w = p[i + 3];
    return v;
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// scoring of generated impulse responses (evalmetrics.hip); arguments are validated by the entry points in api.hip
int launch_eval_metrics(const float* pred, const float* target, const float* phase_ref, int B, int H, int W, const float* wav_pred,
                        const float* wav_true, int T, int n50, double* out, hipStream_t s);
int launch_eval_accumulate(const double* out, const int* group, int B, int G, double* acc, hipStream_t s);

// room-acoustic figures of impulse responses (acoustics.hip); arguments are validated by the entry points in api.hip
int launch_acoustic_figures(const float* wav_a, const float* wav_b, int B, int T, int n_pre, int n_dir, int n_early, double fs,
                            double* fig, hipStream_t s);
int launch_acoustic_accumulate(const double* fig, const int* group, int B, int G, double fs, double* err, double* acc, hipStream_t s);
