// api.hip - the C ABI (include/unetrir.h): TF padding='same' geometry -> tap tables -> launches.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>
#include "kernels.h"

// ---- kernel-selection switches: the only environment variables the library reads, once.  The switches in effect are an IMMUTABLE
//      snapshot behind one atomic pointer: unetrir_set_config publishes a new snapshot (release), every reader takes the pointer
//      (acquire) - a launch being issued on another thread sees the old values or the new ones, never a half-written struct.
//      Replaced snapshots are kept (a few hundred bytes per call of a function only tests and A/B scripts use): a reader may still
//      hold one.
namespace {
int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
const unetrir_config* load_config() {
    unetrir_config* c = new unetrir_config;
    c->conv3x3 = env_int("UNETRIR_CONV3X3", 1);
    c->conv3x3g = env_int("UNETRIR_CONV3X3G", 1);
    c->conv3x3g_pair = env_int("UNETRIR_CONV3X3G_PAIR", 1);
    c->conv3x3h = env_int("UNETRIR_CONV3X3H", 1);
    c->conv3x3s = env_int("UNETRIR_CONV3X3S", 1);
    c->conv3x3r = env_int("UNETRIR_CONV3X3R", 1);
    c->stem = env_int("UNETRIR_STEM", 1);
    c->upconv3x3g = env_int("UNETRIR_UPCONV3X3G", 1);
    c->wgrad3x3g = env_int("UNETRIR_WGRAD3X3G", 1);
    c->wgrad3x3r = env_int("UNETRIR_WGRAD3X3R", 1);
    c->wgrad3x3d = env_int("UNETRIR_WGRAD3X3D", 1);
    c->conv3x3d = env_int("UNETRIR_CONV3X3D", 1);
    c->conv3x3p = env_int("UNETRIR_CONV3X3P", 1);
    c->upconv3x3q = env_int("UNETRIR_UPCONV3X3Q", 1);
    c->dyn_tiles = env_int("UNETRIR_DYN_TILES", 1);
    c->head_mfma = env_int("UNETRIR_HEAD_MFMA", 1);
    c->pw1x1 = env_int("UNETRIR_PW1X1", 1);
    c->igemm2 = env_int("UNETRIR_IGEMM2", 1);
    return c;
}
std::atomic<const unetrir_config*>& config_slot() {
    static std::atomic<const unetrir_config*> p{load_config()};
    return p;
}
}  // namespace
const unetrir_config& unetrir_cfg() { return *config_slot().load(std::memory_order_acquire); }
extern "C" int unetrir_get_config(unetrir_config* out) {
    if (!out) return UNETRIR_EINVAL;
    *out = unetrir_cfg();
    return 0;
}
extern "C" int unetrir_set_config(const unetrir_config* in) {
    if (!in) return UNETRIR_EINVAL;
    config_slot().store(new unetrir_config(*in), std::memory_order_release);
    return 0;
}

#ifdef UNETRIR_ABLATIONS
int g_unetrir_abl = 0;
extern "C" int unetrir_abl_set(int v) { g_unetrir_abl = v; return 0; }
// A stand-in for a communication kernel beside the step (ablation build only): n workgroups that hold `lds` bytes of LDS and
// spin for `cycles` clock cycles - CUs on which a 158 KB persistent workgroup cannot be placed meanwhile.
__global__ void abl_hog_kernel(long long cycles, int lds, unsigned* sink) {
    extern __shared__ unsigned hog_smem[];
    if (lds > 0) hog_smem[threadIdx.x] = threadIdx.x;
    const long long t0 = wall_clock64();
    unsigned acc = 0;
    while (wall_clock64() - t0 < cycles) acc += hog_smem[(threadIdx.x + acc) & 63];
    if (acc == 0xFFFFFFFFu) *sink = acc;
}
extern "C" int unetrir_abl_hog(int n, long long cycles, int lds, void* sink, void* stream) {
    hipLaunchKernelGGL(abl_hog_kernel, dim3(n), dim3(256), (size_t)lds, (hipStream_t)stream, cycles, lds, (unsigned*)sink);
    return (int)hipGetLastError();
}
#endif

// ---- per-stream ticket slots: a static device array, one slot per (device, stream) in use, for the tile tickets of the
//      persistent convolution kernels (tile_tickets.h has the layout of a slot and the protocol).  Zero between launches: every
//      kernel that uses a slot leaves it cleared.
__device__ unsigned g_sched_slots[128][80];
// A __device__ symbol has one instance PER DEVICE: the table below is keyed by the device that is current at the launch (the
// reference's own process shape is one process driving several GPUs, main_training.py:56), and a slot by (device, stream).
// More than 16 devices or 128 streams in use on one device: no slot (-1) - the callers then take their slot-free path.
// The table is append-only, so the lookup every persistent-kernel launch performs takes NO lock: `used` is published with release
// after the owner entry is written; only a miss (a stream's first launch, a device's first use) takes the mutex.
namespace {
struct SlotTable { std::atomic<unsigned*> sched{nullptr}; hipStream_t owner[128]; std::atomic<int> used{0}; };
constexpr int MAX_DEV = 16;
std::mutex g_slot_mu;
SlotTable g_slot_tab[MAX_DEV];

// index of the slot of (current device, s), or -1; *base receives the device's slot array
int slot_index(hipStream_t s, unsigned** base) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEV) return -1;
    SlotTable& d = g_slot_tab[dev];
    unsigned* sched = d.sched.load(std::memory_order_acquire);
    if (sched) {
        const int n = d.used.load(std::memory_order_acquire);
        for (int i = 0; i < n; ++i) if (d.owner[i] == s) { *base = sched; return i; }
    }
    std::lock_guard<std::mutex> lk(g_slot_mu);           // miss: first launch of this stream (or first use of this device)
    sched = d.sched.load(std::memory_order_relaxed);
    if (!sched) {
        void* p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_sched_slots)) != hipSuccess) return -1;              // resolve on the current device
        // zeroed once, synchronously, on first use of this device (a stream that is being captured into a HIP graph refuses the
        // call: no slot then, and nothing is cached - the engines call unetrir_reset_tile_tickets() when they are built)
        if (hipMemset(p, 0, sizeof(unsigned) * 128 * 80) != hipSuccess) {
            (void)hipGetLastError();
            return -1;
        }
        sched = (unsigned*)p;
        d.sched.store(sched, std::memory_order_release);
    }
    *base = sched;
    const int n = d.used.load(std::memory_order_relaxed);
    for (int i = 0; i < n; ++i) if (d.owner[i] == s) return i;      // another thread appended it meanwhile
    if (n == 128) return -1;
    d.owner[n] = s;
    d.used.store(n + 1, std::memory_order_release);
    return n;
}
}  // namespace

unsigned* sched_slot(hipStream_t s) {
    if (!unetrir_cfg().dyn_tiles) return nullptr;
    unsigned* base = nullptr;
    const int i = slot_index(s, &base);
    return i < 0 ? nullptr : base + i * 80;
}

// Host-side reset of every ticket slot of the current device (after toggling dyn_tiles, or after a launch failed): call with the
// device idle.  The kernels clear their own slot at the end of every launch, so a healthy run never needs it.
extern "C" int unetrir_reset_tile_tickets(void) {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_sched_slots)) != hipSuccess) return UNETRIR_EINVAL;
    return (int)hipMemset(p, 0, sizeof(unsigned) * 128 * 80);
}

namespace {

struct Same { int out, before; };
// tf.nn.convolution padding='same': out = ceil(in/s), pad_total = max((out-1)*s + k - in, 0),
// pad_before = pad_total / 2 (dl_models/u_net.py:269-276 relies on it for the strided convs).
inline Same same_geom(int n_in, int k, int s) {
    Same r;
    r.out = (n_in + s - 1) / s;
    int total = (r.out - 1) * s + k - n_in;
    if (total < 0) total = 0;
    r.before = total / 2;
    return r;
}

inline uint32_t pack_tap(int dy, int dx, int widx) {
    return (uint32_t)(uint8_t)(int8_t)dy | ((uint32_t)(uint8_t)(int8_t)dx << 8) | ((uint32_t)widx << 16);
}

inline bool geom_ok(const unetrir_conv_geom* g) {
    return g && g->B > 0 && g->H > 0 && g->W > 0 && g->Cin > 0 && g->Cout > 0 && g->k >= 1 && g->k <= 6 &&
           (g->stride == 1 || g->stride == 2);
}

// ---- profiling (the only process-global state in the library; off by default) ----
struct ProfRec { int fam, tag; hipEvent_t e0, e1; double flops; };
std::mutex g_prof_mu;
bool g_prof_on = false;
unsigned g_prof_mask = ~0u;       // families that get brackets (unetrir_prof_enable(2): forward convolutions only)
std::vector<ProfRec> g_prof;

struct ProfScope {
    bool on; ProfRec r; hipStream_t s;
    // tag: a second family the bracket is ALSO counted under (UNETRIR_FAM_DOMINANT: launches served by the dominant kernel), or -1
    ProfScope(int fam, double flops, hipStream_t st, int tag = -1) : on(g_prof_on && ((g_prof_mask >> fam) & 1u)), s(st) {
        if (!on) return;
        r.fam = fam; r.tag = tag; r.flops = flops;
        hipEventCreate(&r.e0); hipEventCreate(&r.e1);
        hipEventRecord(r.e0, s);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(r.e1, s);
        std::lock_guard<std::mutex> lk(g_prof_mu);
        g_prof.push_back(r);
    }
};

inline double conv_flops(const unetrir_conv_geom* g) {
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    return 2.0 * g->B * sy.out * sx.out * (double)g->Cout * g->Cin * g->k * g->k;
}
inline int conv_family(const unetrir_conv_geom* g, int fam) {
    return (g->Cin <= 8 || g->Cout <= 8) ? 5 : fam;     // zero-padded stem / head: not part of the MFMA roofline figure
}

// ---- the kernel plan: the ONE place that decides which kernel serves a forward, data-gradient or Conv2DTranspose-forward
//      convolution launch, and how many rows of fused column statistics that kernel writes.  The entry points below launch what it
//      chose, the query entry points (unetrir_conv2d_colstat_rows_bf16, unetrir_conv2d_transpose_colstat_rows_bf16,
//      unetrir_conv3x3_kernel_id_bf16) return its fields, and it is the only reader of the kernel-selection switches conv3x3,
//      conv3x3g, conv3x3g_pair, conv3x3h, conv3x3s, conv3x3r, stem, conv3x3p, conv3x3d, upconv3x3g, upconv3x3q and pw1x1 (the
//      kernels' *_applies predicates are shape rules).  The weight gradients have their own plan, plan_wgrad below.
enum class Kern { TAPTABLE, TAPTABLE_CLASSES, PATCH, STEM, CONV3X3G_PAIR, CONV3X3P, CONV3X3G, CONV3X3S, CONV3X3H, CONV3X3R, CONV3X3D,
                  UPCONV3X3, UPCONV3X3G, UPCONV3X3Q, PW1X1 };
struct ConvPlan {
    Kern kernel;
    long long colstat_rows;     // rows the kernel writes when the launch asks for statistics; 0: the *_colstat entry points refuse
};

// Direction of a launch.  FWD: Conv2D forward (also the Conv2DTranspose data gradient, on the adjoint geometry); DGRAD: Conv2D data
// gradient; TFWD: Conv2DTranspose forward = the data-gradient form on the adjoint geometry, with a bias.
enum Dir { FWD, DGRAD, TFWD };
// One launch: g is the geometry the kernels see (the adjoint one for the transposed layers); `in` is x (FWD) or dy (DGRAD, TFWD).
struct ConvCall {
    const unetrir_conv_geom* g; Dir dir;
    const void* in; int ldi; const void* w; const void* wpk; const float* bias; const void* addend; int ldadd; void* out; int ldo;
    float* colstat;
};

// share of the patch-staged kernels' 8 x 32 pixel tiles that an H x W image fills
inline double patch_util(int H, int W) { return (double)H * W / ((double)((H + 7) / 8 * 8) * ((W + 31) / 32 * 32)); }

// The Conv3Args of a 3x3 launch.  Stride 1: the forward kernels, data gradient = the same kernel with flipped taps.  Stride 2 forward:
// conv3x3d (H, W = input size; the packed weight copy only where it is defined).  Stride 2 data-gradient form: upconv3x3* on the dy grid.
Conv3Args conv3_args(const ConvCall& c) {
    const unetrir_conv_geom* g = c.g;
    const bool dg = c.dir != FWD;
    Conv3Args a{};
    a.in = c.in; a.ldi = c.ldi; a.w = c.w; a.bias = c.bias; a.addend = c.addend; a.ldadd = c.ldadd; a.out = c.out; a.ldo = c.ldo;
    a.colstat = c.colstat;
    a.B = g->B; a.H = g->H; a.W = g->W; a.C = dg ? g->Cout : g->Cin; a.N = dg ? g->Cin : g->Cout;
    if (g->stride == 1) {
        a.flip = dg ? 1 : UNETRIR_ABL(UNETRIR_ABL_HOST(), 256) ? 2 : 0;     // ablation build only: register-staged kernel without its stores
    } else if (dg) {
        a.H = same_geom(g->H, 3, 2).out; a.W = same_geom(g->W, 3, 2).out;
    } else {
        a.wpk = (g->Cin % 64 == 0 && g->Cout % 64 == 0) ? c.wpk : nullptr;
    }
    return a;
}

// 1x1 layers in bf16 storage: the register-streaming kernel (pw1x1.hip).  Forward form: gather at the convolution's stride;
// data-gradient form (also Conv2DTranspose forward): scatter at the stride, the other pixels of a 2 x 2 cell filled with bias
// (+ addend) - for k = 1 TF 'same' has no padding at either stride, so input pixel = stride * output pixel exactly.
PwArgs pw_args(const ConvCall& c) {
    const unetrir_conv_geom* g = c.g;
    const Same sy = same_geom(g->H, 1, g->stride), sx = same_geom(g->W, 1, g->stride);
    PwArgs a{};
    a.in = (const __bf16*)c.in; a.ldi = c.ldi; a.w = (const __bf16*)c.w; a.bias = c.bias; a.addend = (const __bf16*)c.addend;
    a.ldadd = c.ldadd; a.out = (__bf16*)c.out; a.ldo = c.ldo; a.colstat = c.colstat;
    a.B = g->B; a.PH = sy.out; a.PW = sx.out;
    if (c.dir == FWD) {
        a.IH = g->H; a.IW = g->W; a.OH = sy.out; a.OW = sx.out; a.SI = g->stride; a.SO = 1; a.C = g->Cin; a.N = g->Cout;
    } else {
        a.IH = sy.out; a.IW = sx.out; a.OH = g->H; a.OW = g->W; a.SI = 1; a.SO = g->stride; a.fill = g->stride == 2; a.C = g->Cout;
        a.N = g->Cin;
    }
    return a;
}

// rows of the tap-table kernel: one per pixel tile of its iteration grid (forward: the output grid; stride-1 data gradient: the input
// grid; stride-2 data-gradient form: the dy grid, four parity classes with a row range each)
long long taptable_rows(const unetrir_conv_geom* g, Dir dir) {
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    if (dir == FWD) return igemm_colstat_rows((long long)g->B * sy.out * sx.out, g->Cout);
    if (g->stride == 1) return igemm_colstat_rows((long long)g->B * g->H * g->W, g->Cin);
    return 4 * igemm_colstat_rows((long long)g->B * sy.out * sx.out, g->Cin, 4);
}

ConvPlan plan_conv(const ConvCall& c, bool bf16, bool stats) {
    const unetrir_config& cfg = unetrir_cfg();
    const unetrir_conv_geom* g = c.g;
    if (g->k == 3 && g->stride == 1) {
        const Conv3Args a = conv3_args(c);
        // patch-staged kernels where their tiles cover the image well; narrow images (the 16 x 16 level) would half-fill the 32-column
        // tiles: bf16 has a paired-image tile for them
        const bool pair = bf16 && cfg.conv3x3g_pair && conv3x3g_pair_applies(a, cfg.conv3x3g_pair == 2);
        if ((cfg.conv3x3 && patch_util(g->H, g->W) >= 0.7) || pair) {
            if (!bf16) return {Kern::PATCH, 0};
            if (cfg.stem && !stats && stem3x3_applies(a)) return {Kern::STEM, 0};         // first layer: 8 stored channels -> 64
            if (cfg.conv3x3g) {       // the pair, then the persistent form, then the plain LDS-DMA kernel
                if (pair) return {Kern::CONV3X3G_PAIR, conv3x3g_colstat_rows(a, true)};
                if (cfg.conv3x3p && conv3x3p_applies(a)) return {Kern::CONV3X3P, conv3x3p_colstat_rows(a)};
                if (conv3x3g_applies(a)) return {Kern::CONV3X3G, conv3x3g_colstat_rows(a, false)};
            }
            if (cfg.conv3x3s && conv3x3s_applies(a)) return {Kern::CONV3X3S, conv3x3s_colstat_rows(a)};
            if (cfg.conv3x3h && conv3x3h_applies(a)) return {Kern::CONV3X3H, conv3x3h_colstat_rows(a)};
            // the row-reuse kernel unless a timing ablation asks for the generic kernel's no-store variant
            if (cfg.conv3x3r && !(a.flip & 2)) return {Kern::CONV3X3R, conv3x3r_colstat_rows(a)};
            return {Kern::PATCH, 0};
        }
    }
    if (bf16 && g->k == 1 && cfg.pw1x1 && !(stats && c.addend) && pw1x1_applies(pw_args(c)))
        return {Kern::PW1X1, pw1x1_colstat_rows(pw_args(c))};
    // 3x3 stride 2 has no fused statistics in either direction: its own kernels write none, and the tap-table fallback is not offered
    if (g->stride == 1) return {Kern::TAPTABLE, taptable_rows(g, c.dir)};
    if (c.dir == FWD) {
        if (bf16 && g->k == 3 && cfg.conv3x3d && conv3x3d_applies(conv3_args(c))) return {Kern::CONV3X3D, 0};
        return {Kern::TAPTABLE, g->k == 3 ? 0 : taptable_rows(g, c.dir)};
    }
    // stride-2 data-gradient form.  3x3, even sizes (pad_before 0): all four output parity classes in one patch-staged launch; half-empty
    // tiles (16-wide coarse grids) stay on the four tap-table launches: measured 0.2 ms/step faster than this kernel there
    const Same sy = same_geom(g->H, g->k, 2), sx = same_geom(g->W, g->k, 2);
    if (g->k == 3 && sy.before == 0 && sx.before == 0 && g->H == 2 * sy.out && g->W == 2 * sx.out && patch_util(sy.out, sx.out) >= 0.7) {
        const Conv3Args a = conv3_args(c);
        if (bf16 && cfg.upconv3x3g && upconv3x3g_applies(a))
            return {cfg.upconv3x3q && upconv3x3q_applies(a) ? Kern::UPCONV3X3Q : Kern::UPCONV3X3G, 0};
        if (cfg.conv3x3) return {Kern::UPCONV3X3, 0};
    }
    // the four parity classes of the tap-table kernel: statistics for the Conv2DTranspose forward only
    return {Kern::TAPTABLE_CLASSES, c.dir == TFWD && g->k != 3 ? taptable_rows(g, c.dir) : 0};
}

// element-type policies: fp32 and bf16-storage variants share the tap-table construction
struct F32 {
    static constexpr int is_bf16 = 0;
    using T = float; using Args = IgemmArgs;
    static int launch(const Args& a, hipStream_t s) { return launch_igemm_fwd(a, s); }
    static int launch_classes(const Args* a, hipStream_t s) {
        for (int i = 0; i < 4; ++i) { const int err = launch_igemm_fwd(a[i], s); if (err) return err; }
        return 0;
    }
};
struct BF16 {
    static constexpr int is_bf16 = 1;
    using T = __bf16; using Args = IgemmArgsH;
    static int launch(const Args& a, hipStream_t s) { return launch_igemm_fwd_bf16(a, s); }
    static int launch_classes(const Args* a, hipStream_t s) {
        return launch_igemm_fwd_bf16_x4(a, s);          // the four parity classes share one grid
    }
};

// ---- the tap-table launches.  Forward: iteration grid = output grid.  Data-gradient form:
// dx[q][ci] = sum_t sum_co dy[p][co] * wt[ci][t][co]  with q = p*s + (k_t - pad_before)
template <class P>
int launch_taptable(const ConvCall& c, hipStream_t s) {
    const unetrir_conv_geom* g = c.g;
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    typename P::Args a{};
    a.g.B = g->B; a.g.wtaps = g->k * g->k; a.g.ntaps = g->k * g->k; a.g.SI = 1; a.g.SO = 1; a.g.ooy = 0; a.g.oox = 0;
    a.g.ldi = c.ldi; a.g.ldo = c.ldo;
    a.in = (const typename P::T*)c.in; a.w = (const typename P::T*)c.w; a.bias = c.bias; a.addend = (const typename P::T*)c.addend;
    a.ldadd = c.ldadd; a.out = (typename P::T*)c.out;
    if constexpr (P::is_bf16) a.colstat = c.colstat;      // one row of column statistics per pixel tile
    if (c.dir == FWD) {
        a.g.PH = sy.out; a.g.PW = sx.out; a.g.IH = g->H; a.g.IW = g->W; a.g.C = g->Cin;
        a.g.OH = sy.out; a.g.OW = sx.out; a.g.N = g->Cout; a.g.SI = g->stride;
        for (int kh = 0; kh < g->k; ++kh)
            for (int kw = 0; kw < g->k; ++kw)
                a.g.tap[kh * g->k + kw] = pack_tap(kh - sy.before, kw - sx.before, kh * g->k + kw);
        return P::launch(a, s);
    }
    a.g.IH = sy.out; a.g.IW = sx.out; a.g.C = g->Cout;
    a.g.OH = g->H; a.g.OW = g->W; a.g.N = g->Cin;
    if (g->stride == 1) {      // dgrad of a stride-1 conv = the same conv with flipped taps
        a.g.PH = g->H; a.g.PW = g->W;
        for (int kh = 0; kh < g->k; ++kh)
            for (int kw = 0; kw < g->k; ++kw)
                a.g.tap[kh * g->k + kw] = pack_tap(-(kh - sy.before), -(kw - sx.before), kh * g->k + kw);
        return P::launch(a, s);
    }
    // stride 2: one launch per output parity class (ay, ax); q = 2p' + a, p = p' + (a - off)/2
    a.g.PH = (g->H + 1) / 2; a.g.PW = (g->W + 1) / 2; a.g.SO = 2;
    typename P::Args cls[4];
    for (int ay = 0; ay < 2; ++ay)
        for (int ax = 0; ax < 2; ++ax) {
            int nt = 0;
            for (int kh = 0; kh < g->k; ++kh) {
                const int offy = kh - sy.before;
                if (((offy - ay) & 1) != 0) continue;
                for (int kw = 0; kw < g->k; ++kw) {
                    const int offx = kw - sx.before;
                    if (((offx - ax) & 1) != 0) continue;
                    a.g.tap[nt++] = pack_tap((ay - offy) / 2, (ax - offx) / 2, kh * g->k + kw);
                }
            }
            a.g.ntaps = nt; a.g.ooy = ay; a.g.oox = ax;
            if constexpr (P::is_bf16) {      // column statistics: the four classes write consecutive row ranges
                if (c.colstat) a.colstat = c.colstat + (size_t)(ay * 2 + ax) * igemm_colstat_rows((long long)g->B * a.g.PH * a.g.PW, g->Cin, 4) * g->Cin * 2;
            }
            cls[ay * 2 + ax] = a;
        }
    return P::launch_classes(cls, s);       // bf16: the four classes share one grid
}

template <class P>
int launch_planned(const ConvCall& c, Kern k, hipStream_t s) {
    switch (k) {
        case Kern::TAPTABLE: case Kern::TAPTABLE_CLASSES: return launch_taptable<P>(c, s);
        case Kern::PATCH: return launch_conv3x3(conv3_args(c), P::is_bf16, s);
        case Kern::STEM: return launch_stem3x3_bf16(conv3_args(c), s);
        case Kern::CONV3X3G_PAIR: return launch_conv3x3g_bf16(conv3_args(c), true, s);
        case Kern::CONV3X3P: return launch_conv3x3p_bf16(conv3_args(c), s);
        case Kern::CONV3X3G: return launch_conv3x3g_bf16(conv3_args(c), false, s);
        case Kern::CONV3X3S: return launch_conv3x3s_bf16(conv3_args(c), s);
        case Kern::CONV3X3H: return launch_conv3x3h_bf16(conv3_args(c), s);
        case Kern::CONV3X3R: return launch_conv3x3r_bf16(conv3_args(c), s);
        case Kern::CONV3X3D: return launch_conv3x3d_bf16(conv3_args(c), s);
        case Kern::UPCONV3X3: return launch_upconv3x3(conv3_args(c), P::is_bf16, s);
        case Kern::UPCONV3X3G: return launch_upconv3x3g_bf16(conv3_args(c), s);
        case Kern::UPCONV3X3Q: return launch_upconv3x3q_bf16(conv3_args(c), s);
        case Kern::PW1X1: return launch_pw1x1_bf16(pw_args(c), s);
    }
    return UNETRIR_EINVAL;
}

// Plan and launch.  With a statistics buffer the plan must offer statistics (else UNETRIR_EINVAL).  dominant: profile the launch under
// UNETRIR_FAM_DOMINANT as well when the plan picked conv3x3p (the dominant kernel of the bf16 step).
template <class P>
int run_conv(const ConvCall& c, int fam, double flops, hipStream_t s, bool dominant = false) {
    const ConvPlan p = plan_conv(c, P::is_bf16, c.colstat != nullptr);
    if (c.colstat && p.colstat_rows == 0) return UNETRIR_EINVAL;
    ProfScope ps(fam, flops, s, dominant && p.kernel == Kern::CONV3X3P ? UNETRIR_FAM_DOMINANT : -1);
    return launch_planned<P>(c, p.kernel, s);
}

// what the query entry points describe: a bf16 launch with aligned buffers, no addend, output rows as wide as the output channels
ConvPlan plan_query(const unetrir_conv_geom* g, Dir dir, int ld_in, bool stats) {
    const ConvCall c{g, dir, nullptr, ld_in, nullptr, nullptr, nullptr, nullptr, 0, nullptr, dir == FWD ? g->Cout : g->Cin, nullptr};
    return plan_conv(c, true, stats);
}

// ---- the weight-gradient plan: the ONE place that decides which kernel serves a weight gradient and how it splits K, and the only
//      reader of the switches wgrad3x3g, wgrad3x3r and wgrad3x3d.  run_wgrad launches what it chose; the workspace query sizes every
//      plan it could choose.
enum class WgKern { TAPTABLE, PATCH, PATCH1X1, WGRAD3X3G, WGRAD3X3R, WGRAD3X3D };
struct WgradPlan {
    WgKern kernel;
    int nslabs;              // fp32 partial slabs the kernel writes (grid.y); 1 and no l2 term: dw itself
    long long per_split;     // K per slice: patches (patch kernels) or 32-pixel chunks (tap-table kernel)
    int npy, npx;            // patch grid of one image (patch kernels)
};

void wgrad_args(const unetrir_conv_geom* g, int ldx, int lddy, WgradArgs* a) {
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    a->g.B = g->B; a->g.PH = sy.out; a->g.PW = sx.out;
    a->g.IH = g->H; a->g.IW = g->W; a->g.C = g->Cin; a->g.ldi = ldx;
    a->g.N = g->Cout; a->g.SI = g->stride;
    a->g.ntaps = g->k * g->k; a->g.wtaps = g->k * g->k;
    for (int kh = 0; kh < g->k; ++kh)
        for (int kw = 0; kw < g->k; ++kw)
            a->g.tap[kh * g->k + kw] = pack_tap(kh - sy.before, kw - sx.before, kh * g->k + kw);
    a->lddy = lddy;
}

// the Wgrad3Args / Wgrad3ArgsH of a patch-kernel launch; part and the split are the caller's
template <class A>
A wgrad3_args(const unetrir_conv_geom* g, const void* x, int ldx, const void* dy, int lddy) {
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    A a{};
    a.x = (decltype(a.x))x; a.ldx = ldx; a.IH = g->H; a.IW = g->W;
    a.dy = (decltype(a.dy))dy; a.lddy = lddy; a.OH = sy.out; a.OW = sx.out;
    a.B = g->B; a.C = g->Cin; a.N = g->Cout;
    a.pad_t = sy.before; a.pad_l = sx.before;
    return a;
}

// The split of the patch kernels but wgrad3x3d: tph x tpw patches, about 512 workgroups over the 64 x 64 (N, C) tiles, at least 4
// patches per slice.
WgradPlan plan_patch(WgKern kernel, int tph, int tpw, const unetrir_conv_geom* g) {
    const Same sy = same_geom(g->H, g->k, g->stride), sx = same_geom(g->W, g->k, g->stride);
    WgradPlan p{kernel};
    p.npy = (sy.out + tph - 1) / tph;
    p.npx = (sx.out + tpw - 1) / tpw;
    const long long G = (long long)g->B * p.npy * p.npx;
    const long long tiles = (long long)((g->Cout + 63) / 64) * ((g->Cin + 63) / 64);
    long long want = (512 + tiles - 1) / tiles;
    long long maxs = (G + 3) / 4;
    if (maxs < 1) maxs = 1;
    if (want > maxs) want = maxs;
    if (want < 1) want = 1;
    p.per_split = (G + want - 1) / want;
    p.nslabs = (int)((G + p.per_split - 1) / p.per_split);
    return p;
}
// wgrad3x3g: two split-K slices per workgroup share one slab
WgradPlan plan_wgrad3x3g(const unetrir_conv_geom* g) {
    WgradPlan p = plan_patch(WgKern::WGRAD3X3G, WG_ROW_TPH, WG_ROW_TPW, g);
    p.nslabs = (p.nslabs + 1) / 2;
    return p;
}
WgradPlan plan_wgrad3x3d(const unetrir_conv_geom* g) {
    const Same sy = same_geom(g->H, 3, 2), sx = same_geom(g->W, 3, 2);
    WgradPlan p{WgKern::WGRAD3X3D};
    int per;
    wgrad3x3d_plan(g->B, sy.out, sx.out, g->Cout, g->Cin, &p.nslabs, &per, &p.npy, &p.npx);
    p.per_split = per;
    return p;
}
WgradPlan plan_taptable(const unetrir_conv_geom* g) {
    WgradArgs a{};
    wgrad_args(g, g->Cin, g->Cout, &a);
    WgradPlan p{WgKern::TAPTABLE};
    wgrad_plan(a.g, &p.nslabs, &p.per_split);
    return p;
}

// g is the geometry the kernels see (the adjoint one for the transposed layers), ldx / lddy the pixel strides of x / dy
WgradPlan plan_wgrad(const unetrir_conv_geom* g, bool bf16, int ldx, int lddy) {
    const unetrir_config& cfg = unetrir_cfg();
    const bool s1 = g->stride == 1;
    if (g->k == 3 && !bf16) return plan_patch(WgKern::PATCH, s1 ? WG_F32_TPH_S1 : WG_F32_TPH_S2, WG_TPW, g);
    if (g->k == 3) {          // LDS-DMA kernels first, then (stride 1) the register-staged twin, then the generic patch kernel
        const Wgrad3ArgsH a = wgrad3_args<Wgrad3ArgsH>(g, nullptr, ldx, nullptr, lddy);
        if (s1 && cfg.wgrad3x3g && wgrad3x3g_applies(a, true)) return plan_wgrad3x3g(g);
        if (s1 && cfg.wgrad3x3r && wgrad3x3r_applies(a)) return plan_patch(WgKern::WGRAD3X3R, WG_ROW_TPH, WG_ROW_TPW, g);
        if (!s1 && cfg.wgrad3x3d && wgrad3x3d_applies(a, true)) return plan_wgrad3x3d(g);
        return plan_patch(WgKern::PATCH, s1 ? WG_BF16_TPH_S1 : WG_BF16_TPH_S2, WG_TPW, g);
    }
    if (g->k == 1 && bf16) return plan_patch(WgKern::PATCH1X1, s1 ? WG_1X1_TPH_S1 : WG_1X1_TPH_S2, WG_TPW, g);
    return plan_taptable(g);  // other kernel sizes, and fp32 1x1: the tap-table kernel (bf16: on the bf16 tensors as stored)
}

// The workspace of a weight gradient: the largest slab set of every plan that could serve the geometry - either storage type, any
// switches, any pixel strides (the shape rules without their ld limits) - so run_wgrad never needs more.  The 1x1 kernel is sized at
// both of its patch heights whatever the stride, as the query always has (ReduceBatch's packing follows its value).
size_t wgrad_ws_bytes(const unetrir_conv_geom* g) {
    int slabs = 0;
    auto cover = [&](const WgradPlan& p) { if (p.nslabs > slabs) slabs = p.nslabs; };
    if (g->k == 3) {
        const Wgrad3ArgsH a = wgrad3_args<Wgrad3ArgsH>(g, nullptr, g->Cin, nullptr, g->Cout);
        const bool s1 = g->stride == 1;
        cover(plan_patch(WgKern::PATCH, s1 ? WG_F32_TPH_S1 : WG_F32_TPH_S2, WG_TPW, g));
        cover(plan_patch(WgKern::PATCH, s1 ? WG_BF16_TPH_S1 : WG_BF16_TPH_S2, WG_TPW, g));
        if (s1 && wgrad3x3g_applies(a, false)) cover(plan_wgrad3x3g(g));
        if (s1 && wgrad3x3r_applies(a)) cover(plan_patch(WgKern::WGRAD3X3R, WG_ROW_TPH, WG_ROW_TPW, g));
        if (!s1 && wgrad3x3d_applies(a, false)) cover(plan_wgrad3x3d(g));
    } else {
        cover(plan_taptable(g));
        if (g->k == 1) {
            cover(plan_patch(WgKern::PATCH1X1, WG_1X1_TPH_S1, WG_TPW, g));
            cover(plan_patch(WgKern::PATCH1X1, WG_1X1_TPH_S2, WG_TPW, g));
        }
    }
    return (size_t)slabs * g->Cout * g->k * g->k * g->Cin * sizeof(float);
}

// the partial-sum kernel of plan p into part
int launch_wgrad(const unetrir_conv_geom* g, const WgradPlan& p, bool bf16, const void* x, int ldx, const void* dy, int lddy, float* part,
                 hipStream_t s) {
    if (p.kernel == WgKern::TAPTABLE) {
        WgradArgs a{};
        wgrad_args(g, ldx, lddy, &a);
        a.x = (const float*)x; a.dy = (const float*)dy; a.part = part; a.chunks_per_split = p.per_split;
        return launch_igemm_wgrad(a, p.nslabs, s, bf16);
    }
    if (!bf16) {
        Wgrad3Args a = wgrad3_args<Wgrad3Args>(g, x, ldx, dy, lddy);
        a.part = part; a.patches_per_split = (int)p.per_split; a.npy = p.npy; a.npx = p.npx;
        return launch_wgrad3x3(a, g->stride, p.nslabs, s);
    }
    Wgrad3ArgsH a = wgrad3_args<Wgrad3ArgsH>(g, x, ldx, dy, lddy);
    a.part = part; a.patches_per_split = (int)p.per_split; a.npy = p.npy; a.npx = p.npx;
    switch (p.kernel) {
        case WgKern::WGRAD3X3G: return launch_wgrad3x3g_bf16(a, p.nslabs, s);
        case WgKern::WGRAD3X3R: return launch_wgrad3x3r_bf16(a, p.nslabs, s);
        case WgKern::WGRAD3X3D: return launch_wgrad3x3d_bf16(a, p.nslabs, s);
        case WgKern::PATCH1X1: return launch_wgrad1x1_bf16(a, g->stride, p.nslabs, s);
        default: return launch_wgrad3x3_bf16(a, g->stride, p.nslabs, s);
    }
}

// Conv2DTranspose(k, s=2, 'same') on an H x W input is the adjoint of Conv2D(k, s=2, 'same') that maps the
// 2H x 2W grid back to H x W: swap the channel roles and double the spatial size.
inline unetrir_conv_geom adjoint_geom(const unetrir_conv_geom* g) {
    unetrir_conv_geom c = *g;
    c.H = g->H * g->stride; c.W = g->W * g->stride;
    c.Cin = g->Cout; c.Cout = g->Cin;
    return c;
}

inline bool ld_ok(int ld, int c) { return ld >= c && (ld & 3) == 0; }
inline bool ldh_ok(int ld, int c) { return ld >= c && (ld & 7) == 0; }     // bf16: 16-byte rows

// One weight gradient dw[Cout][k][k][Cin] = sum_pixels dy * x + reg * w (transposed: of the Conv2DTranspose, whose weight gradient is
// that of its adjoint Conv2D - with our dy as its x and our x as its dy).  The planned kernel writes dw itself (one slab, reg == 0) or
// its slabs into ws; then the fixed-order reduction is launched or, with `defer`, described there for unetrir_splitk_reduce_batched.
template <class P>
int run_wgrad(const unetrir_conv_geom* gin, bool transposed, const void* x, int ldx, const void* dy, int lddy, float* dw, float reg,
              const float* w, void* ws, size_t ws_bytes, unetrir_reduce_desc* defer, hipStream_t s) {
    if (defer) *defer = unetrir_reduce_desc{};          // nsplit == 0: nothing to reduce
    if (!geom_ok(gin)) return UNETRIR_EINVAL;
    const unetrir_conv_geom g = transposed ? adjoint_geom(gin) : *gin;
    if (transposed) { std::swap(x, dy); std::swap(ldx, lddy); }
    const bool ld_fits = P::is_bf16 ? (g.Cin & 7) == 0 && (g.Cout & 7) == 0 && ldh_ok(ldx, g.Cin) && ldh_ok(lddy, g.Cout)
                                    : (g.Cin & 3) == 0 && ld_ok(ldx, g.Cin) && ld_ok(lddy, g.Cout);
    if (!x || !dy || !dw || !ld_fits || (reg != 0.f && !w)) return UNETRIR_EINVAL;
    ProfScope ps(conv_family(&g, UNETRIR_FAM_CONV_WGRAD), conv_flops(&g), s);
    const WgradPlan p = plan_wgrad(&g, P::is_bf16, ldx, lddy);
    const size_t nout = (size_t)g.Cout * g.k * g.k * g.Cin;
    const bool direct = p.nslabs == 1 && reg == 0.f;
    if (!direct && ws_bytes < (size_t)p.nslabs * nout * sizeof(float)) return UNETRIR_EINVAL;
    float* part = direct ? dw : (float*)ws;
    const int err = launch_wgrad(&g, p, P::is_bf16, x, ldx, dy, lddy, part, s);
    if (err || direct) return err;
    if (!defer) return launch_splitk_reduce(part, p.nslabs, nout, dw, reg, w, s);
    *defer = unetrir_reduce_desc{part, p.nslabs, nout, dw, reg, w};
    return 0;
}

// ---- the 2x2 stride-2 layers on even sizes (conv2x2.hip): entry points of their own, never chosen by plan_conv / plan_wgrad.
// A layer as the kernels see it: a coarse grid B x PH x PW and a fine grid of twice the size; Conv2D(2, strides=2) maps fine ->
// coarse (H, W of the geometry = the fine grid, which must be even), Conv2DTranspose(2, strides=2) coarse -> fine (H, W = the
// coarse grid).
struct C22Layer { int B, PH, PW, Cfine, Ccoarse; };
inline bool c22_layer(const unetrir_conv_geom* g, bool transposed, C22Layer* l) {
    if (!geom_ok(g) || g->k != 2 || g->stride != 2) return false;
    if (!transposed && ((g->H | g->W) & 1)) return false;
    *l = transposed ? C22Layer{g->B, g->H, g->W, g->Cout, g->Cin} : C22Layer{g->B, g->H / 2, g->W / 2, g->Cin, g->Cout};
    return l->Cfine <= 512;           // the gather form keeps 32 kernel rows of 4 Cfine values in LDS
}
inline double c22_flops(const C22Layer& l) { return 2.0 * l.B * l.PH * l.PW * 4.0 * l.Cfine * l.Ccoarse; }

// gather: fine -> coarse (Conv2D forward, Conv2DTranspose data gradient); scatter: coarse -> fine (the other two)
int run_c22_gemm(const unetrir_conv_geom* g, bool transposed, bool scatter, int fam, const void* in, int ldi, const void* w,
                 const float* bias, const void* addend, int ldadd, void* out, int ldo, hipStream_t s) {
    C22Layer l;
    if (!c22_layer(g, transposed, &l) || !in || !w || !out) return UNETRIR_EINVAL;
    C22Args a{};
    a.in = (const __bf16*)in; a.ldi = ldi; a.w = (const __bf16*)w; a.bias = bias; a.addend = (const __bf16*)addend; a.ldadd = ldadd;
    a.out = (__bf16*)out; a.ldo = ldo; a.B = l.B; a.PH = l.PH; a.PW = l.PW;
    a.C = scatter ? l.Ccoarse : l.Cfine; a.N = scatter ? l.Cfine : l.Ccoarse;
    if (!conv2x2s2_gemm_applies(a, scatter)) return UNETRIR_EINVAL;
    ProfScope ps(fam, c22_flops(l), s);
    return launch_conv2x2s2_gemm_bf16(a, scatter, s);
}

C22WgradArgs c22_wgrad_args(const C22Layer& l, const void* coarse, int ldc, const void* fine, int ldf) {
    C22WgradArgs a{};
    a.small = (const __bf16*)coarse; a.lds = ldc; a.S = l.Ccoarse; a.large = (const __bf16*)fine; a.ldl = ldf; a.L = l.Cfine;
    a.B = l.B; a.PH = l.PH; a.PW = l.PW;
    return a;
}

size_t c22_wgrad_ws_bytes(const unetrir_conv_geom* g, bool transposed) {
    C22Layer l;
    if (!c22_layer(g, transposed, &l)) return 0;
    if (!conv2x2s2_wgrad_applies(c22_wgrad_args(l, nullptr, l.Ccoarse, nullptr, l.Cfine))) return 0;
    int nslabs; long long per;
    conv2x2s2_wgrad_plan(l.B, l.PH, l.PW, l.Ccoarse, l.Cfine, &nslabs, &per);
    return (size_t)nslabs * l.Ccoarse * 4 * l.Cfine * sizeof(float);
}

// dw in the layer's primary layout [coarse channel][2][2][fine channel] (Conv2D: [Cout][2][2][Cin]; Conv2DTranspose:
// [Cin][2][2][Cout]) = sum over pixels + reg * w; slabs, direct write and the deferred reduction as run_wgrad has them.
int run_c22_wgrad(const unetrir_conv_geom* g, bool transposed, const void* x, int ldx, const void* dy, int lddy, float* dw, float reg,
                  const float* w, void* ws, size_t ws_bytes, unetrir_reduce_desc* defer, hipStream_t s) {
    if (defer) *defer = unetrir_reduce_desc{};
    C22Layer l;
    if (!c22_layer(g, transposed, &l) || !x || !dy || !dw || (reg != 0.f && !w)) return UNETRIR_EINVAL;
    C22WgradArgs a = transposed ? c22_wgrad_args(l, x, ldx, dy, lddy) : c22_wgrad_args(l, dy, lddy, x, ldx);
    if (!conv2x2s2_wgrad_applies(a)) return UNETRIR_EINVAL;
    int nslabs;
    conv2x2s2_wgrad_plan(l.B, l.PH, l.PW, l.Ccoarse, l.Cfine, &nslabs, &a.blocks_per_split);
    const size_t nout = (size_t)l.Ccoarse * 4 * l.Cfine;
    const bool direct = nslabs == 1 && reg == 0.f;
    if (!direct && (!ws || ws_bytes < (size_t)nslabs * nout * sizeof(float))) return UNETRIR_EINVAL;
    a.part = direct ? dw : (float*)ws;
    ProfScope ps(UNETRIR_FAM_CONV_WGRAD, c22_flops(l), s);
    const int err = launch_conv2x2s2_wgrad_bf16(a, nslabs, s);
    if (err || direct) return err;
    if (!defer) return launch_splitk_reduce(a.part, nslabs, nout, dw, reg, w, s);
    *defer = unetrir_reduce_desc{a.part, nslabs, nout, dw, reg, w};
    return 0;
}

// Which passes of the layer the caller should run on these kernels: UNETRIR_C22_FWD | _DGRAD | _WGRAD (ld_fine / ld_coarse: pixel
// strides of the tensors on the two grids).  A pass is offered where the kernel computes it AND the record (profiles/aenet.json: the
// default AENet at 144 x 160, batch 32, both variants alternating in one process) shows it not slower than the generic entry point:
// the weight gradient everywhere (2.06 - 2.58 x), the GEMM forms up to K = 256 (1.07 - 2.01 x; at K = 512 and 1024 a 32 ... 128
// channel tile re-reads the pixels N / tile times through L2 and the tap-table kernel's 128-pixel tiles win: 0.70 - 0.86 x).
// The rule is GENERALISED from those eight layer shapes (batch 32, number_filters_0 = 32, channels 32 ... 512): the shapes of
// number_filters_0 = 16 and 64 (16 and 1024 channels) and small batches were not timed, yet the predicate decides for them too.
constexpr int C22_GEMM_MAX_K = 256;
int c22_supported(const unetrir_conv_geom* g, bool transposed, int ld_fine, int ld_coarse) {
    C22Layer l;
    if (!c22_layer(g, transposed, &l)) return 0;
    C22Args ga{}, sc{};
    ga.B = sc.B = l.B; ga.PH = sc.PH = l.PH; ga.PW = sc.PW = l.PW;
    ga.C = l.Cfine; ga.N = l.Ccoarse; ga.ldi = ld_fine; ga.ldo = ld_coarse;
    sc.C = l.Ccoarse; sc.N = l.Cfine; sc.ldi = ld_coarse; sc.ldo = ld_fine;
    const bool gather = conv2x2s2_gemm_applies(ga, false) && 4 * ga.C <= C22_GEMM_MAX_K;
    const bool scatter = conv2x2s2_gemm_applies(sc, true) && sc.C <= C22_GEMM_MAX_K;
    int mask = conv2x2s2_wgrad_applies(c22_wgrad_args(l, nullptr, ld_coarse, nullptr, ld_fine)) ? UNETRIR_C22_WGRAD : 0;
    if (transposed ? scatter : gather) mask |= UNETRIR_C22_FWD;
    if (transposed ? gather : scatter) mask |= UNETRIR_C22_DGRAD;
    return mask;
}

}  // namespace

extern "C" {

int unetrir_abi_version(void) { return UNETRIR_ABI_VERSION; }

int unetrir_conv2x2s2_supported_bf16(const unetrir_conv_geom* g, int ld_in, int ld_out) { return c22_supported(g, false, ld_in, ld_out); }
int unetrir_conv2x2s2_transpose_supported_bf16(const unetrir_conv_geom* g, int ld_in, int ld_out) {
    return c22_supported(g, true, ld_out, ld_in);
}

int unetrir_conv2x2s2_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w, const float* bias,
                               const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy, unetrir_stream_t stream) {
    return run_c22_gemm(g, false, false, UNETRIR_FAM_CONV_FWD, x, ldx, w, bias, addend, ldadd, y, ldy, (hipStream_t)stream);
}

int unetrir_conv2x2s2_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                                 const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx, unetrir_stream_t stream) {
    return run_c22_gemm(g, false, true, UNETRIR_FAM_CONV_DGRAD, dy, lddy, wt, nullptr, addend, ldadd, dx, lddx, (hipStream_t)stream);
}

size_t unetrir_conv2x2s2_wgrad_ws_bytes(const unetrir_conv_geom* g) { return c22_wgrad_ws_bytes(g, false); }

int unetrir_conv2x2s2_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy, float* dw,
                                 float reg_coef, const float* w, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    return run_c22_wgrad(g, false, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int unetrir_conv2x2s2_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy,
                                          float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                          unetrir_reduce_desc* desc, unetrir_stream_t stream) {
    if (!desc) return UNETRIR_EINVAL;
    return run_c22_wgrad(g, false, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, desc, (hipStream_t)stream);
}

int unetrir_conv2x2s2_transpose_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* wt,
                                         const float* bias, unetrir_bf16* y, int ldy, unetrir_stream_t stream) {
    return run_c22_gemm(g, true, true, UNETRIR_FAM_CONV_FWD, x, ldx, wt, bias, nullptr, 0, y, ldy, (hipStream_t)stream);
}

int unetrir_conv2x2s2_transpose_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* w,
                                           const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx,
                                           unetrir_stream_t stream) {
    return run_c22_gemm(g, true, false, UNETRIR_FAM_CONV_DGRAD, dy, lddy, w, nullptr, addend, ldadd, dx, lddx, (hipStream_t)stream);
}

size_t unetrir_conv2x2s2_transpose_wgrad_ws_bytes(const unetrir_conv_geom* g) { return c22_wgrad_ws_bytes(g, true); }

int unetrir_conv2x2s2_transpose_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy,
                                           float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                           unetrir_stream_t stream) {
    return run_c22_wgrad(g, true, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int unetrir_conv2x2s2_transpose_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                                    int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                                    unetrir_reduce_desc* desc, unetrir_stream_t stream) {
    if (!desc) return UNETRIR_EINVAL;
    return run_c22_wgrad(g, true, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, desc, (hipStream_t)stream);
}

int unetrir_conv2d_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* w, const float* bias,
                           const float* addend, int ldadd, float* y, int ldy, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !w || !y || (g->Cin & 3) || !ld_ok(ldx, g->Cin) || ldy < g->Cout) return UNETRIR_EINVAL;
    return run_conv<F32>({g, FWD, x, ldx, w, nullptr, bias, addend, ldadd, y, ldy, nullptr}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                         conv_flops(g), (hipStream_t)stream);
}

int unetrir_conv2d_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy, const float* wt,
                             const float* addend, int ldadd, float* dx, int lddx, unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !wt || !dx || (g->Cout & 3) || !ld_ok(lddy, g->Cout) || lddx < g->Cin) return UNETRIR_EINVAL;
    return run_conv<F32>({g, DGRAD, dy, lddy, wt, nullptr, nullptr, addend, ldadd, dx, lddx, nullptr},
                         conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(g), (hipStream_t)stream);
}

size_t unetrir_conv2d_wgrad_ws_bytes(const unetrir_conv_geom* g) { return geom_ok(g) ? wgrad_ws_bytes(g) : 0; }

int unetrir_conv2d_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* dy, int lddy, float* dw,
                             float reg_coef, const float* w, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    return run_wgrad<F32>(g, false, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int unetrir_conv2d_transpose_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* wt,
                                     const float* bias, float* y, int ldy, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !wt || !y || (g->Cin & 3) || !ld_ok(ldx, g->Cin) || ldy < g->Cout)
        return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<F32>({&c, TFWD, x, ldx, wt, nullptr, bias, nullptr, 0, y, ldy, nullptr}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                         conv_flops(&c), (hipStream_t)stream);
}

int unetrir_conv2d_transpose_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy, const float* w,
                                       const float* addend, int ldadd, float* dx, int lddx, unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !w || !dx || (g->Cout & 3) || !ld_ok(lddy, g->Cout) || lddx < g->Cin)
        return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<F32>({&c, FWD, dy, lddy, w, nullptr, nullptr, addend, ldadd, dx, lddx, nullptr},
                         conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(&c), (hipStream_t)stream);
}

size_t unetrir_conv2d_transpose_wgrad_ws_bytes(const unetrir_conv_geom* g) {
    if (!geom_ok(g)) return 0;
    const unetrir_conv_geom c = adjoint_geom(g);
    return wgrad_ws_bytes(&c);
}

int unetrir_conv2d_transpose_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* dy, int lddy,
                                       float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                       unetrir_stream_t stream) {
    return run_wgrad<F32>(g, true, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

/* ---- bf16-storage variants: x / dy / y / dx and the weight work copies are bf16, bias fp32, weight gradients fp32 ---- */
int unetrir_conv2d_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w, const float* bias,
                            const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !w || !y || (g->Cin & 7) || !ldh_ok(ldx, g->Cin) || ldy < g->Cout) return UNETRIR_EINVAL;
    return run_conv<BF16>({g, FWD, x, ldx, w, nullptr, bias, addend, ldadd, y, ldy, nullptr}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                          conv_flops(g), (hipStream_t)stream, true);
}

size_t unetrir_conv3x3s2_packed_elems(int N, int C) {
    if (N <= 0 || C <= 0 || (N & 63) || (C & 63)) return 0;
    return (size_t)((N + 127) / 128) * 128 * 9 * C;
}

int unetrir_conv2d_fwd_packed_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w,
                                   const unetrir_bf16* w_packed, const float* bias, const unetrir_bf16* addend, int ldadd,
                                   unetrir_bf16* y, int ldy, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !w || !y || (g->Cin & 7) || !ldh_ok(ldx, g->Cin) || ldy < g->Cout) return UNETRIR_EINVAL;
    return run_conv<BF16>({g, FWD, x, ldx, w, w_packed, bias, addend, ldadd, y, ldy, nullptr}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                          conv_flops(g), (hipStream_t)stream);
}

int unetrir_conv2d_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                              const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx, unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !wt || !dx || (g->Cout & 7) || !ldh_ok(lddy, g->Cout) || lddx < g->Cin) return UNETRIR_EINVAL;
    return run_conv<BF16>({g, DGRAD, dy, lddy, wt, nullptr, nullptr, addend, ldadd, dx, lddx, nullptr},
                          conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(g), (hipStream_t)stream, true);
}

/* Fused column statistics and the kernel serving a 3x3 stride-1 layer: fields of the plan (plan_conv) of the launch as the query
 * describes it.  rows == 0: the kernel serving this layer cannot emit statistics. */
long long unetrir_conv2d_colstat_rows_bf16(const unetrir_conv_geom* g, int dgrad, int ld_in) {
    return geom_ok(g) ? plan_query(g, dgrad ? DGRAD : FWD, ld_in, true).colstat_rows : 0;
}

long long unetrir_conv2d_transpose_colstat_rows_bf16(const unetrir_conv_geom* g, int ld_in) {
    if (!geom_ok(g)) return 0;
    const unetrir_conv_geom c = adjoint_geom(g);
    return plan_query(&c, TFWD, ld_in, true).colstat_rows;
}

int unetrir_conv3x3_kernel_id_bf16(const unetrir_conv_geom* g, int dgrad, int ld_in) {
    if (!geom_ok(g) || g->k != 3 || g->stride != 1) return UNETRIR_K3_TAPTABLE;
    switch (plan_query(g, dgrad ? DGRAD : FWD, ld_in, false).kernel) {
        case Kern::PATCH: return UNETRIR_K3_PATCH;
        case Kern::STEM: return UNETRIR_K3_STEM;
        case Kern::CONV3X3G_PAIR: return UNETRIR_K3_CONV3X3G_PAIR;
        case Kern::CONV3X3P: return UNETRIR_K3_CONV3X3P;
        case Kern::CONV3X3G: return UNETRIR_K3_CONV3X3G;
        case Kern::CONV3X3S: return UNETRIR_K3_CONV3X3S;
        case Kern::CONV3X3H: return UNETRIR_K3_CONV3X3H;
        case Kern::CONV3X3R: return UNETRIR_K3_CONV3X3R;
        default: return UNETRIR_K3_TAPTABLE;
    }
}

int unetrir_conv2d_fwd_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w, const float* bias,
                                    const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy, float* colstat,
                                    unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !w || !y || !colstat || (g->Cin & 7) || !ldh_ok(ldx, g->Cin) || ldy < g->Cout) return UNETRIR_EINVAL;
    return run_conv<BF16>({g, FWD, x, ldx, w, nullptr, bias, addend, ldadd, y, ldy, colstat}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                          conv_flops(g), (hipStream_t)stream, true);
}

int unetrir_conv2d_dgrad_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                                      const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx, float* colstat,
                                      unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !wt || !dx || !colstat || (g->Cout & 7) || !ldh_ok(lddy, g->Cout) || lddx < g->Cin) return UNETRIR_EINVAL;
    return run_conv<BF16>({g, DGRAD, dy, lddy, wt, nullptr, nullptr, addend, ldadd, dx, lddx, colstat},
                          conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(g), (hipStream_t)stream, true);
}

int unetrir_conv2d_transpose_fwd_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* wt,
                                              const float* bias, unetrir_bf16* y, int ldy, float* colstat, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !wt || !y || !colstat || (g->Cin & 7) || !ldh_ok(ldx, g->Cin) || ldy < g->Cout) return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<BF16>({&c, TFWD, x, ldx, wt, nullptr, bias, nullptr, 0, y, ldy, colstat}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                          conv_flops(&c), (hipStream_t)stream);
}

int unetrir_conv2d_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy,
                              float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    return run_wgrad<BF16>(g, false, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

int unetrir_conv2d_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy,
                                       float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes, unetrir_reduce_desc* desc,
                                       unetrir_stream_t stream) {
    if (!desc) return UNETRIR_EINVAL;
    return run_wgrad<BF16>(g, false, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, desc, (hipStream_t)stream);
}

int unetrir_conv2d_transpose_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                                 int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                                 unetrir_reduce_desc* desc, unetrir_stream_t stream) {
    if (!desc) return UNETRIR_EINVAL;
    return run_wgrad<BF16>(g, true, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, desc, (hipStream_t)stream);
}

int unetrir_conv2d_transpose_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* wt,
                                      const float* bias, unetrir_bf16* y, int ldy, unetrir_stream_t stream) {
    if (!geom_ok(g) || !x || !wt || !y || (g->Cin & 7) || !ldh_ok(ldx, g->Cin) || ldy < g->Cout)
        return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<BF16>({&c, TFWD, x, ldx, wt, nullptr, bias, nullptr, 0, y, ldy, nullptr}, conv_family(g, UNETRIR_FAM_CONV_FWD),
                          conv_flops(&c), (hipStream_t)stream);
}

int unetrir_conv2d_transpose_dgrad_packed_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* w,
                                               const unetrir_bf16* w_packed, const unetrir_bf16* addend, int ldadd,
                                               unetrir_bf16* dx, int lddx, unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !w || !dx || (g->Cout & 7) || !ldh_ok(lddy, g->Cout) || lddx < g->Cin)
        return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<BF16>({&c, FWD, dy, lddy, w, w_packed, nullptr, addend, ldadd, dx, lddx, nullptr},
                          conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(&c), (hipStream_t)stream);
}

int unetrir_conv2d_transpose_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* w,
                                        const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx,
                                        unetrir_stream_t stream) {
    if (!geom_ok(g) || !dy || !w || !dx || (g->Cout & 7) || !ldh_ok(lddy, g->Cout) || lddx < g->Cin)
        return UNETRIR_EINVAL;
    const unetrir_conv_geom c = adjoint_geom(g);
    return run_conv<BF16>({&c, FWD, dy, lddy, w, nullptr, nullptr, addend, ldadd, dx, lddx, nullptr},
                          conv_family(g, UNETRIR_FAM_CONV_DGRAD), conv_flops(&c), (hipStream_t)stream);
}

int unetrir_conv2d_transpose_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                        int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                        unetrir_stream_t stream) {
    return run_wgrad<BF16>(g, true, x, ldx, dy, lddy, dw, reg_coef, w, ws, ws_bytes, nullptr, (hipStream_t)stream);
}

/* The stem's weight and bias gradients through the next 3x3 layer, without the data gradient between them (stem_composite.hip). */
int unetrir_stem_composite_supported(int B, int H, int W, int C0, int C1) { return stem_composite_applies(B, H, W, C0, C1) ? 1 : 0; }

size_t unetrir_stem_composite_ws_bytes(int B) { return B > 0 ? stem_composite_ws_bytes(B) : 0; }

int unetrir_stem_composite_bf16(const unetrir_bf16* g, int ldg, const unetrir_bf16* x, int ldx, int B, int H, int W,
                                const unetrir_bf16* w1t, float reg_coef, const float* w0, float* dw0, int ldw, float* db0, void* ws,
                                size_t ws_bytes, unetrir_stream_t stream) {
    if (!g || !x || !w1t || !dw0 || !db0 || !ws || !stem_composite_applies(B, H, W, 64, 64) || ldg < 64 || (ldg & 7) || ldx < 2 ||
        (ldx & 1) || ldw < 2 || ((uintptr_t)g & 15) || ((uintptr_t)x & 3) || ((uintptr_t)ws & 7) || (reg_coef != 0.f && !w0) ||
        ws_bytes < stem_composite_ws_bytes(B))
        return UNETRIR_EINVAL;
    return launch_stem_composite(g, ldg, x, ldx, B, H, W, w1t, reg_coef, w0, dw0, ldw, db0, ws, (hipStream_t)stream);
}

/* fp32 master weights [N][T][C] -> bf16 work copies: same orientation with the channel dimension padded to Cp, and
 * transposed [C][T][Np] with the row dimension padded to Np (pad entries are written as zero by the first; the second
 * leaves columns >= N untouched: pre-zero the buffer once). */
int unetrir_cast_weight_bf16(const float* w, unetrir_bf16* o, int N, int T, int C, int Cp, unetrir_stream_t stream) {
    if (!w || !o || N <= 0 || T <= 0 || C <= 0 || Cp < C) return UNETRIR_EINVAL;
    return launch_cast_weight(w, o, N, T, C, Cp, (hipStream_t)stream);
}

int unetrir_transpose_cast_weight_bf16(const float* w, unetrir_bf16* wt, int N, int T, int C, int Np, unetrir_stream_t stream) {
    if (!w || !wt || N <= 0 || T <= 0 || C <= 0 || Np < N) return UNETRIR_EINVAL;
    return launch_transpose_cast_weight(w, wt, N, T, C, Np, (hipStream_t)stream);
}

int unetrir_cast_weights_batched_bf16(const unetrir_cast_desc* desc, int n_layers, unetrir_stream_t stream) {
    if (!desc || n_layers <= 0 || n_layers > 65535) return UNETRIR_EINVAL;
    return launch_cast_weights_batched(desc, n_layers, (hipStream_t)stream);
}

/* Dense(N) (dl_models/u_net.py:259) on a small batch: y[B][N] = x[B][K] . w[N][K]^T + bias, split-K so that the 134 MB
 * weight matrix streams from every CU.  The data gradient is the same call with the transposed weight copy and no bias. */
size_t unetrir_dense_fwd_ws_bytes(int B, int K, int N) { return dense_fwd_ws_bytes(B, K, N); }

int unetrir_dense_fwd_f32(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B, int K, int N,
                          void* ws, size_t ws_bytes, unetrir_stream_t stream) {
    if (!x || !w || !y || !ws || B <= 0 || K <= 0 || N <= 0 || (K & 3) || ldx < K || (ldx & 3) || ldy < N) return UNETRIR_EINVAL;
    return launch_dense_fwd(x, ldx, w, bias, y, ldy, B, K, N, ws, ws_bytes, (hipStream_t)stream);
}

int unetrir_dense_dgrad_supported(int B, int K, int N) { return dense_dgrad_applies(B, K, N) ? 1 : 0; }

size_t unetrir_dense_dgrad_ws_bytes(int B, int K, int N) { return dense_dgrad_applies(B, K, N) ? dense_dgrad_ws_bytes(B, K, N) : 0; }

int unetrir_dense_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx, int B, int K, int N, void* ws,
                            size_t ws_bytes, unetrir_stream_t stream) {
    if (!dy || !w || !dx || !ws || !dense_dgrad_applies(B, K, N) || lddy < N || lddx < K || ((uintptr_t)w & 15) || ((uintptr_t)ws & 15))
        return UNETRIR_EINVAL;
    return launch_dense_dgrad(dy, lddy, w, dx, lddx, B, K, N, ws, ws_bytes, (hipStream_t)stream);
}

int unetrir_transpose_weight_f32(const float* w, float* wt, int N, int T, int C, unetrir_stream_t stream) {
    if (!w || !wt || N <= 0 || T <= 0 || C <= 0) return UNETRIR_EINVAL;
    return launch_transpose_weight(w, wt, N, T, C, (hipStream_t)stream);
}

int unetrir_stage_h2d(int n, const void* const* src, void* const* pinned, void* const* dev, const size_t* bytes,
                      unetrir_stream_t stream) {
    if (n <= 0 || !src || !pinned || !dev || !bytes) return UNETRIR_EINVAL;
    for (int k = 0; k < n; ++k) {
        if (!src[k] || !pinned[k] || !dev[k]) return UNETRIR_EINVAL;
        std::memcpy(pinned[k], src[k], bytes[k]);
        const hipError_t e = hipMemcpyAsync(dev[k], pinned[k], bytes[k], hipMemcpyHostToDevice, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

// ---- scoring of generated impulse responses (evalmetrics.hip): every argument is checked before the device is touched
int unetrir_eval_metrics_f32(const float* pred, const float* target, const float* phase_ref, int B, int H, int W,
                             const float* wav_pred, const float* wav_true, int T, int n50, double* out, unetrir_stream_t stream) {
    if (!pred || !target || !out || B <= 0 || H <= 0 || W <= 0) return UNETRIR_EINVAL;
    if ((wav_pred == nullptr) != (wav_true == nullptr)) return UNETRIR_EINVAL;          // the waveforms come as a pair
    if (wav_pred && (T <= 0 || n50 <= 0)) return UNETRIR_EINVAL;
    return launch_eval_metrics(pred, target, phase_ref, B, H, W, wav_pred, wav_true, T, n50, out, (hipStream_t)stream);
}

int unetrir_eval_accumulate(const double* out, const int* group, int B, int G, double* acc, unetrir_stream_t stream) {
    if (!out || !group || !acc || B <= 0 || G < 1 || G > (0x7fffffff >> 3) - 1) return UNETRIR_EINVAL;
    return launch_eval_accumulate(out, group, B, G, acc, (hipStream_t)stream);
}

// ---- room-acoustic figures of impulse responses (acoustics.hip): every argument is checked before the device is touched
int unetrir_acoustic_figures_f32(const float* wav_a, const float* wav_b, int B, int T, int n_pre, int n_dir, int n_early, double fs,
                                 double* fig, unetrir_stream_t stream) {
    if (!wav_a || !fig || B <= 0 || T <= 0 || n_pre < 0 || n_dir < 0 || n_early < 0 || !(fs > 0.0)) return UNETRIR_EINVAL;
    return launch_acoustic_figures(wav_a, wav_b, B, T, n_pre, n_dir, n_early, fs, fig, (hipStream_t)stream);
}

int unetrir_acoustic_accumulate(const double* fig, const int* group, int B, int G, double fs, double* err, double* acc,
                                unetrir_stream_t stream) {
    if (!fig || !group || !acc || B <= 0 || G < 0 || G > 0x7fffffff / 20 - 1 || !(fs > 0.0)) return UNETRIR_EINVAL;
    return launch_acoustic_accumulate(fig, group, B, G, fs, err, acc, (hipStream_t)stream);
}

int unetrir_prof_enable(int on) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    g_prof_on = on != 0;
    g_prof_mask = on == 2 ? (1u << UNETRIR_FAM_CONV_FWD) : ~0u;
    if (!g_prof_on) {
        for (auto& r : g_prof) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
        g_prof.clear();
    }
    return 0;
}

int unetrir_prof_collect(int* counts, double* ms, double* flops) {
    std::lock_guard<std::mutex> lk(g_prof_mu);
    for (int i = 0; i < UNETRIR_PROF_FAMILIES; ++i) { counts[i] = 0; ms[i] = 0.0; flops[i] = 0.0; }
    for (auto& r : g_prof) {
        hipEventSynchronize(r.e1);
        float t = 0.f;
        hipEventElapsedTime(&t, r.e0, r.e1);
        if (r.fam >= 0 && r.fam < UNETRIR_PROF_FAMILIES) { counts[r.fam]++; ms[r.fam] += t; flops[r.fam] += r.flops; }
        if (r.tag >= 0 && r.tag < UNETRIR_PROF_FAMILIES) { counts[r.tag]++; ms[r.tag] += t; flops[r.tag] += r.flops; }
        hipEventDestroy(r.e0); hipEventDestroy(r.e1);
    }
    g_prof.clear();
    return 0;
}

}  // extern "C"
