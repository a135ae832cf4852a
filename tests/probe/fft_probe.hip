// fft_probe.hip - csrc/fft_lds.h on its own, for the tests (tests/fft_probe.py, tests/test_fft_lds*.py): the host walk of fft_walk.h and
// the same transforms on the device, image by image, with nothing of a consumer around them.  Built into libunetrir_probe.so by
// build.build_probe(); not part of libunetrir.so or of include/unetrir.h.
//
// Device form: group g = tid / (M / 8) of a workgroup of G M / 8 threads works image blockIdx.x G + g at img + g M with t = tid mod
// (M / 8); G = 1 is the header's own contract (M = 64: a workgroup of 8 threads), G = 2048 / M is 256 threads and 16 KB, the form of
// spectralloss_fft.hip.  Every group loads its image from global memory to fl_swz, the workgroup meets, the transforms run, and the
// group stores its image.  A group beyond n_img loads zeros, runs every pass (the barriers are the workgroup's) and stores nothing.
// Modes 2 and 3 are the call sequences of sf_spectra / sf_adjoint and of the two auralize kernels.  With stop >= 0 the same passes are
// called one by one (fl_pass_load, barrier, fl_pass_store, barrier) and the kernel ends after pass `stop`, as the host walk does.
#include "fft_walk.h"

using namespace fftlds;

namespace {

constexpr int PROBE_EINVAL = 10001;
constexpr int PROBE_THREADS = 256;                      // G M / 8 at G = 2048 / M

template <int M, int DIR, int NS = 1>
__device__ __forceinline__ void fft_upto(cf* buf, int t, int& left) {
    if constexpr (NS < M) {
        if (left == 0) return;                          // uniform over the workgroup
        --left;
        constexpr int R = fl_radix(M, NS);
        cf v[8];
        fl_pass_load<M, R>(buf, t, v);
        __syncthreads();
        fl_pass_store<M, R, NS, DIR>(buf, t, v);
        __syncthreads();
        fft_upto<M, DIR, NS * R>(buf, t, left);
    }
}

template <int M, int MODE>
__global__ __launch_bounds__(PROBE_THREADS) void probe_kernel(const cf* __restrict__ in, cf* __restrict__ out, long n_img, int G, int stop) {
    __shared__ cf img[FL_MAX_M];
    constexpr int TG = M / 8;
    const int g = threadIdx.x / TG, t = threadIdx.x % TG;   // g < G as the block is G TG threads, so g M + M <= 2048
    const long im = (long)blockIdx.x * G + g;
    const bool live = im < n_img;
    cf* buf = img + g * M;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int i = t + TG * e;
        buf[fl_swz(i)] = live ? in[im * M + i] : cf{0.f, 0.f};
    }
    __syncthreads();
    if (stop < 0) {
        if constexpr (MODE == 0) fl_fft<M, -1>(buf, t);
        if constexpr (MODE == 1) fl_fft<M, 1>(buf, t);
        if constexpr (MODE == 2) {
            fl_fft<M, -1>(buf, t);
            fl_split_fwd<M>(buf, t, TG);
            __syncthreads();
        }
        if constexpr (MODE == 3) {
            fl_split_inv<M>(buf, t, TG);
            __syncthreads();
            fl_fft<M, 1>(buf, t);
        }
    } else {
        int left = stop + 1;
        if constexpr (MODE == 0) fft_upto<M, -1>(buf, t, left);
        if constexpr (MODE == 1) fft_upto<M, 1>(buf, t, left);
        if constexpr (MODE == 2) {
            fft_upto<M, -1>(buf, t, left);
            if (left) fl_split_fwd<M>(buf, t, TG);
            __syncthreads();
        }
        if constexpr (MODE == 3) {
            if (left) {
                --left;
                fl_split_inv<M>(buf, t, TG);
            }
            __syncthreads();
            fft_upto<M, 1>(buf, t, left);
        }
    }
    if (live) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int i = t + TG * e;
            out[im * M + i] = buf[fl_swz(i)];
        }
    }
}

__global__ __launch_bounds__(PROBE_THREADS) void table_kernel(cf* __restrict__ out) {
    const int t = blockIdx.x * PROBE_THREADS + threadIdx.x;
    if (t < 2 * FL_TAB) {
        out[t] = fl_w<-1>(t);
        out[2 * FL_TAB + t] = fl_w<1>(t);
    }
}

template <int M>
void launch_m(int mode, dim3 grid, dim3 block, hipStream_t s, const cf* in, cf* out, long n_img, int G, int stop) {
    switch (mode) {
        case 0: probe_kernel<M, 0><<<grid, block, 0, s>>>(in, out, n_img, G, stop); break;
        case 1: probe_kernel<M, 1><<<grid, block, 0, s>>>(in, out, n_img, G, stop); break;
        case 2: probe_kernel<M, 2><<<grid, block, 0, s>>>(in, out, n_img, G, stop); break;
        default: probe_kernel<M, 3><<<grid, block, 0, s>>>(in, out, n_img, G, stop); break;
    }
}

}  // namespace

extern "C" {

// host walk: in, out [n_img][M] float2 on the host
int fftprobe_host(int M, int mode, int order, int stop, const void* in, void* out, long n_img) {
    if (!in || !out) return PROBE_EINVAL;
    return fftwalk::run(M, mode, order, stop, (const cf*)in, (cf*)out, n_img) ? PROBE_EINVAL : 0;
}

// device: in, out [n_img][M] float2 in device memory, 8-byte aligned; G = 1 or 2048 / M images per workgroup
int fftprobe_device(int M, int mode, int G, int stop, const void* in, void* out, long n_img, void* stream) {
    if (!fftwalk::valid_m(M) || mode < 0 || mode >= fftwalk::N_MODES || (G != 1 && G != FL_MAX_M / M) || !in || !out || n_img < 1 ||
        n_img > (1L << 24) || ((size_t)in & 7) || ((size_t)out & 7))
        return PROBE_EINVAL;
    const dim3 grid((unsigned)((n_img + G - 1) / G)), block(G * M / 8);
    hipStream_t s = (hipStream_t)stream;
    switch (M) {
        case 64: launch_m<64>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
        case 128: launch_m<128>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
        case 256: launch_m<256>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
        case 512: launch_m<512>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
        case 1024: launch_m<1024>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
        default: launch_m<2048>(mode, grid, block, s, (const cf*)in, (cf*)out, n_img, G, stop); break;
    }
    return (int)hipGetLastError();
}

// fl_w<-1>(t) in out[t] and fl_w<+1>(t) in out[4096 + t], 0 <= t < 4096: 8192 float2
void fftprobe_table_host(void* out) { fftwalk::table((cf*)out); }

int fftprobe_table_device(void* out, void* stream) {
    if (!out || ((size_t)out & 7)) return PROBE_EINVAL;
    table_kernel<<<dim3(2 * FL_TAB / PROBE_THREADS), dim3(PROBE_THREADS), 0, (hipStream_t)stream>>>((cf*)out);
    return (int)hipGetLastError();
}

// the 2048 entries of fl_tab_host as they are
void fftprobe_tab_host(void* out) {
    for (int t = 0; t < FL_TAB; ++t) ((cf*)out)[t] = fl_tab_host.w[t];
}

}  // extern "C"
