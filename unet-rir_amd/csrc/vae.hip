// vae.hip - what the variational autoencoder (dl_models/vae.py) adds to the Autoencoder's graph: the standard-normal draw of
// SamplingLayer.call (vae.py:34-39, tf.keras.backend.random_normal), the reparameterisation z = mu + exp(0.5 log_var) eps fused
// with the KL term of main_training.py:192-201, and its backward pass into the two Dense heads `mu` / `log_variance`
// (vae.py:466-468).  fp32 streaming kernels, plain HIP C++; the contracts are in include/unetrir.h.
#include "kernels.h"

#define GOLD64 0x9E3779B97F4A7C15ULL
// "NORMAL64": separates the noise key from the key dropout_mask_kernel derives from the same (seed, step) (elementwise.hip)
#define NORMAL_TAG 0x4E4F524D414C3634ULL
#define VAE_T 256

// Element i of draw (seed, step) - the recipe of include/unetrir.h (unetrir_normal_f32), one hash per output:
//   key = mix64(mix64(seed * GOLD + step) ^ TAG);  r = mix64(key + GOLD * (i + 1));
//   u1 = ((r >> 40) + 1) / 2^24 in (0, 1];  u2 = ((r >> 16) & 0xFFFFFF) / 2^24 in [0, 1);
//   out = sqrt(-2 ln u1) * cos(2 pi u2), evaluated as sqrtf(-2.f * logf(u1)) * cospif(2 u2) (2 u2 is exact in fp32).
__global__ void normal_kernel(float* __restrict__ out, long long n, unsigned long long seed, unsigned long long step,
                              const unsigned long long* __restrict__ step_dev) {
    if (step_dev) step += *step_dev;          // draw number from device memory (a captured HIP graph replays the same arguments)
    const unsigned long long key = mix64(mix64(seed * GOLD64 + step) ^ NORMAL_TAG);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long r = mix64(key + GOLD64 * (unsigned long long)(i + 1));
        const float u1 = (float)((unsigned)(r >> 40) + 1u) * (1.0f / 16777216.0f);              // 24 bits -> (0, 1]
        const float u2x2 = (float)((unsigned)(r >> 16) & 0xFFFFFFu) * (1.0f / 8388608.0f);      // the next 24 bits -> 2 u2 in [0, 2)
        out[i] = sqrtf(-2.0f * logf(u1)) * cospif(u2x2);
    }
}

// z = mu + exp(0.5 lv) eps and the KL sum over all B * L elements.  ONE workgroup: every thread adds its terms (fp32 expressions)
// into an fp64 partial in index order, the partials are summed by a fixed tree in LDS - two runs are bit-identical.  B * L is the
// latent tensor (main_training.py:143-152: 64 per sample), far below the size at which a second stage would pay.
__global__ __launch_bounds__(VAE_T) void vae_sample_kl_fwd_kernel(const float* __restrict__ mu, int ld_mu, const float* __restrict__ lv,
                                                                  int ld_lv, const float* __restrict__ eps, int B, int L, float inv_gb,
                                                                  float* __restrict__ z, int ld_z, float* __restrict__ kl_out) {
    __shared__ double red[VAE_T];
    const int L4 = L >> 2;
    const long long n4 = (long long)B * L4;
    double acc = 0.0;
    for (long long i = threadIdx.x; i < n4; i += VAE_T) {
        const long long b = i / L4;
        const int c = (int)(i - b * L4) << 2;
        const float4 m = *reinterpret_cast<const float4*>(mu + b * ld_mu + c);
        const float4 l = *reinterpret_cast<const float4*>(lv + b * ld_lv + c);
        const float4 e = *reinterpret_cast<const float4*>(eps + b * L + c);
        float4 o;
        o.x = m.x + expf(0.5f * l.x) * e.x;
        o.y = m.y + expf(0.5f * l.y) * e.y;
        o.z = m.z + expf(0.5f * l.z) * e.z;
        o.w = m.w + expf(0.5f * l.w) * e.w;
        *reinterpret_cast<float4*>(z + b * ld_z + c) = o;
        acc += (double)(-0.5f * (1.0f + l.x - m.x * m.x - expf(l.x)));
        acc += (double)(-0.5f * (1.0f + l.y - m.y * m.y - expf(l.y)));
        acc += (double)(-0.5f * (1.0f + l.z - m.z * m.z - expf(l.z)));
        acc += (double)(-0.5f * (1.0f + l.w - m.w * m.w - expf(l.w)));
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = VAE_T / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float raw = (float)red[0];
        kl_out[1] = raw;               // what kl_loss_object yields, summed (the *_loss_kl metrics average it)
        kl_out[0] = inv_gb * raw;      // compute_kl_loss: per-example sums / global batch
    }
}

// dmu = dz + inv_gb mu;  dlv = dz 0.5 exp(0.5 lv) eps + inv_gb 0.5 (exp(lv) - 1): first writer of both heads' gradients
__global__ void vae_sample_kl_bwd_kernel(const float* __restrict__ mu, int ld_mu, const float* __restrict__ lv, int ld_lv,
                                         const float* __restrict__ eps, const float* __restrict__ dz, int ld_dz, int B, int L, float inv_gb,
                                         float* __restrict__ dmu, int ld_dmu, float* __restrict__ dlv, int ld_dlv) {
    const int L4 = L >> 2;
    const long long n4 = (long long)B * L4;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long b = i / L4;
        const int c = (int)(i - b * L4) << 2;
        const float4 m = *reinterpret_cast<const float4*>(mu + b * ld_mu + c);
        const float4 l = *reinterpret_cast<const float4*>(lv + b * ld_lv + c);
        const float4 e = *reinterpret_cast<const float4*>(eps + b * L + c);
        const float4 g = *reinterpret_cast<const float4*>(dz + b * ld_dz + c);
        float4 gm, gl;
        gm.x = g.x + inv_gb * m.x;
        gm.y = g.y + inv_gb * m.y;
        gm.z = g.z + inv_gb * m.z;
        gm.w = g.w + inv_gb * m.w;
        gl.x = g.x * 0.5f * expf(0.5f * l.x) * e.x + inv_gb * (0.5f * (expf(l.x) - 1.0f));
        gl.y = g.y * 0.5f * expf(0.5f * l.y) * e.y + inv_gb * (0.5f * (expf(l.y) - 1.0f));
        gl.z = g.z * 0.5f * expf(0.5f * l.z) * e.z + inv_gb * (0.5f * (expf(l.z) - 1.0f));
        gl.w = g.w * 0.5f * expf(0.5f * l.w) * e.w + inv_gb * (0.5f * (expf(l.w) - 1.0f));
        *reinterpret_cast<float4*>(dmu + b * ld_dmu + c) = gm;
        *reinterpret_cast<float4*>(dlv + b * ld_dlv + c) = gl;
    }
}

// loss += compute_kl_loss(mean, log_var) (main_training.py:264-265): loss_out[0] of the sigmoid + loss kernel gains kl_out[0]
__global__ void vae_loss_add_kernel(const float* __restrict__ kl_out, float* __restrict__ loss_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) loss_out[0] += kl_out[0];
}

static inline unsigned vae_grid(long long n) {
    long long b = (n + VAE_T - 1) / VAE_T;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

static inline bool misaligned(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline bool bad_ld(int ld, int L) { return ld < L || (ld & 3); }

extern "C" {

int unetrir_normal_f32(float* out, long long n, unsigned long long seed, unsigned long long step, unetrir_stream_t stream) {
    if (!out || n <= 0) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(normal_kernel, dim3(vae_grid(n)), dim3(VAE_T), 0, (hipStream_t)stream, out, n, seed, step,
                       (const unsigned long long*)nullptr);
    return (int)hipGetLastError();
}

int unetrir_normal_dev_f32(float* out, long long n, unsigned long long seed, const unsigned long long* step_base,
                           unsigned long long step_offset, unetrir_stream_t stream) {
    if (!out || !step_base || n <= 0) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(normal_kernel, dim3(vae_grid(n)), dim3(VAE_T), 0, (hipStream_t)stream, out, n, seed, step_offset,
                       step_base);           // draw number = *step_base + step_offset
    return (int)hipGetLastError();
}

int unetrir_vae_sample_kl_fwd_f32(const float* mu, int ld_mu, const float* log_var, int ld_lv, const float* eps, int B, int L,
                                  float inv_global_batch, float* z, int ld_z, float* kl_out, unetrir_stream_t stream) {
    if (!mu || !log_var || !eps || !z || !kl_out || B <= 0 || L <= 0 || (L & 3) || bad_ld(ld_mu, L) || bad_ld(ld_lv, L) || bad_ld(ld_z, L))
        return UNETRIR_EINVAL;
    if (misaligned(mu) || misaligned(log_var) || misaligned(eps) || misaligned(z)) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(vae_sample_kl_fwd_kernel, dim3(1), dim3(VAE_T), 0, (hipStream_t)stream, mu, ld_mu, log_var, ld_lv, eps, B, L,
                       inv_global_batch, z, ld_z, kl_out);
    return (int)hipGetLastError();
}

int unetrir_vae_sample_kl_bwd_f32(const float* mu, int ld_mu, const float* log_var, int ld_lv, const float* eps, const float* dz,
                                  int ld_dz, int B, int L, float inv_global_batch, float* dmu, int ld_dmu, float* dlv, int ld_dlv,
                                  unetrir_stream_t stream) {
    if (!mu || !log_var || !eps || !dz || !dmu || !dlv || B <= 0 || L <= 0 || (L & 3) || bad_ld(ld_mu, L) || bad_ld(ld_lv, L) ||
        bad_ld(ld_dz, L) || bad_ld(ld_dmu, L) || bad_ld(ld_dlv, L))
        return UNETRIR_EINVAL;
    if (misaligned(mu) || misaligned(log_var) || misaligned(eps) || misaligned(dz) || misaligned(dmu) || misaligned(dlv)) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(vae_sample_kl_bwd_kernel, dim3(vae_grid((long long)B * (L >> 2))), dim3(VAE_T), 0, (hipStream_t)stream, mu, ld_mu,
                       log_var, ld_lv, eps, dz, ld_dz, B, L, inv_global_batch, dmu, ld_dmu, dlv, ld_dlv);
    return (int)hipGetLastError();
}

int unetrir_vae_loss_add_f32(const float* kl_out, float* loss_out, unetrir_stream_t stream) {
    if (!kl_out || !loss_out) return UNETRIR_EINVAL;
    hipLaunchKernelGGL(vae_loss_add_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, kl_out, loss_out);
    return (int)hipGetLastError();
}

}  // extern "C"
