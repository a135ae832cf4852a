/*
 * unetrir.h - C ABI of the MI355X (gfx950) U-Net train-step hot path.
 *
 * The reference (igmsalinas/unet-rir) has no FFI: its hot path is a Keras graph
 * (dl_models/u_net.py:201-251) that TensorFlow lowers to cuDNN / NCCL.  Each
 * entry point below replaces the kernel TensorFlow would dispatch for one Keras
 * call site; the call site is cited next to it.  INTEGRATION.md shows the
 * ctypes binding a maintainer would add.
 *
 * Conventions (all entry points):
 *   - device pointers only, caller owns every buffer, 16-byte aligned;
 *   - activations are NHWC fp32 (the reference's own layout) addressed as
 *     base + pixel * ld + channel, `ld` (pixel stride in elements) >= channels and a
 *     multiple of 4, so a channel-concat is two writers into one buffer (no copy);
 *   - Conv2D weights are [Cout][kh][kw][Cin] ("OHWI"), Conv2DTranspose weights
 *     are [Cin][kh][kw][Cout] ("IHWO"): the layout the weight-gradient kernel
 *     produces; unetrir_transpose_weight_f32 makes the other one;
 *   - Cin and Cout multiples of 4 unless stated; TF padding='same' geometry;
 *   - asynchronous on `stream`, never allocate, never synchronise; thread-safe for
 *     distinct streams.  The library holds three pieces of process-global state, documented
 *     where they are declared: the kernel-selection switches (unetrir_config), the profiling
 *     brackets (unetrir_prof_*), and the tile-ticket slots of the persistent convolution
 *     kernels - a static device array of counters PER DEVICE (resolved for the device that is
 *     current at the launch; up to 16 devices per process), one slot per (device, stream) that
 *     has launched such a kernel (at most 128 streams per device; beyond that the kernels fall
 *     back to a fixed tile assignment), zero between launches (unetrir_reset_tile_tickets
 *     clears them from the host after a failed launch); no memory is allocated for it;
 *   - return 0 on success, a hipError_t value or UNETRIR_EINVAL otherwise.
 */
#ifndef UNETRIR_H
#define UNETRIR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UNETRIR_EINVAL 10001
#define UNETRIR_ABI_VERSION 1

typedef void* unetrir_stream_t; /* hipStream_t */
typedef uint16_t unetrir_bf16;  /* bfloat16 storage (upper 16 bits of an IEEE fp32) */

/* Geometry of one Conv2D / Conv2DTranspose(padding='same') call.
 * H, W: spatial size of the layer INPUT (for the transpose: the low-res input). */
typedef struct {
    int B, H, W;
    int Cin, Cout;
    int k;      /* square kernel size: 1, 3 or 6 in the reference graph */
    int stride; /* 1 or 2 */
} unetrir_conv_geom;

int unetrir_abi_version(void);

/* ---- kernel-selection switches.  Several hand-written kernels can serve the same layer (e.g. a 3x3 stride-1 convolution:
 *      tap-table implicit GEMM -> register-staged patch kernel -> LDS-DMA kernels).  The dispatch picks the most
 *      specialised one that takes the shape; a switch set to 0 removes that kernel from the dispatch, so the layer runs on
 *      the next more general one - for A/B measurements and for parity cross-checks between kernels.  The switches are
 *      read ONCE, at first use, from the environment variables named below (the only variables the library reads) into
 *      an immutable snapshot of this struct; unetrir_set_config publishes a new snapshot atomically (tests, A/B scripts:
 *      process-global; a launch issued concurrently on another thread sees the old values or the new ones, never a mixture
 *      within one read - but a dispatch reads the switches more than once, so flip them between launches).  Defaults: all 1.
 *      The order in which the convolution switches below (all but the weight-gradient ones, head_mfma, dyn_tiles and igemm2) are
 *      tried lives in one function, plan_conv in api.hip; the kernel-id and statistics-row queries answer from it.
 *      (Rounds 3's measured refusals - one-launch BatchNorm `bn_fused`, the LDS-DMA tap-table kernel `igemm3`, the head with
 *      BatchNorm on its load path - were removed from the library in round 4; DESIGN.md keeps their numbers.)
 *        conv3x3        UNETRIR_CONV3X3        3x3 stride-1: patch-staged kernels at all (0: tap-table implicit GEMM)
 *        conv3x3g       UNETRIR_CONV3X3G       bf16 LDS-DMA kernel, > 64 output channels, and 64 output channels from > 64 input channels (64-channel tiles; conv3x3g.hip)
 *        conv3x3g_pair  UNETRIR_CONV3X3G_PAIR  its two-images-per-tile form for images <= 16 wide: 0 off, 1 when it yields
 *                                              >= 32 workgroups (64-channel tiles), 2 whenever the shape allows
 *        conv3x3h       UNETRIR_CONV3X3H       bf16 LDS-DMA kernel, <= 64 output channels where conv3x3g / conv3x3s do not take the layer (conv3x3h.hip)
 *        conv3x3s       UNETRIR_CONV3X3S       bf16 strip kernel, 64 -> 64 channels, kernel resident in LDS (conv3x3s.hip)
 *        conv3x3r       UNETRIR_CONV3X3R       bf16 register-staged row-reuse kernel (conv3x3r.hip)
 *        stem           UNETRIR_STEM           bf16 first layer, 8 stored input channels (stem3x3.hip)
 *        upconv3x3g     UNETRIR_UPCONV3X3G     bf16 LDS-DMA transposed / strided-dgrad kernel (upconv3x3g.hip)
 *        wgrad3x3g      UNETRIR_WGRAD3X3G      bf16 LDS-DMA 3x3 weight gradient (wgrad3x3g.hip)
 *        wgrad3x3r      UNETRIR_WGRAD3X3R      bf16 register-staged 3x3 weight gradient (wgrad3x3r.hip)
 *        head_mfma      UNETRIR_HEAD_MFMA      bf16 6x6 head on the matrix cores (head_mfma.hip)
 *        wgrad3x3d      UNETRIR_WGRAD3X3D      bf16 LDS-DMA 3x3 stride-2 weight gradient (wgrad3x3d.hip)
 *        conv3x3d       UNETRIR_CONV3X3D       bf16 LDS-DMA 3x3 stride-2 forward / transposed data gradient (conv3x3d.hip)
 *        conv3x3p       UNETRIR_CONV3X3P       bf16 persistent form of conv3x3g for layers with >= 512 tiles (conv3x3p.hip)
 *        upconv3x3q     UNETRIR_UPCONV3X3Q     bf16 persistent form of upconv3x3g for layers with >= 512 tiles (upconv3x3q.hip)
 *        dyn_tiles      UNETRIR_DYN_TILES      bf16 persistent kernels draw their tiles at run time (0: fixed assignment per workgroup)
 *        pw1x1          UNETRIR_PW1X1          bf16 register-streaming kernel of the 1x1 layers, forward and data gradient (pw1x1.hip)
 *        igemm2         UNETRIR_IGEMM2         bf16 tap-table kernel for small problems: 64-pixel tiles, two K chunks in flight (igemm2_bf16.hip) */
typedef struct {
    int conv3x3, conv3x3g, conv3x3g_pair, conv3x3h, conv3x3s, conv3x3r, stem, upconv3x3g, wgrad3x3g, wgrad3x3r, head_mfma,
        wgrad3x3d, conv3x3d, conv3x3p, upconv3x3q, dyn_tiles, pw1x1, igemm2;
} unetrir_config;
int unetrir_get_config(unetrir_config* out);
int unetrir_set_config(const unetrir_config* in);
/* Zero every tile-ticket slot of the CURRENT device from the host (synchronous; call with the device idle): after a launch that
 * failed or was aborted, or when dyn_tiles is toggled between launches.  A healthy run never needs it - the last workgroup of
 * every persistent launch clears its own slot. */
int unetrir_reset_tile_tickets(void);

/* ---- Conv2D(padding='same'): dl_models/u_net.py:269-276 (strided, stride 1|2),
 *      :366 (3x3 block conv), :248 (6x6 head), :262 (1x1 on the information vector).
 *      y = conv(x, w) + bias (+ addend): `addend` (nullable) is the Add() of
 *      dl_models/u_net.py:229 fused into the epilogue.                            */
int unetrir_conv2d_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* w,
                           const float* bias, const float* addend, int ldadd, float* y, int ldy,
                           unetrir_stream_t stream);
/* dL/dx of the above (TensorFlow: Conv2DBackpropInput via tape.gradient, main_training.py:267).
 * wt = weights transposed to [Cin][kh][kw][Cout]; dx = conv^T(dy) (+ addend). */
int unetrir_conv2d_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy, const float* wt,
                             const float* addend, int ldadd, float* dx, int lddx,
                             unetrir_stream_t stream);
/* dL/dw (Conv2DBackpropFilter): dw[Cout][k][k][Cin] = sum_pixels dy * x  + reg_coef * w.
 * Deterministic split-K: partials go to `ws` (>= unetrir_conv2d_wgrad_ws_bytes), then a
 * fixed-order reduction.  `w` may be NULL when reg_coef == 0. */
size_t unetrir_conv2d_wgrad_ws_bytes(const unetrir_conv_geom* g);
int unetrir_conv2d_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* dy,
                             int lddy, float* dw, float reg_coef, const float* w, void* ws,
                             size_t ws_bytes, unetrir_stream_t stream);

/* ---- Conv2DTranspose(strides=2, padding='same'): dl_models/u_net.py:297-304.
 *      Defined as the adjoint of the SAME stride-2 conv on the 2H x 2W grid.
 *      fwd takes wt = [Cout][k][k][Cin]; dgrad and wgrad take/produce the primary
 *      [Cin][k][k][Cout].  g->H, g->W are the low-res input size, g->stride = 2. */
int unetrir_conv2d_transpose_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx,
                                     const float* wt, const float* bias, float* y, int ldy,
                                     unetrir_stream_t stream);
int unetrir_conv2d_transpose_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy,
                                       const float* w, const float* addend, int ldadd, float* dx,
                                       int lddx, unetrir_stream_t stream);
size_t unetrir_conv2d_transpose_wgrad_ws_bytes(const unetrir_conv_geom* g);
int unetrir_conv2d_transpose_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx,
                                       const float* dy, int lddy, float* dw, float reg_coef,
                                       const float* w, void* ws, size_t ws_bytes,
                                       unetrir_stream_t stream);

/* Dense(N) (dl_models/u_net.py:259, Flatten -> Dense) on a small batch: y[B][N] = x[B][K] . w[N][K]^T + bias (bias nullable),
 * split-K over the workgroups so the weight matrix streams from every CU; ws >= unetrir_dense_fwd_ws_bytes.  The data
 * gradient is the same call with the [K][N] weight copy and no bias. */
size_t unetrir_dense_fwd_ws_bytes(int B, int K, int N);
int unetrir_dense_fwd_f32(const float* x, int ldx, const float* w, const float* bias, float* y, int ldy, int B, int K,
                          int N, void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* Data gradient of the same layer from the SAME [N][K] kernel (no transposed copy): dx[b][k] = sum_n dy[b][n] w[n][k] for
 * B <= 32 batch rows, K % 4 == 0 (unetrir_dense_dgrad_supported).  The kernel streams once with 16-byte loads; n is split
 * over the workgroups and reduced in a fixed order; ws >= unetrir_dense_dgrad_ws_bytes. */
int unetrir_dense_dgrad_supported(int B, int K, int N);
size_t unetrir_dense_dgrad_ws_bytes(int B, int K, int N);
int unetrir_dense_dgrad_f32(const float* dy, int lddy, const float* w, float* dx, int lddx, int B, int K, int N, void* ws,
                            size_t ws_bytes, unetrir_stream_t stream);

/* [N][T][C] -> [C][T][N] (swap the channel roles of a conv kernel, taps kept). */
int unetrir_transpose_weight_f32(const float* w, float* wt, int N, int T, int C,
                                 unetrir_stream_t stream);

/* ---- BatchNormalization() training mode + Activation('relu'):
 *      dl_models/u_net.py:367-369 (Keras defaults eps=1e-3, momentum=0.99).
 *      x is [P][C] with pixel stride ldx.  stats: per-channel batch mean / biased
 *      variance (fp64 accumulation, two-stage deterministic), writes
 *      scale = gamma*rsqrt(var+eps), shift = beta - mean*scale into `affine[2*C]`,
 *      mean and rstd into `saved[2*C]`, and updates the moving statistics
 *      (moving = momentum*moving + (1-momentum)*batch, unbiased variance) when non-NULL.
 *      ws >= unetrir_bn_ws_bytes(P, C): ONE size per (P, C), sufficient for the fp32 and the bf16 form of every entry point
 *      that refers to it (bn_stats, bn_bwd, bn_bwd_junction, colsum) - the larger of the two kernels' needs; no kernel writes
 *      behind it. */
size_t unetrir_bn_ws_bytes(long long P, int C);
int unetrir_bn_stats_f32(const float* x, int ldx, long long P, int C, const float* gamma,
                         const float* beta, float eps, float momentum, float* moving_mean,
                         float* moving_var, float* affine, float* saved, void* ws, size_t ws_bytes,
                         unetrir_stream_t stream);
/* y = max(x*scale + shift, 0) (relu != 0) or x*scale + shift */
int unetrir_bn_apply_f32(const float* x, int ldx, long long P, int C, const float* affine, int relu,
                         float* y, int ldy, unetrir_stream_t stream);
/* Backward of BN(+ReLU): given da = dL/d(output), the saved conv output x and the batch
 * statistics, writes dx = dL/dx and dgamma, dbeta.  (TensorFlow: FusedBatchNormGradV3 + ReluGrad.) */
int unetrir_bn_bwd_f32(const float* da, int ldda, const float* x, int ldx, long long P, int C,
                       const float* gamma, const float* affine, const float* saved, int relu,
                       float* dx, int lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                       unetrir_stream_t stream);
/* Per-channel column sum (BiasAddGrad): out[c] = sum_p x[p][c]. */
int unetrir_colsum_f32(const float* x, int ldx, long long P, int C, float* out, void* ws,
                       size_t ws_bytes, unetrir_stream_t stream);
/* ReLU without BN (BatchNorm=False graphs): y = max(x, 0); dx = da * (x > 0). */
int unetrir_relu_fwd_f32(const float* x, int ldx, long long P, int C, float* y, int ldy,
                         unetrir_stream_t stream);
int unetrir_relu_bwd_f32(const float* da, int ldda, const float* x, int ldx, long long P, int C,
                         float* dx, int lddx, unetrir_stream_t stream);

/* ---- residual blocks of the ResAE graph (dl_models/res_ae.py:310-371, :453-514): BatchNormalization -> Add ->
 *      LeakyReLU() (keras default alpha 0.3).  Activation codes: 0 none, 1 ReLU, 2 LeakyReLU(0.3); the `relu` argument of
 *      unetrir_bn_apply / unetrir_bn_bwd accepts the same codes.
 *      bn_act_add: y = act(x*scale + shift + addend) (affine NULL = identity, addend NULL = none).
 *      act_bwd:    g = da * act'(out), derivative chosen by the sign of the activation output.
 *      add:        y = a + b (n % 4 == 0). */
int unetrir_bn_act_add_f32(const float* x, int ldx, long long P, int C, const float* affine, int act,
                           const float* addend, int ldadd, float* y, int ldy, unetrir_stream_t stream);
int unetrir_act_bwd_f32(const float* da, int ldda, const float* out, int ldo, long long P, int C, int act, float* g,
                        int ldg, unetrir_stream_t stream);
int unetrir_add_f32(const float* a, const float* b, float* y, long long n, unetrir_stream_t stream);
/* Backward of the whole junction out = act(BatchNormalization(x) + skip) in three launches (reduce, finalize, apply) instead
 * of seven: with g = da * act'(out) (decided by the sign of the stored OUTPUT `out`), dgamma / dbeta and dx are the BatchNorm
 * backward of g, and gskip = g (+ gskip_add; gskip_add may be gskip itself: in-place accumulation when `skip` has another
 * consumer whose gradient is already there; gskip NULL: the other operand needs no gradient).  ws >= unetrir_bn_ws_bytes(P, C). */
int unetrir_bn_bwd_junction_f32(const float* da, int ldda, const float* x, int ldx, const float* out, int ldo, long long P, int C,
                                const float* affine, const float* saved, int act, float* dx, int lddx, float* gskip, int ldgs,
                                const float* gskip_add, int ldga, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                unetrir_stream_t stream);

/* ---- boundary layout: the model input is NCHW [B,2,H,W] (north_star); the first conv reads
 *      NHWC padded to 4 channels.  nchw -> [B,H,W,Cpad] with zero fill, and back. */
int unetrir_nchw_to_nhwc_pad_f32(const float* x, int B, int C, int H, int W, float* y, int Cpad,
                                 unetrir_stream_t stream);

/* ---- head: Activation('sigmoid') (dl_models/u_net.py:249) fused with the loss of
 *      main_training.py:184-235.  logits is NHWC [B*H*W][ldl>=2]; pred/target are NCHW
 *      [B,2,H,W].  Writes pred = sigmoid(logits); partial sums of the data loss into ws and
 *      the final scalar loss_out[0] = sum(alpha*(a-a^)^2 + (1-alpha)*(1-cos(2pi(p-p^)))) /
 *      (2*H*W*global_batch), loss_out[1] = sum of the amplitude term, loss_out[2] = sum of
 *      the phase term; dlogits [B*H*W][4] = dL/dlogits (channels 2,3 zero). */
size_t unetrir_loss_ws_bytes(long long npix);
int unetrir_sigmoid_loss_f32(const float* logits, int ldl, const float* target, int B, int H, int W,
                             float alpha, float inv_norm, float* pred, float* dlogits,
                             float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* The same with the two switches of compute_loss (main_training.py:38-39): `phase_ref` (nullable; diff_loss, :214-217) = the
 * network INPUT, NCHW [B,2,H,W]: the phase target becomes target[:,1] - phase_ref[:,1]; `phase_weight` (nullable; sigmoid_loss,
 * :221-222 with preprocess.py:116-121) = [W] column weights multiplied into the phase term of the loss and its gradient.
 * loss_out[2] stays the UNWEIGHTED phase sum (the train_loss_phase metric, main_training.py:278-284). */
int unetrir_sigmoid_loss_ex_f32(const float* logits, int ldl, const float* target, const float* phase_ref,
                                const float* phase_weight, int B, int H, int W, float alpha, float inv_norm, float* pred,
                                float* dlogits, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* sigmoid only (inference / forward without a target) */
int unetrir_sigmoid_nchw_f32(const float* logits, int ldl, int B, int H, int W, float* pred,
                             unetrir_stream_t stream);
/* dlogits from an upstream gradient on the NCHW prediction: dl = dpred * p * (1 - p) */
int unetrir_sigmoid_bwd_f32(const float* pred, const float* dpred, int B, int H, int W,
                            float* dlogits, unetrir_stream_t stream);

/* ---- output head Conv2D(2, (6,6), padding='same') (dl_models/u_net.py:248), direct (non-MFMA) kernels: with 2
 *      output channels an implicit GEMM would waste 15/16 of every MFMA tile.  C % 8 == 0.
 *      fwd: w is [>=2][6][6][C] (rows 0,1 used); y is [B*H*W][ldy], ldy >= 2; with ldy >= 4 channels 2,3 are zeroed.
 *      wgrad: dw[0..1][6][6][C] = sum_pixels dy[p][0..1] * x[p+off][c]; dy is [B*H*W][lddy>=2]; further rows of a
 *      padded kernel gradient are left untouched.  ws >= unetrir_head6x6_wgrad_ws_bytes(C). */
int unetrir_head6x6_supported(int C);
int unetrir_head6x6_fwd_f32(const float* x, int ldx, int B, int H, int W, int C, const float* w, const float* bias,
                            float* y, int ldy, unetrir_stream_t stream);
size_t unetrir_head6x6_wgrad_ws_bytes(int C);
int unetrir_head6x6_wgrad_f32(const float* x, int ldx, int B, int H, int W, int C, const float* dy, int lddy,
                              float* dw, void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- information vector branch: Embedding(2000,256) -> Flatten (dl_models/u_net.py:257-258).
 *      idx int32 [n_idx]; out [n_idx][dim].  Backward is a deterministic gather-by-row:
 *      dtable[v] = sum over positions with idx == v, in position order. */
int unetrir_embedding_fwd_f32(const int* idx, int n_idx, const float* table, int vocab, int dim,
                              float* out, unetrir_stream_t stream);
int unetrir_embedding_bwd_f32(const int* idx, int n_idx, const float* dout, int vocab, int dim,
                              float* dtable, unetrir_stream_t stream);
/* y = x * mask (Dropout(.3), dl_models/u_net.py:260; mask already scaled by 1/(1-p)) */
int unetrir_mul_f32(const float* x, const float* m, float* y, long long n, unetrir_stream_t stream);
/* sum_i x_i^2 over n elements into out[0] (+= when accumulate != 0): l2 regulariser value. */
int unetrir_sumsq_f32(const float* x, long long n, float coef, float* out, int accumulate,
                      void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- tf.keras.optimizers.Adam (main_training.py:168-169, :268): beta1 .9, beta2 .999,
 *      epsilon 1e-7 outside the sqrt, lr_t = lr*sqrt(1-b2^t)/(1-b1^t).  One launch over a flat
 *      parameter buffer.  grad_scale multiplies g first (1/world_size style rescaling). */
int unetrir_adam_f32(float* theta, const float* g, float* m, float* v, long long n, float lr_t,
                     float beta1, float beta2, float eps, float grad_scale,
                     unetrir_stream_t stream);

/* ---- the other optimizers main_training.py:164-169 selects by name.  SGD(learning_rate): theta -= lr * grad_scale * g.
 *      Nadam(learning_rate) (tf.keras optimizer_v2: Nesterov Adam with the momentum schedule mu_t = beta1 (1 - 0.5 * 0.96^(0.004 t))):
 *      m, v as Adam; theta -= lr (c_g g + c_m m) / (sqrt(c_v v) + eps) with c_g = (1 - mu_t) / (1 - prod_{i<=t} mu_i),
 *      c_m = mu_{t+1} / (1 - prod_{i<=t+1} mu_i), c_v = 1 / (1 - beta2^t), computed by the caller per step. */
int unetrir_sgd_f32(float* theta, const float* g, long long n, float lr, float grad_scale, unetrir_stream_t stream);
int unetrir_nadam_f32(float* theta, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps,
                      float c_g, float c_m, float c_v, float grad_scale, unetrir_stream_t stream);

/* ---- step counters in DEVICE memory, so that a whole train step can be captured once into a HIP graph and replayed: the values
 *      that change from step to step (Adam's bias-corrected rate, the dropout draw number) are then read by the kernels instead
 *      of being launch arguments.
 *      state: 3 x uint64 {Adam step count t, dropout draws made so far, first draw of the current step};
 *      cfg:   5 x float  {lr, beta1, beta2, eps, grad_scale} as the host last set them;
 *      hyper: 5 x float  written by step_advance: {lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t), beta1, beta2, eps, grad_scale}.
 *      step_advance:      t += 1 (advance_t != 0), hyper from cfg, state[2] = state[1], state[1] += n_draws (one launch at the
 *                         start of a step; advance_t = 0 for a forward-only pass that draws dropout masks).
 *      adam_dev:          unetrir_adam_f32 with its five scalars read from `hyper`.
 *      dropout_mask_dev:  unetrir_dropout_mask_f32 with draw number *step_base + step_offset (step_base = state + 2). */
int unetrir_step_advance(unsigned long long* state, const float* cfg, float* hyper, int n_draws, int advance_t,
                         unetrir_stream_t stream);
int unetrir_adam_dev_f32(float* theta, const float* g, float* m, float* v, long long n, const float* hyper,
                         unetrir_stream_t stream);
int unetrir_dropout_mask_dev_f32(float* mask, long long n, float p, unsigned long long seed,
                                 const unsigned long long* step_base, unsigned long long step_offset, unetrir_stream_t stream);

/* ---- tfa.optimizers.LAMB(learning_rate) (trainer.py:37-38; tensorflow_addons' _resource_apply_dense).  PARITY UNPINNED
 *      (tensorflow_addons is not available here): a restatement of the source text, held to an fp64 restatement.  Per variable,
 *      step t (1-based), g already multiplied by grad_scale:
 *          m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) g^2;   m^ = m / corr1;   v^ = v / corr2
 *          u = m^ / (sqrt(v^) + eps)  [+ weight_decay w  if the variable is flagged UNETRIR_LAMB_DECAY]
 *          r = ||w||_2 / ||u||_2  if the variable is flagged UNETRIR_LAMB_ADAPT and both norms are > 0, else 1
 *          w = w - (lr r) u
 *      corr1 = 1 - beta1^t, corr2 = 1 - beta2^t, formed in fp64 from the fp32 betas and rounded to fp32 once (by the caller, or -
 *      the _dev form - by the kernels from state[0] and cfg of unetrir_step_advance: lr, the betas, eps and grad_scale then come
 *      from cfg too, so a captured step replays correctly; weight_decay stays a launch argument).  tfa's defaults: beta1 .9,
 *      beta2 .999, eps 1e-6, weight_decay 0; the reference passes learning_rate only (no decay, every variable adapted).
 *      The variables are described by a table of unetrir_lamb_seg, one per variable, slots back to back in the flat buffers:
 *      only the first `count` elements of a slot are read for the norms or written (the alignment tail is carried through
 *      unchanged).  unetrir_lamb_table_init validates a table (offsets / slots multiples of 4, 1 <= count <= slot, contiguous),
 *      fills every chunk0 and - when chunk_seg is given, with room for chunk_cap entries - the map chunk -> variable; it returns
 *      the number of chunks (-1: invalid table).  A chunk is unetrir_lamb_chunk_elems() consecutive elements of ONE variable,
 *      numbered from the variable's own start: the reduction order of a variable does not depend on the range a call covers.
 *      unetrir_lamb_f32 / _dev_f32 run the step on the variables whose slots are exactly [lo, hi) (element offsets into theta /
 *      g / m / v, which all share the table's layout) in THREE launches whatever the number of variables: moments + fp64 partial
 *      sums of w^2 and u^2 per chunk; one workgroup per variable combines them in a fixed order (comparison with zero and the
 *      division in fp64, one rounding to fp32); the step, with u recomputed from the stored m, v and the old w by the same
 *      arithmetic.  No atomics; two runs are bit-identical, and so are a whole-buffer call and calls range by range.
 *      segs_host and segs are the same initialised table in host and in device memory, chunk_seg is in device memory.
 *      ws: unetrir_lamb_ws_bytes(n_seg, n_chunks) bytes, 8-byte aligned, shared by every range of one table:
 *      n_chunks x {sum w^2, sum u^2} doubles, then n_seg floats r (readable after the call).
 *      UNETRIR_EINVAL before any launch: a null pointer, n_seg <= 0, theta / g / m / v not 16-byte aligned, [lo, hi) not beginning
 *      and ending on a variable boundary, ws_bytes too small. */
#define UNETRIR_LAMB_DECAY 1
#define UNETRIR_LAMB_ADAPT 2
typedef struct unetrir_lamb_seg {
    long long offset;   /* first element of the variable's slot */
    long long count;    /* the variable's own elements */
    long long slot;     /* slot length: the next variable starts at offset + slot */
    int flags;          /* UNETRIR_LAMB_DECAY | UNETRIR_LAMB_ADAPT */
    int chunk0;         /* number of the variable's first chunk (written by unetrir_lamb_table_init) */
} unetrir_lamb_seg;
int unetrir_lamb_chunk_elems(void);
long long unetrir_lamb_table_init(unetrir_lamb_seg* segs, int n_seg, int32_t* chunk_seg, long long chunk_cap);
size_t unetrir_lamb_ws_bytes(int n_seg, long long n_chunks);
int unetrir_lamb_f32(float* theta, const float* g, float* m, float* v, const unetrir_lamb_seg* segs_host, const unetrir_lamb_seg* segs,
                     const int32_t* chunk_seg, int n_seg, long long lo, long long hi, float lr, float beta1, float beta2, float eps,
                     float weight_decay, float corr1, float corr2, float grad_scale, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_lamb_dev_f32(float* theta, const float* g, float* m, float* v, const unetrir_lamb_seg* segs_host, const unetrir_lamb_seg* segs,
                         const int32_t* chunk_seg, int n_seg, long long lo, long long hi, float weight_decay,
                         const unsigned long long* state, const float* cfg, void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- bf16-storage variants (BASELINE.json configs[1] names bf16): activations, their gradients and the weight work
 *      copies are bfloat16 (unetrir_bf16), accumulation is fp32 (v_mfma_f32_32x32x16_bf16), bias / BatchNorm parameters /
 *      statistics / weight gradients / master weights stay fp32.  Channel counts and pixel strides are multiples of 8
 *      (16-byte rows).  Same call sites as the _f32 entry points above.  The weight gradient has dedicated bf16 kernels
 *      for 3x3 and 1x1 layers; other kernel sizes (kernels = 6, the reference's constructor default) run on the tap-table
 *      weight-gradient kernel with bf16 operand loads (fp32 MFMA arithmetic); the Dense layers stay fp32.
 *      `addend` of the forward / data-gradient entry points (here and in the _packed and _colstat forms): the convolution result
 *      (+ bias) is ROUNDED to bf16 first, the addend is added to that rounded value and the sum is rounded again -
 *      y = bf16(bf16(conv + bias) + addend), what storing the convolution and adding afterwards would give, in every kernel;
 *      addend may be the output itself (in-place accumulation). */
int unetrir_conv2d_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w,
                            const float* bias, const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy,
                            unetrir_stream_t stream);
int unetrir_conv2d_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                              const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx,
                              unetrir_stream_t stream);
int unetrir_conv2d_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                              int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                              unetrir_stream_t stream);
int unetrir_conv2d_transpose_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx,
                                      const unetrir_bf16* wt, const float* bias, unetrir_bf16* y, int ldy,
                                      unetrir_stream_t stream);
int unetrir_conv2d_transpose_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy,
                                        const unetrir_bf16* w, const unetrir_bf16* addend, int ldadd,
                                        unetrir_bf16* dx, int lddx, unetrir_stream_t stream);
int unetrir_conv2d_transpose_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx,
                                        const unetrir_bf16* dy, int lddy, float* dw, float reg_coef, const float* w,
                                        void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* Deferred split-K reduction.  Every weight gradient above ends in a fixed-order reduction of its fp32 partial slabs - a launch of
 * 5-20 us of which most is the launch itself, 23 times per step at configs[1], 57 times at configs[4].  The *_partials_* forms run
 * the same weight-gradient kernel, LEAVE the slabs in `ws` (which the caller must keep untouched until the reduction has run) and
 * fill `desc`; unetrir_splitk_reduce_batched then performs up to 16 such reductions per launch (more: several launches), each
 * output element summed by the same code in the same slab order as the single launch: bit-identical results.  desc->nsplit == 0
 * after the call: the kernel wrote dw directly, nothing is left to do (the batched call skips such descriptors). */
typedef struct unetrir_reduce_desc {
    const float* part; /* [nsplit][n] partial slabs */
    int nsplit;
    size_t n;          /* outputs */
    float* out;        /* [n]: sum over slabs + reg * w */
    float reg;
    const float* w;    /* nullable when reg == 0 */
} unetrir_reduce_desc;
int unetrir_conv2d_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                       int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                       unetrir_reduce_desc* desc, unetrir_stream_t stream);
int unetrir_conv2d_transpose_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx,
                                                 const unetrir_bf16* dy, int lddy, float* dw, float reg_coef, const float* w,
                                                 void* ws, size_t ws_bytes, unetrir_reduce_desc* desc, unetrir_stream_t stream);
int unetrir_splitk_reduce_batched(const unetrir_reduce_desc* desc, int n, unetrir_stream_t stream);
/* ---- The 2x2 stride-2 layers of AENet: Conv2D(k=2, strides=2, 'same') (dl_models/ae_net.py:273-279) and
 *      Conv2DTranspose(k=2, strides=2, 'same') (dl_models/ae_net.py:301-307), bf16 storage (conv2x2.hip).  On even sizes the windows
 *      do not overlap (TF 'same': pad_before 0, out = in / 2), so each pass is a GEMM with an index map: a gather-GEMM
 *      (M = B H/2 W/2, K = 4 Cin, N = Cout: Conv2D forward, Conv2DTranspose data gradient), a scatter-GEMM (K = Cin, N = 4 Cout,
 *      every output pixel written exactly once: Conv2DTranspose forward, Conv2D data gradient) and one weight-gradient launch for
 *      the four taps.  These entry points are the only way to the kernels - unetrir_conv2d_* never choose them - and take the SAME
 *      geometry, tensors, weight copies ([Cout][2][2][Cin] / [Cin][2][2][Cout], the orientation the corresponding unetrir_conv2d_*
 *      entry point takes), addend rule, workspace and descriptor conventions as their unetrir_conv2d_* / unetrir_conv2d_transpose_*
 *      twins, whose results they reproduce.
 *      The kernels compute: k == 2, stride == 2, (Conv2D: H and W even), both channel counts powers of two in [16, 1024] with at
 *      most 512 on the fine (larger) grid, ld >= channels and ld % 8 == 0, fewer than 2^31 fine pixels.
 *      *_supported_bf16(g, ld_in, ld_out): the passes of the layer with input / output pixel strides ld_in / ld_out that the caller
 *      should run here, as a mask of UNETRIR_C22_FWD | UNETRIR_C22_DGRAD | UNETRIR_C22_WGRAD: those the kernels compute AND
 *      profiles/aenet.json measured as not slower than the unetrir_conv2d_* twin (the weight gradient: always; forward and data
 *      gradient: up to K = 256, i.e. 4 x the fine-grid channels of a gather, the coarse-grid channels of a scatter).  The other
 *      passes - 0: all of them - run on the unetrir_conv2d_* entry points.
 *      UNETRIR_EINVAL before the device is touched: a geometry the kernels do not compute, a null required pointer, a pointer that
 *      is not 16-byte aligned, reg_coef != 0 without w, a workspace smaller than *_wgrad_ws_bytes (unless one slab suffices and
 *      reg_coef == 0: dw is then written directly), the _partials_ forms without a descriptor. */
#define UNETRIR_C22_FWD 1
#define UNETRIR_C22_DGRAD 2
#define UNETRIR_C22_WGRAD 4
int unetrir_conv2x2s2_supported_bf16(const unetrir_conv_geom* g, int ld_in, int ld_out);
int unetrir_conv2x2s2_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w, const float* bias,
                               const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy, unetrir_stream_t stream);
int unetrir_conv2x2s2_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                                 const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx, unetrir_stream_t stream);
size_t unetrir_conv2x2s2_wgrad_ws_bytes(const unetrir_conv_geom* g);
int unetrir_conv2x2s2_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy,
                                 float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_conv2x2s2_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                          int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                          unetrir_reduce_desc* desc, unetrir_stream_t stream);
int unetrir_conv2x2s2_transpose_supported_bf16(const unetrir_conv_geom* g, int ld_in, int ld_out);
int unetrir_conv2x2s2_transpose_fwd_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* wt,
                                         const float* bias, unetrir_bf16* y, int ldy, unetrir_stream_t stream);
int unetrir_conv2x2s2_transpose_dgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* w,
                                           const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx,
                                           unetrir_stream_t stream);
size_t unetrir_conv2x2s2_transpose_wgrad_ws_bytes(const unetrir_conv_geom* g);
int unetrir_conv2x2s2_transpose_wgrad_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* dy,
                                           int lddy, float* dw, float reg_coef, const float* w, void* ws, size_t ws_bytes,
                                           unetrir_stream_t stream);
int unetrir_conv2x2s2_transpose_wgrad_partials_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx,
                                                    const unetrir_bf16* dy, int lddy, float* dw, float reg_coef, const float* w,
                                                    void* ws, size_t ws_bytes, unetrir_reduce_desc* desc, unetrir_stream_t stream);
/* The stride-2 3x3 forward kernel (conv3x3d.hip: strided Conv2D forward, Conv2DTranspose data gradient) streams its kernel
 * 16 input channels at a time; from the [N][9][C] copy that is a gather of 32-byte pieces.  A PACKED copy holds the same values
 * in the order the kernel's LDS-DMA reads them - [N / 128][C / 16][9 taps][4 blocks of 32 channels][64 lanes][8 values], lane =
 * (row of the block, permuted as the MFMA accumulator layout wants it; 8-channel half) - so every DMA piece is 1 KB of
 * contiguous memory (measured: 22-26 us of 100-160 per launch).  In full, element (n, t, c) of the [N][9][C] kernel lies at
 *   group   n / 128        (N / 128 rounded up: a last group of 64 channels fills blocks 0 and 1, blocks 2 and 3 are never written)
 *   chunk   c / 16         (16 input channels)
 *   tap     t              (0 .. 8)
 *   block   (n / 32) % 4   (32 output channels)
 *   lane    row + 32 * ((c / 8) % 2), where row is the position m = n % 32 of the channel in its block with bits 2 and 3 of m
 *           exchanged: m = 16 a + 8 b + 4 c' + d (a, b, c' in {0, 1}, d in 0 .. 3) sits in row 16 a + 8 c' + 4 b + d.  (Lane half h
 *           of a 32 x 32 MFMA accumulator holds rows 8 j + 4 h + e, j, e in 0 .. 3: with this order they are the channels
 *           8 h .. 8 h + 7 and 16 + 8 h .. 16 + 8 h + 7 of the block - two runs of 8 consecutive channels, two 16-byte stores.)
 *   value   c % 8
 * with every dimension contiguous inside the one before it.  unetrir_cast_weights_batched_bf16 writes it when the
 * descriptor carries a destination, T == 9 and C % 16 == 0 - whether or not the descriptor also asks for the `same` or the
 * transposed copy - and never touches it otherwise; the _packed entry points take it beside the plain copy (NULL: plain copy
 * only).  unetrir_conv3x3s2_packed_elems returns the element count of the packed copy, 0 where none is defined (N or C not a
 * multiple of 64). */
size_t unetrir_conv3x3s2_packed_elems(int N, int C);
int unetrir_conv2d_fwd_packed_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w,
                                   const unetrir_bf16* w_packed, const float* bias, const unetrir_bf16* addend, int ldadd,
                                   unetrir_bf16* y, int ldy, unetrir_stream_t stream);
int unetrir_conv2d_transpose_dgrad_packed_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy,
                                               const unetrir_bf16* w, const unetrir_bf16* w_packed,
                                               const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx,
                                               unetrir_stream_t stream);
/* fp32 master weights [N][T][C] -> bf16 work copies: same orientation with channels zero-padded to Cp; transposed
 * [C][T][Np] with the row dimension zero-padded to Np. */
int unetrir_cast_weight_bf16(const float* w, unetrir_bf16* o, int N, int T, int C, int Cp, unetrir_stream_t stream);
int unetrir_transpose_cast_weight_bf16(const float* w, unetrir_bf16* wt, int N, int T, int C, int Np,
                                       unetrir_stream_t stream);
/* every layer's work copies in two launches: `desc` is an array of n_layers descriptors IN DEVICE MEMORY (same
 * semantics per layer as the two calls above; a NULL destination skips that copy). */
typedef struct unetrir_cast_desc {
    const float* w;            /* fp32 master [N][T][C] */
    unetrir_bf16* same;        /* bf16 [N][T][Cp] or NULL */
    unetrir_bf16* transposed;  /* bf16 [C][T][Np] or NULL */
    int N, T, C, Cp, Np, reserved;
    unetrir_bf16* packed_s2;   /* 3x3 kernels served by the stride-2 forward kernel: a third copy in the order its LDS-DMA reads it
                                  (unetrir_conv3x3s2_packed_elems(N, C) elements, zero-initialised by the caller), or NULL */
} unetrir_cast_desc;
int unetrir_cast_weights_batched_bf16(const unetrir_cast_desc* desc, int n_layers, unetrir_stream_t stream);
int unetrir_bn_stats_bf16(const unetrir_bf16* x, int ldx, long long P, int C, const float* gamma, const float* beta,
                          float eps, float momentum, float* moving_mean, float* moving_var, float* affine,
                          float* saved, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_bn_apply_bf16(const unetrir_bf16* x, int ldx, long long P, int C, const float* affine, int relu,
                          unetrir_bf16* y, int ldy, unetrir_stream_t stream);
int unetrir_bn_bwd_bf16(const unetrir_bf16* da, int ldda, const unetrir_bf16* x, int ldx, long long P, int C,
                        const float* affine, const float* saved, int relu, unetrir_bf16* dx, int lddx, float* dgamma,
                        float* dbeta, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_colsum_bf16(const unetrir_bf16* x, int ldx, long long P, int C, float* out, void* ws, size_t ws_bytes,
                        unetrir_stream_t stream);
int unetrir_relu_bwd_bf16(const unetrir_bf16* da, int ldda, const unetrir_bf16* x, int ldx, long long P, int C,
                          unetrir_bf16* dx, int lddx, unetrir_stream_t stream);
int unetrir_nchw_to_nhwc_pad_bf16(const float* x, int B, int C, int H, int W, unetrir_bf16* y, int Cpad,
                                  unetrir_stream_t stream);
/* head: bf16 activations in, fp32 logits [P][ldy] out; weight gradient from bf16 dlogits [P][lddy] */
int unetrir_head6x6_fwd_bf16(const unetrir_bf16* x, int ldx, int B, int H, int W, int C, const float* w,
                             const float* bias, float* y, int ldy, unetrir_stream_t stream);
int unetrir_head6x6_wgrad_bf16(const unetrir_bf16* x, int ldx, int B, int H, int W, int C, const unetrir_bf16* dy,
                               int lddy, float* dw, void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* ---- the stem's gradients through the next layer (bf16 storage).  Conv2D(64, 3x3) on the 2-channel input is followed by
 *      Conv2D(64 -> 64, 3x3) with nothing in between (dl_models/u_net.py:269-276, :366), so the stem's kernel and bias
 *      gradients follow from g = dL/d(output of the second convolution) [B][H][W][ldg] (64 channels), the network input x
 *      [B][H][W][ldx] (channels 0, 1 read) and the second kernel's transposed bf16 work copy w1t [64][9][64] - a 5 x 5
 *      correlation of x with g, border terms for the zero padding of the tensor between the two layers, and a contraction with
 *      w1t - without the 64-channel data gradient between them.  dw0 [64][3][3][ldw] = gradient + reg_coef * w0 (channels >= 2:
 *      reg_coef * w0), db0 [64].  Fixed summation order: bit-reproducible.  Supported for 64 -> 64 channels, W <= 4096, ldg a
 *      multiple of 8, ldx even; ws >= unetrir_stem_composite_ws_bytes(B), 8-byte aligned. */
int unetrir_stem_composite_supported(int B, int H, int W, int C0, int C1);
size_t unetrir_stem_composite_ws_bytes(int B);
int unetrir_stem_composite_bf16(const unetrir_bf16* g, int ldg, const unetrir_bf16* x, int ldx, int B, int H, int W,
                                const unetrir_bf16* w1t, float reg_coef, const float* w0, float* dw0, int ldw, float* db0,
                                void* ws, size_t ws_bytes, unetrir_stream_t stream);
/* ---- fused column statistics (bf16).  The 3x3 stride-1 kernels that serve most layers can emit, per 16 x 32 pixel tile,
 *      the per-channel (sum, sum of squares) of the bf16 output they store: colstat is [rows][N][2] floats with N the
 *      convolution's output channels (forward: Cout, data gradient: Cin).  BatchNormalization statistics (dl_models/
 *      u_net.py:204-206) and bias gradients then come from these rows instead of re-reading the tensor.
 *      unetrir_conv2d_colstat_rows_bf16 returns 0 when the kernel serving this layer (geometry, dgrad flag, pixel stride
 *      ld_in of its input) has no fused statistics; the *_colstat entry points then return UNETRIR_EINVAL. */
long long unetrir_conv2d_colstat_rows_bf16(const unetrir_conv_geom* g, int dgrad, int ld_in);
/* which hand-written kernel serves a 3x3 stride-1 layer (forward or data gradient) under the switches in effect: for tests and
 * measurement scripts that must know what they are looking at.  PATCH: the generic patch-staged kernel (conv3x3.hip), what is left
 * when the switches remove every specialised one */
enum { UNETRIR_K3_TAPTABLE = 0, UNETRIR_K3_CONV3X3R = 1, UNETRIR_K3_CONV3X3G = 2, UNETRIR_K3_CONV3X3G_PAIR = 3, UNETRIR_K3_CONV3X3H = 4,
       UNETRIR_K3_CONV3X3S = 5, UNETRIR_K3_CONV3X3P = 6, UNETRIR_K3_STEM = 7, UNETRIR_K3_PATCH = 8 };
int unetrir_conv3x3_kernel_id_bf16(const unetrir_conv_geom* g, int dgrad, int ld_in);
int unetrir_conv2d_fwd_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* w,
                                    const float* bias, const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy,
                                    float* colstat, unetrir_stream_t stream);
int unetrir_conv2d_dgrad_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* dy, int lddy, const unetrir_bf16* wt,
                                      const unetrir_bf16* addend, int ldadd, unetrir_bf16* dx, int lddx, float* colstat,
                                      unetrir_stream_t stream);
/* The same for every other convolution of the graphs (1x1 layers, strided layers, the tap-table path of small images): the
 * implicit-GEMM kernel emits one row per pixel tile (128 or 64 pixels) of its launch.  unetrir_conv2d_colstat_rows_bf16 answers for these
 * layers too (0 only where the serving kernel has none: 3x3 stride-2 forward, strided data gradients).  Conv2DTranspose
 * forward (dl_models/res_ae.py:310-371: every decoder convolution of the residual graph sits in front of a BatchNormalization):
 * stride 1 = one row per 128-pixel tile; stride 2 (1x1 'valid', 6x6) = the four output-parity classes, each with its own row
 * range (4 x tiles rows); 3x3 stride 2: none (0). */
long long unetrir_conv2d_transpose_colstat_rows_bf16(const unetrir_conv_geom* g, int ld_in);
int unetrir_conv2d_transpose_fwd_colstat_bf16(const unetrir_conv_geom* g, const unetrir_bf16* x, int ldx, const unetrir_bf16* wt,
                                              const float* bias, unetrir_bf16* y, int ldy, float* colstat,
                                              unetrir_stream_t stream);
/* as unetrir_bn_stats_f32 / unetrir_colsum_f32 but from colstat rows; fixed-order fp64 reduction over the rows.
 * colsum: out[0..C) = sum over rows of colstat[row][c0 + c][0], ldc = channels per row. */
int unetrir_bn_stats_colstat(const float* colstat, long long rows, long long P, int C, const float* gamma, const float* beta,
                             float eps, float momentum, float* moving_mean, float* moving_var, float* affine, float* saved,
                             unetrir_stream_t stream);
int unetrir_colsum_colstat(const float* colstat, long long rows, int ldc, int c0, int C, float* out, unetrir_stream_t stream);
/* unetrir_bn_stats_colstat followed by unetrir_bn_act_add_* in one call: statistics rows -> affine / saved / moving statistics, then
 * y = act(x * scale + shift (+ addend)): the finalize and the apply launch. */
int unetrir_bn_colstat_act_add_f32(const float* colstat, long long rows, const float* x, int ldx, long long P, int C, const float* gamma,
                                   const float* beta, float eps, float momentum, float* moving_mean, float* moving_var, float* affine,
                                   float* saved, int act, const float* addend, int ldadd, float* y, int ldy, unetrir_stream_t stream);
int unetrir_bn_colstat_act_add_bf16(const float* colstat, long long rows, const unetrir_bf16* x, int ldx, long long P, int C,
                                    const float* gamma, const float* beta, float eps, float momentum, float* moving_mean,
                                    float* moving_var, float* affine, float* saved, int act, const unetrir_bf16* addend, int ldadd,
                                    unetrir_bf16* y, int ldy, unetrir_stream_t stream);
/* head data gradient on the matrix cores: dx[p][c] = sum_{n<2,kh,kw} dy[p - off][n] * w[n][kh][kw][c] (the adjoint of
 * unetrir_head6x6_fwd_bf16; w is the fp32 [>=2][6][6][C] kernel, rounded to bf16 on load).  Only channels 0,1 of dy are
 * read.  Supported for C a multiple of 32 up to 512 (unetrir_head6x6_dgrad_supported; 64 channels per workgroup, images wider
 * than 256 pixels in column blocks); otherwise UNETRIR_EINVAL and the caller uses unetrir_conv2d_dgrad_bf16 on the padded kernel. */
int unetrir_head6x6_dgrad_supported(int W, int C);
int unetrir_head6x6_dgrad_bf16(const unetrir_bf16* dy, int lddy, int B, int H, int W, const float* w, int C,
                               unetrir_bf16* dx, int lddx, unetrir_stream_t stream);
/* as unetrir_sigmoid_loss_f32 / unetrir_sigmoid_bwd_f32 but dlogits is bf16 [B*H*W][8] (channels 2..7 zero) */
int unetrir_sigmoid_loss_bf16(const float* logits, int ldl, const float* target, int B, int H, int W, float alpha,
                              float inv_norm, float* pred, unetrir_bf16* dlogits, float* loss_out, void* ws,
                              size_t ws_bytes, unetrir_stream_t stream);
int unetrir_sigmoid_loss_ex_bf16(const float* logits, int ldl, const float* target, const float* phase_ref,
                                 const float* phase_weight, int B, int H, int W, float alpha, float inv_norm, float* pred,
                                 unetrir_bf16* dlogits, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_sigmoid_bwd_bf16(const float* pred, const float* dpred, int B, int H, int W, unetrir_bf16* dlogits,
                             unetrir_stream_t stream);
/* The clipped-ReLU output of AENet, `tf.keras.activations.relu(out, alpha=0.0, max_value=1)` (dl_models/ae_net.py:249), in place of
 * the sigmoid: pred = min(max(logit, 0), 1); dL/dlogit = dL/dpred where 0 < logit < 1, else 0 (the stored prediction tells it:
 * 0 < pred < 1).  unetrir_relu1_loss_ex_*: arguments, loss_out layout, phase_ref / phase_weight, alpha, inv_norm, workspace and the
 * fixed-order sums of unetrir_sigmoid_loss_ex_*; unetrir_relu1_nchw_f32: inference, as unetrir_sigmoid_nchw_f32; unetrir_relu1_bwd_*:
 * the autograd bridge, as unetrir_sigmoid_bwd_*. */
int unetrir_relu1_loss_ex_f32(const float* logits, int ldl, const float* target, const float* phase_ref, const float* phase_weight,
                              int B, int H, int W, float alpha, float inv_norm, float* pred, float* dlogits, float* loss_out,
                              void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_relu1_loss_ex_bf16(const float* logits, int ldl, const float* target, const float* phase_ref, const float* phase_weight,
                               int B, int H, int W, float alpha, float inv_norm, float* pred, unetrir_bf16* dlogits, float* loss_out,
                               void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_relu1_nchw_f32(const float* logits, int ldl, int B, int H, int W, float* pred, unetrir_stream_t stream);
int unetrir_relu1_bwd_f32(const float* pred, const float* dpred, int B, int H, int W, float* dlogits, unetrir_stream_t stream);
int unetrir_relu1_bwd_bf16(const float* pred, const float* dpred, int B, int H, int W, unetrir_bf16* dlogits, unetrir_stream_t stream);
/* The linear output of the phase-difference models, `Conv2D(2, (1, 1), activation='linear')` (dl_models/diff_u_net.py:247) and
 * `Activation("linear")` (dl_models/diff_vae.py:385), in place of the sigmoid: pred = logit, dL/dlogit = dL/dpred - a phase
 * difference lies in [-1, 1], which neither bounded output can reach.  unetrir_linear_loss_ex_*: arguments, loss_out layout,
 * phase_ref / phase_weight, alpha, inv_norm, workspace and the fixed-order sums of unetrir_relu1_loss_ex_*;
 * unetrir_linear_nchw_f32: inference (the NHWC -> NCHW copy); unetrir_linear_bwd_*: the autograd bridge (`pred` is not read). */
int unetrir_linear_loss_ex_f32(const float* logits, int ldl, const float* target, const float* phase_ref, const float* phase_weight,
                               int B, int H, int W, float alpha, float inv_norm, float* pred, float* dlogits, float* loss_out,
                               void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_linear_loss_ex_bf16(const float* logits, int ldl, const float* target, const float* phase_ref, const float* phase_weight,
                                int B, int H, int W, float alpha, float inv_norm, float* pred, unetrir_bf16* dlogits, float* loss_out,
                                void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_linear_nchw_f32(const float* logits, int ldl, int B, int H, int W, float* pred, unetrir_stream_t stream);
int unetrir_linear_bwd_f32(const float* pred, const float* dpred, int B, int H, int W, float* dlogits, unetrir_stream_t stream);
int unetrir_linear_bwd_bf16(const float* pred, const float* dpred, int B, int H, int W, unetrir_bf16* dlogits, unetrir_stream_t stream);
/* ---- output head Conv2D(2, (1, 1), activation='linear') of DiffUNet (dl_models/diff_u_net.py:247) on a bf16 trunk: streaming
 *      kernels, one pass over the activations forward and one for the whole backward pass (head1x1.hip).
 *      unetrir_head1x1_supported: mask of the passes served for C input channels - 1 forward, 2 backward; 0 unless C % 8 == 0 and
 *      8 <= C <= 256.  The caller runs the other passes on unetrir_conv2d_*_bf16 / unetrir_colsum_bf16 with the padded kernel.
 *      fwd: x bf16 [B*H*W][ldx], ldx >= C, ldx % 8 == 0; w the fp32 [>=2][C] kernel, rounded to bf16 on load (as
 *      unetrir_head6x6_fwd_bf16 does); bias fp32 [>=2]; y fp32 logits [B*H*W][ldy], ldy >= 4: channels 0, 1 written, 2, 3 zeroed,
 *      further ones untouched.  fp32 accumulation.
 *      bwd: dy bf16 [B*H*W][lddy], lddy >= 8, channels 0, 1 read.  dx[p][c] = dy[p][0] w[0][c] + dy[p][1] w[1][c], formed in fp32,
 *      rounded once, written (no addend); dw[j][c] = sum_p dy[p][j] x[p][c] and dbias[j] = sum_p dy[p][j] for j < 2 in fp32 (further
 *      rows / entries of a padded gradient are left untouched).  No atomics: one slab of partial sums per workgroup in ws
 *      (>= unetrir_head1x1_bwd_ws_bytes), summed by a second launch in a fixed order (64 runs of consecutive slabs in index order, then the run sums in run order);
 *      the slab count depends on (B, H, W, C) alone.
 *      Every pointer 16-byte aligned; UNETRIR_EINVAL otherwise, before the device is touched. */
int unetrir_head1x1_supported(int C);
int unetrir_head1x1_fwd_bf16(const unetrir_bf16* x, int ldx, int B, int H, int W, int C, const float* w, const float* bias,
                             float* y, int ldy, unetrir_stream_t stream);
size_t unetrir_head1x1_bwd_ws_bytes(int B, int H, int W, int C);
int unetrir_head1x1_bwd_bf16(const unetrir_bf16* x, int ldx, const unetrir_bf16* dy, int lddy, int B, int H, int W, int C,
                             const float* w, unetrir_bf16* dx, int lddx, float* dw, float* dbias, void* ws, size_t ws_bytes,
                             unetrir_stream_t stream);
/* glue between the bf16 trunk and the fp32 information-vector branch: y = a + b (Add(), dl_models/u_net.py:229);
 * fp32 copy of a bf16 gradient.  n is a multiple of 4. */
int unetrir_add_f32_to_bf16(const unetrir_bf16* a, const float* b, unetrir_bf16* y, long long n,
                            unetrir_stream_t stream);
int unetrir_cast_bf16_to_f32(const unetrir_bf16* a, float* y, long long n, unetrir_stream_t stream);
int unetrir_cast_f32_to_bf16(const float* a, unetrir_bf16* y, long long n, unetrir_stream_t stream);
/* residual-block glue in bf16 storage (as unetrir_bn_act_add_f32 / unetrir_act_bwd_f32; C % 8 == 0): the graphs of
 * dl_models/res_ae.py and the feature-block modes 1-3 of dl_models/u_net.py on the bf16 convolution kernels */
int unetrir_bn_act_add_bf16(const unetrir_bf16* x, int ldx, long long P, int C, const float* affine, int act,
                            const unetrir_bf16* addend, int ldadd, unetrir_bf16* y, int ldy, unetrir_stream_t stream);
int unetrir_act_bwd_bf16(const unetrir_bf16* da, int ldda, const unetrir_bf16* out, int ldo, long long P, int C, int act,
                         unetrir_bf16* g, int ldg, unetrir_stream_t stream);
int unetrir_bn_bwd_junction_bf16(const unetrir_bf16* da, int ldda, const unetrir_bf16* x, int ldx, const unetrir_bf16* out, int ldo,
                                 long long P, int C, const float* affine, const float* saved, int act, unetrir_bf16* dx, int lddx,
                                 unetrir_bf16* gskip, int ldgs, const unetrir_bf16* gskip_add, int ldga, float* dgamma, float* dbeta,
                                 void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- waveform <-> feature transforms at the two ends of the data path; all fp32 in HBM,
 *      fp64 direct DFT inside.  n_fft is a power of two <= 1024, win_length <= n_fft, window = periodic Hann centred in
 *      n_fft (librosa's default), centred frames (n_fft/2 samples of padding each side), frames = 1 + T / hop_length.
 *
 * unetrir_stft_features_f32 replaces Loader.load's mean removal (preprocess.py:56, remove_mean), FeatureExtractor.extract
 * (preprocess.py:13-18: librosa.stft -> abs, angle), Normalizer.normalize (preprocess.py:26-32, normalize) and
 * TensorPadder.pad_amp_phase (preprocess.py:65-70): wav [B][T] -> out [B][2][H][W] (plane 0 amplitude, plane 1 phase; row =
 * frequency bin, column = frame; rows >= n_fft/2+1 and columns >= frames are written as zeros).  pad_mode 0 = 'reflect'
 * (librosa < 0.10, the reference's era), 1 = 'constant'.  UNETRIR_EINVAL when H < n_fft/2+1, W < frames or T <= n_fft/2.
 *
 * unetrir_istft_features_f32 replaces PostProcess.post_process's arithmetic (postprocess.py:68-71, 'ph' branch :127-134):
 * TensorPadder.un_pad to n_bins x n_frames (preprocess.py:107-113), Normalizer.denormalize (preprocess.py:34-41,
 * denormalize) and librosa.istft: feat [B][2][H][W] -> wav [B][hop_length * (n_frames - 1)].  n_bins must be n_fft/2+1. */
int unetrir_stft_frames(int T, int hop_length);
int unetrir_stft_features_f32(const float* wav, int B, int T, int n_fft, int win_length, int hop_length, int pad_mode,
                              int remove_mean, int normalize, float* out, int H, int W, unetrir_stream_t stream);
int unetrir_istft_features_f32(const float* feat, int B, int H, int W, int n_bins, int n_frames, int n_fft, int win_length,
                               int hop_length, int denormalize, float* wav, unetrir_stream_t stream);

/* ---- a loss on the reconstructed waveform and its gradient on the prediction (waveloss.hip; the derivation is in its header).
 *
 * unetrir_wave_loss_f32: pred fp32 NCHW [B][2][H][W]; y^_b = the waveform unetrir_istft_features_f32(denormalize = 1) makes of pred_b
 * (phase_ref nullable [B][2][H][W] = the network INPUT: the reconstructed phase plane is pred + phase_ref, plane 1 of each, summed
 * in fp32); wav_true fp32 [B][T], T = hop_length (n_frames - 1); time_weight nullable fp32 [T] (null: ones).
 *   E_b = sum_t w[t] (y^_b[t] - y_b[t])^2;   D_b = T (norm 0) or sum_t w[t] y_b[t]^2 (norm 1);   a sample with D_b == 0 counts 0
 *   wave_out fp64 [2] = (sum_b E_b / D_b, sum_b E_b);   loss_out nullable: loss_out[0] += weight inv_global_batch wave_out[0]
 *   dpred nullable fp32 [B][2][H][W], every element written: d(weight inv_global_batch sum_b E_b / D_b) / d pred, exact zeros in rows
 *   >= n_bins and columns >= n_frames - plus, with spec_target [B][2][H][W] (nullable), over all H x W the gradient on pred of the
 *   spectrogram loss of unetrir_sigmoid_loss_ex_f32: -2 alpha inv_norm (t0 - p0) and -(1 - alpha) inv_norm 2 pi sin(ph) wgt with that
 *   kernel's t1 -= phase_ref, wgt = phase_weight[column] (nullable [W]) and ph.  Without dpred the adjoint kernel is not launched.
 *   wav_pred nullable fp32 [B][T]: y^, the bits of unetrir_istft_features_f32.
 * fp64 inside, one rounding per fp32 output, fixed summation order, no atomics: two runs give the same bits and a sample's bits depend
 * neither on B nor on its place in the batch (inv_global_batch is an argument).  ws: unetrir_wave_loss_ws_bytes(B, n_frames,
 * hop_length) bytes, 8-byte aligned (0: a geometry the kernels do not take).
 * UNETRIR_EINVAL before the device is touched: the geometry rules of unetrir_istft_features_f32, a null pred / wav_true / wave_out /
 * ws, norm outside {0, 1}, a negative or non-finite weight, a non-positive or non-finite inv_global_batch, ws_bytes too small. */
size_t unetrir_wave_loss_ws_bytes(int B, int n_frames, int hop_length);
int unetrir_wave_loss_f32(const float* pred, const float* phase_ref, const float* wav_true, const float* time_weight, int B, int H,
                          int W, int n_bins, int n_frames, int n_fft, int win_length, int hop_length, int norm, double weight,
                          double inv_global_batch, const float* spec_target, const float* phase_weight, float alpha, float inv_norm,
                          float* dpred, float* wav_pred, double* wave_out, float* loss_out, void* ws, size_t ws_bytes,
                          unetrir_stream_t stream);

/* ---- the vector-Jacobian product of PostProcess (istft_bwd.hip): the adjoint of unetrir_wave_loss_f32 as an entry point of its own.
 *
 * unetrir_istft_features_bwd_f32: pred fp32 NCHW [B][2][H][W], phase_ref nullable with the same layout (the phase plane is pred +
 * phase_ref, plane 1 of each, summed in fp32), dwav fp32 [B][T], T = hop_length (n_frames - 1): a cotangent on the waveform y^_b that
 * unetrir_istft_features_f32(denormalize = 1) makes of pred_b.  dpred[b] = (d y^_b / d pred_b)^T dwav_b: the math of waveloss.hip's
 * header with u[t] = dwav[t] / env[t] where env[t] > tiny and 0 elsewhere, env recomputed from the frames that reach a sample in
 * ascending order.  accumulate = 0: every element of dpred is written, exact zeros in rows >= n_bins and columns >= n_frames.
 * accumulate = 1: dpred[i] = (float)((double)dpred[i] + g), rows >= n_bins and columns >= n_frames are left untouched.
 * One launch, no workspace, no atomics, fp64 inside with one rounding per output; two runs give the same bits and a sample's bits
 * depend neither on B nor on its place in the batch.
 * UNETRIR_EINVAL before the device is touched: the geometry rules of unetrir_wave_loss_f32, a null pred / dwav / dpred. */
int unetrir_istft_features_bwd_f32(const float* pred, const float* phase_ref, const float* dwav, int B, int H, int W, int n_bins,
                                   int n_frames, int n_fft, int win_length, int hop_length, int accumulate, float* dpred,
                                   unetrir_stream_t stream);

/* ---- a loss on the energy decay curve of the waveform and its gradient on the waveform (decayloss.hip; the derivation is in its
 *      header).
 *
 * unetrir_decay_loss_f32: wav_pred (y^), wav_true (y) fp32 [B][T]; fp64 arithmetic; per row
 *   S_x[t] = sum_{s >= t} x[s]^2;  E0 = S_y[0];  delta = 10^(-floor_db / 10);  c_x[t] = 10 log10(S_x[t] / E0 + delta)
 *   Q_b = (1 / T) sum_t (c_y^[t] - c_y[t])^2  (dB^2);  a row with E0 == 0 counts nothing
 *   decay_out fp64 [2] = (sum_b Q_b, rows counted);   loss_out nullable: loss_out[0] += (float)(weight inv_global_batch decay_out[0])
 *   dwav nullable fp32 [B][T], every element written (zeros in rows that are not counted):
 *   dwav[b][s] = weight inv_global_batch 2 y^[s] sum_{t <= s} (2 / T) (c_y^[t] - c_y[t]) (10 / ln 10) / (S_y^[t] + delta E0)
 * Two launches whatever B is, no atomics, every order fixed: two runs give the same bits and a row's bits depend neither on B nor on
 * its place in the batch.  unetrir_decay_loss_supported(T): 1 for 1 <= T <= 16384 (a thread's run of the row stays in registers), else
 * 0.  ws: unetrir_decay_loss_ws_bytes(B, T) bytes, 8-byte aligned (0: B <= 0 or an unsupported T).
 * UNETRIR_EINVAL before the device is touched: a null wav_pred / wav_true / decay_out / ws, B <= 0, an unsupported T, floor_db not
 * finite or outside (0, 200], a negative or non-finite weight, a non-positive or non-finite inv_global_batch, ws too small or
 * misaligned. */
size_t unetrir_decay_loss_ws_bytes(int B, int T);
int unetrir_decay_loss_supported(int T);
int unetrir_decay_loss_f32(const float* wav_pred, const float* wav_true, int B, int T, double floor_db, double weight,
                           double inv_global_batch, float* dwav, double* decay_out, float* loss_out, void* ws, size_t ws_bytes,
                           unetrir_stream_t stream);

/* ---- the multi-resolution STFT loss on the waveform and its gradient on the waveform (spectralloss.hip; the derivation is in its
 *      header).
 *
 * unetrir_spectral_loss_f32: wav_pred (y^), wav_true (y) fp32 [B][T]; res: R triples (n_fft N, win_length, hop_length h) in HOST memory,
 * 1 <= R <= 8.  The transform of each is the analysis transform of features.hip: periodic Hann of win_length samples centred in N zeros
 * (left pad (N - win) / 2), centred frames with reflect padding of N / 2 each side, F = 1 + T / h frames, one-sided bins K = N / 2 + 1,
 * no mean removal, no normalisation.  fp64 arithmetic; per row b and resolution r
 *   E0_b = sum_t y_b[t]^2 (a row with E0 == 0 counts nothing: zeros in its gradient, nothing in any sum)
 *   P0 = (sum_n w_r[n]^2) E0_b / T;  delta = 10^(-floor_db / 10);  M_x[f,k] = sqrt(|X[f,k]|^2 + delta P0)
 *   SC_{b,r} = sum_{f,k} (M_y^ - M_y)^2 / sum_{f,k} M_y^2;   LM_{b,r} = (1 / (F K)) sum_{f,k} (ln M_y^ - ln M_y)^2
 *   Q_b = (1 / R) sum_r (sc_weight SC_{b,r} + log_weight LM_{b,r});   L = weight inv_global_batch sum_b Q_b
 *   spectral_out fp64 [3] = (sum_b mean_r SC, sum_b mean_r LM, rows counted);  loss_out nullable: loss_out[0] += (float) L
 *   dwav nullable fp32 [B][T]: every element written, or with accumulate every element dwav[i] = (float)((double)dwav[i] + g):
 *   g[f,k] = (weight inv_global_batch / R) [sc_weight 2 (M_y^ - M_y) / sum M_y^2 + log_weight 2 (ln M_y^ - ln M_y) / (F K M_y^)] / M_y^
 *   p[j] = sum_f w[j - f h] sum_k g[f,k] (Re X^[f,k] cos(2 pi k n / N) - Im X^[f,k] sin(2 pi k n / N)), n = j - f h in [0, N)
 *   dwav[t] = p[t + N/2] + p at the padded positions that reflect onto t (j < N/2 reads sample N/2 - j; j >= T + N/2 reads
 *   2 (T - 1) - (j - N/2)), summed over the resolutions in index order.
 * Four launches with dwav, two without, whatever B and R are; no atomics, every order fixed: two runs give the same bits and a row's
 * bits depend neither on B nor on its place in the batch; nothing is allocated, cleared or waited for.
 * unetrir_spectral_loss_supported: 1 for n_fft even, 16 <= n_fft <= 1024, 2 <= win_length <= n_fft, 1 <= hop_length,
 * n_fft / 2 + 1 <= T <= 16384, else 0.  ws: unetrir_spectral_loss_ws_bytes(B, T, R, res) bytes, 8-byte aligned (0: B <= 0, R outside
 * 1...8, a null res, an unsupported resolution, or more than 2^31 - 1 workgroups in a launch).
 * UNETRIR_EINVAL before the device is touched: a null wav_pred / wav_true / spectral_out / ws / res, B <= 0, R outside 1...8, an
 * unsupported resolution, floor_db not finite or outside (0, 200], a negative or non-finite sc_weight / log_weight / weight, a
 * non-positive or non-finite inv_global_batch, accumulate without dwav, ws too small or misaligned. */
int unetrir_spectral_loss_supported(int T, int n_fft, int win_length, int hop_length);
size_t unetrir_spectral_loss_ws_bytes(int B, int T, int R, const int* res);
int unetrir_spectral_loss_f32(const float* wav_pred, const float* wav_true, int B, int T, int R, const int* res, double floor_db,
                              double sc_weight, double log_weight, double weight, double inv_global_batch, int accumulate, float* dwav,
                              double* spectral_out, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- the FFT form of the multi-resolution STFT loss: the same definition with fp32 transforms in LDS (spectralloss_fft.hip, fft_lds.h).
 *
 * unetrir_spectral_loss_fft_f32: arguments and their rules as unetrir_spectral_loss_f32; the same E0, P0, delta, M_x, SC, LM, Q_b, L,
 * gradient, frames, fold of the reflected edges and order of the resolutions.  Only the arithmetic differs: window taps, spectra and
 * every per-bin quantity are fp32 (a real transform of N points as a complex FFT of N / 2 points, radix-8 Stockham, twiddles correctly
 * rounded from fp64); every reduction (E0, sum w^2, the three sums of a (row, resolution), the sums over r and b, the overlap-add and
 * fold of a sample) is accumulated in fp64 from fp32 terms in a fixed order; every element of dwav is rounded once (or, with
 * accumulate, dwav[i] = (float)((double)dwav[i] + g)).  The adjoint recomputes the spectra of its frames: the workspace holds the
 * partial sums and the windowed fp32 frames only (4 bytes per frame and window tap; no spectra).
 * Four launches with dwav, two without, whatever B and R are; no atomics, every order fixed: two runs give the same bits and a row's
 * bits depend neither on B nor on its place in the batch; nothing is allocated, cleared or waited for.  A row with a silent target
 * counts nothing and gets zeros.  The bits are NOT those of unetrir_spectral_loss_f32.
 * Error.  No derived per-element bound: the result is that of an fp32 STFT and its adjoint.  With e(v) = max_t |v - dwav64| /
 * max_t |dwav64| per row against the fp64 definition, the tests hold e(kernel) <= 4 e(complex64 torch.stft under autograd) + 2^-22
 * on independent y^ and y (the complex64 form itself: about 1e-4 of the peak at the default resolutions), and spectral_out[0:2] and the
 * increment of loss_out to a relative 64 log2(N_max) 2^-24 (6.66 u per radix-2 level in L2 [Higham, Theorem 24.2], twice for M_y^ - M_y,
 * twice for the square, a factor |M| / |M_y^ - M_y| <= 2 on independent data, rounded up); spectral_out[2] is exact.  e grows as
 * y^ -> y, where M_y^ - M_y cancels: unetrir_spectral_loss_f32 is the form for a gradient that must be held to a
 * bound.  Inputs are taken to be finite and delta P0 to be a normal fp32 number.
 * unetrir_spectral_loss_fft_supported: 1 for n_fft in {128, 256, 512, 1024}, 2 <= win_length <= n_fft, 1 <= hop_length,
 * n_fft / 2 + 1 <= T <= 16384, else 0.  ws: unetrir_spectral_loss_fft_ws_bytes(B, T, R, res) bytes, 8-byte aligned (0: B <= 0, R
 * outside 1...8, a null res, an unsupported resolution, or more than 2^31 - 1 workgroups in a launch).
 * UNETRIR_EINVAL before the device is touched: in the cases of unetrir_spectral_loss_f32, with this predicate and this size. */
int unetrir_spectral_loss_fft_supported(int T, int n_fft, int win_length, int hop_length);
size_t unetrir_spectral_loss_fft_ws_bytes(int B, int T, int R, const int* res);
int unetrir_spectral_loss_fft_f32(const float* wav_pred, const float* wav_true, int B, int T, int R, const int* res, double floor_db,
                                  double sc_weight, double log_weight, double weight, double inv_global_batch, int accumulate, float* dwav,
                                  double* spectral_out, float* loss_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- auralization: dry audio rendered through impulse responses, y_b = h_b * x_b (auralize.hip; the formulation is in its header).
 *
 * unetrir_auralize_f32: rir fp32 [B][K] (h); dry fp32 [N] with dry_stride = 0 (one dry signal for all rows) or [B][dry_stride], dry_stride
 * >= N (one per row); out fp32 [B][L], 1 <= L <= N + K - 1 - the first L samples of the full convolution:
 *   out[b][n] = sum_{k=0}^{K-1} h_b[k] x_b[n - k],   x_b[m] = 0 outside 0 <= m < N.
 * Direct form in ONE launch on v_mfma_f32_32x32x2_f32, no workspace, no atomics; every element of out written exactly once and nothing
 * beyond it.  Summation order: fp32 throughout, one fma per tap in ascending k onto an accumulator that starts at +0,
 *   out[b][n] = fma(h[K-1], x[n-K+1], ... fma(h[1], x[n-1], fma(h[0], x[n], +0)) ...)      (taps that fall outside x add exact zeros),
 * so the bits of an element depend on (h_b, x_b, n) alone: not on B, the row's place in the batch, L (a truncated call returns the
 * head of the full result), dry_stride (shared or per row) or the run; on integer data whose partial sums stay below 2^24 the result
 * is exact.  Inputs are taken to be finite.  unetrir_auralize_supported(K): 1 for 1 <= K <= 16384 (h chunks and the x window of a
 * workgroup share the 160 KB of LDS), else 0.
 * UNETRIR_EINVAL before the device is touched: a null pointer, B, K or N < 1, K unsupported, L outside 1 ... N + K - 1, a dry_stride
 * other than 0 or >= N (and a launch of more than 2^31 - 1 workgroups: B * ceil(L / 16384)). */
int unetrir_auralize_supported(int K);
int unetrir_auralize_f32(const float* rir, const float* dry, float* out, int B, int K, int N, long long dry_stride, int L,
                         unetrir_stream_t stream);

/* ---- the FFT form of auralization: the same y_b = h_b * x_b by uniform partitioned overlap-save, every transform in LDS
 *      (auralize_fft.hip, fft_lds.h; formulation and the derivation of the bound are in the former's header).
 *
 * unetrir_auralize_fft_f32: arguments and their rules as unetrir_auralize_f32, plus a workspace.  With the block P =
 * unetrir_auralize_fft_block(K) (2048 for every supported K, 0 otherwise), real transforms of 2P samples, Q = ceil(K / P) partitions
 * of h and J = ceil(L / P) output blocks anchored at n = 0:
 *   H_q = rfft(h_b[qP ... (q+1)P) | P zeros),   X_i = rfft(x_b[(i-1)P ... (i+1)P)) with zeros outside 0 <= m < N,
 *   Y_j = sum_{q <= min(j, Q-1)} H_q X_{j-q}, summed in ascending q in fp32 complex starting from +0,
 *   out[b][jP ... (j+1)P) = the last P samples of irfft(Y_j).
 * Two launches whatever B, N, L (the spectra of h and x; products, inverse and store), no atomics, no host synchronisation,
 * capturable; every element of out written exactly once and nothing beyond it.  With dry_stride = 0 the spectra of x are computed
 * once for all rows.  Twiddles are a table of fp32 values correctly rounded from an fp64 evaluation.
 * The bits of an element depend on (h_b, x_b, n) and the fixed block grid alone: not on the run, B, the row's place in the batch,
 * shared or per-row x, L (a truncated call returns the head of the full result, bit for bit) or N beyond the samples themselves
 * (x followed by explicit zeros gives the same bits).  They are NOT the direct form's, and the result is NOT exact on integer data.
 * A non-finite input sample spoils every output block its 2P-window or its partition feeds, not K outputs.
 * Error, per element n of block j, u = 2^-24, Q_j = min(j, Q-1) + 1:
 *   |out[b][n] - y_b[n]| <= u (19 log2(2P) + 8 + Q_j) sum_{q < Q_j} |h_b[qP ... (q+1)P)|_1 |x_b[(j-q-1)P ... (j-q+1)P)|_2
 * to first order in u (19 = 4.83 + 2 x 6.66 per radix-2 level rounded up: the componentwise error of H^ and the L2 errors of X^ and of
 * the inverse; 8: the rounding of the product, the split passes and the second-order terms); loose by orders of magnitude on random data.
 * unetrir_auralize_fft_supported(K): 1 for 1 <= K <= 16384, as the direct form.  ws: unetrir_auralize_fft_ws_bytes(B, K, N, dry_stride,
 * L) bytes = 16384 (B Q + (dry_stride ? B : 1) J), 16-byte aligned; 0 for arguments the call refuses.
 * UNETRIR_EINVAL before the device is touched: a null pointer (ws included), B, K or N < 1, K unsupported, L outside 1 ... N + K - 1, a
 * dry_stride other than 0 or >= N, ws too small or misaligned, more workgroups than a launch takes (B Q + (dry_stride ? B : 1) J or
 * B J above 2^31 - 8). */
int unetrir_auralize_fft_supported(int K);
int unetrir_auralize_fft_block(int K);
size_t unetrir_auralize_fft_ws_bytes(int B, int K, int N, long long dry_stride, int L);
int unetrir_auralize_fft_f32(const float* rir, const float* dry, float* out, int B, int K, int N, long long dry_stride, int L, void* ws,
                             size_t ws_bytes, unetrir_stream_t stream);

/* ---- a moving listener: dry audio rendered along a path of impulse responses by crossfaded overlap-save (auralize_fft.hip; the
 *      formulation, the gain arithmetic and the derivation of the bound are in its header).
 *
 * unetrir_auralize_path_f32: rir fp32 [B][R][K] (h_{b,r}: R nodes of a path, for each of B rows that move along one schedule); times
 * int32 [R] ON THE DEVICE (tau_r: the output sample at which the listener is at node r; may be negative or beyond L); dry, dry_stride,
 * out fp32 [B][L], N, L as unetrir_auralize_fft_f32.  With y_{b,r} = h_{b,r} * x_b the stationary convolution and 0 <= n < L:
 *   n <= tau_0:                out[b][n] = y_{b,0}[n]                    n >= tau_{R-1}:  out[b][n] = y_{b,R-1}[n]
 *   tau_r <= n < tau_{r+1}:    a = (n - tau_r) / (tau_{r+1} - tau_r),    out[b][n] = (1 - a) y_{b,r}[n] + a y_{b,r+1}[n]
 * a linear crossfade of the outputs with hat-function gains that sum to 1 (equal, being linear, to a filter interpolated per output
 * sample); R = 1 is the stationary case.
 * Two launches whatever B, R, N, L: (1) the spectra of the FFT form, over the B R responses and x (same packing, block P = 2048, grid
 * anchored at n = 0, a shared x transformed once); (2) one workgroup per row and output block j, which finds from `times` the nodes
 * whose gains touch the block (r_lo: the last with tau <= jP, else 0; r_hi: the first with tau >= (j+1)P - 1, else R - 1; indices
 * clamped into [0, R) whatever the table holds), forms for each in ascending r the stationary form's Y_j = sum_q H_q X_{j-q}, inverse
 * and 2^-12 scaling, and blends the samples in registers.  No intermediate y_r in memory, no atomics, nothing cleared, no host
 * synchronisation, capturable (times is read by the second launch, at replay); every element of out written exactly once and nothing
 * beyond it.
 * Gains are fp32: a = float(n - tau_r) / float(tau_{r+1} - tau_r) by IEEE division, the falling gain 1 - a; a node whose gain at a
 * sample is exactly 0 contributes nothing to it, a gain of 1 multiplies exactly; the blend is one product, then one fmaf, in ascending r.
 * The bits of an element depend on (h_{b,.}, x_b, times, n) and the fixed block grid alone: not on the run, B, the row's place in the
 * batch, shared or per-row x, L (a truncated call returns the head of the full result) or a larger workspace.  Wherever one node has
 * gain 1 - n <= tau_0, n >= tau_{R-1}, every n = tau_r, all of R = 1 - they are the bits of unetrir_auralize_fft_f32 for that response.
 * Error, with E_r[n] the bound of unetrir_auralize_fft_f32 for h_{b,r}, g_r[n] the exact gains and u = 2^-24:
 *   |out[b][n] - sum_r g_r[n] y_{b,r}[n]| <= sum_r g_r[n] E_r[n] + 4 u sum_r g_r[n] |y_{b,r}[n]|
 * (4: the division, the subtraction, the product and the fmaf; where a spacing is no power of two the falling gain inherits the
 * rounding of a, at most 2^-25 |y_r[n]| more).
 * Precondition: times strictly increasing and |tau| <= 2^30; otherwise the result is unspecified, but nothing outside out and ws is
 * read or written.  Cost: one product chain and one inverse transform per node that touches a block - 2 to 3 times the stationary
 * render for nodes at least P apart, more where they are denser.
 * unetrir_auralize_path_supported(K): 1 for 1 <= K <= 16384, as the FFT form.  ws: unetrir_auralize_path_ws_bytes(B, R, K, N,
 * dry_stride, L) bytes = 16384 (B R Q + (dry_stride ? B : 1) J), 16-byte aligned; 0 for arguments the call refuses.
 * UNETRIR_EINVAL before the device is touched: as unetrir_auralize_fft_f32, and R < 1, a null times, more workgroups than a launch
 * takes (B R Q + (dry_stride ? B : 1) J or B J above 2^31 - 8). */
int unetrir_auralize_path_supported(int K);
size_t unetrir_auralize_path_ws_bytes(int B, int R, int K, int N, long long dry_stride, int L);
int unetrir_auralize_path_f32(const float* rir, const int* times, const float* dry, float* out, int B, int R, int K, int N,
                              long long dry_stride, int L, void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- auralization block by block: the FFT form with its state carried between calls, and a response that can be exchanged while
 *      audio runs (auralize_fft.hip; the state layout and the launches are in its header).
 *
 * A stream renders y_b = h_b * x_b for a dry signal that arrives over time, P = 2048 samples (one block) or a multiple at a call.  With
 * Q = ceil(K / P), H_q and X_i as unetrir_auralize_fft_f32 and i, j counted from the first sample pushed since init:
 *   Y_j = sum_{q <= min(j, Q-1)} H_q X_{j-q}, ascending q from +0,   out block j = the last P samples of irfft(Y_j)
 * - the same formulation on the same block grid, with the last Q + max_blocks - 1 spectra of x kept in a ring (X_i in slot i mod S,
 * S = Q + max_blocks - 1) and the last P dry samples carried as the first half of the next window.
 * state: one opaque block of DEVICE memory, 16-byte aligned, unetrir_auralize_stream_state_bytes(B, K, dry_rows, max_blocks) bytes
 *   = 64 + 16384 (2 B Q + dry_rows S) + 8192 dry_rows
 * (control words; the spectra of the current response and of the one being faded in; the ring; the carry), 0 for arguments the calls
 * refuse.  dry_rows: 1 (one dry signal heard through all B responses) or B (one per row); 1 <= max_blocks <= 64: the most blocks one
 * push takes.  Everything that changes from call to call - the count of blocks rendered (64-bit), which response is current, whether a
 * fade is pending - lives in state, so the launch arguments of a push are the same every time: a push is capturable and a replay
 * renders the NEXT blocks from whatever the dry buffer holds then.  A larger state than advertised is accepted; the rest is not touched.
 *
 * unetrir_auralize_stream_init: rir fp32 [B][K].  Clears state (ring, carry, control) and writes the spectra of rir as the current
 *   response: a memset and one launch.  Calling it again restarts the stream (block 0, silence before it).
 * unetrir_auralize_stream_update: rir fp32 [B][K], a new response: its spectra go into the slot that is not current and a fade is marked
 *   pending; ONE launch.  The next push renders its first block through both responses and crossfades them linearly across that block
 *   (below); from the second block on the new response alone is heard, and it becomes the current one.  A second update before a push
 *   replaces the first: the last one wins.
 * unetrir_auralize_stream_push: consumes blocks P new dry samples per dry row, 1 <= blocks <= max_blocks, and writes the next blocks P
 *   output samples of every row into out fp32 [B][out_stride], out_stride >= blocks P.  dry fp32 [blocks P] with dry_stride = 0
 *   (dry_rows = 1) or [dry_rows][dry_stride], dry_stride >= blocks P; a NULL dry stands for zeros (to render the tail after the last
 *   sample; dry_stride is then not looked at).  THREE launches whatever B, K, blocks: (a) the spectra of the new windows into their ring slots; (b) one workgroup per row
 *   and pair of output blocks: products through the ring, inverse, store; (c) the last P dry samples into the carry, the count advanced
 *   by blocks and a pending fade completed - a launch of its own because the workgroups of (a) and (b) read what it writes.
 *   No atomics, no host synchronisation; nothing outside state and the blocks P samples per row of out is written, and every one of
 *   those samples exactly once.
 * The fade: with the update pending at block j, block j is the result of unetrir_auralize_path_f32 for the two nodes (old response at
 *   jP, new response at (j+1)P): out[n] = (1 - a) y_old[n] + a y_new[n], a = float(n - jP) / 2048 (exact), by that kernel's sequence -
 *   o = g y for the first node, o = fmaf(g, y, o) for the second, a gain of exactly 0 skipped.
 * Bits: block j of a stream that was never updated is block j of unetrir_auralize_fft_f32(rir, x, ..., L) for x = everything pushed so
 *   far (followed by zeros), bit for bit; after an update at block j the blocks from j on are those of unetrir_auralize_path_f32 with
 *   the two nodes above.  They do not depend on how the samples were divided into pushes, max_blocks, B, the row's place, shared or
 *   per-row dry, the run, or a larger state.  The error bounds are those of the two one-shot calls.
 * unetrir_auralize_stream_supported(K): 1 for 1 <= K <= 16384, as the FFT form.
 * UNETRIR_EINVAL before the device is touched: a null state, rir (init, update) or out (push); state not 16-byte aligned; state_bytes
 * below unetrir_auralize_stream_state_bytes(B, K, dry_rows, max_blocks) for the arguments given (so B, K, dry_rows and max_blocks
 * must be those the state was sized and initialised for: they are not stored where the host could compare them); B or K < 1, K
 * unsupported, dry_rows neither 1 nor B, max_blocks outside 1 ... 64; blocks outside 1 ... max_blocks; with a dry, a dry_stride that
 * is neither 0 with dry_rows = 1 nor >= blocks P; out_stride < blocks P; more workgroups than a launch takes (2 B Q + dry_rows S or
 * B max_blocks above 2^31 - 8). */
int unetrir_auralize_stream_supported(int K);
size_t unetrir_auralize_stream_state_bytes(int B, int K, int dry_rows, int max_blocks);
int unetrir_auralize_stream_init(void* state, size_t state_bytes, const float* rir, int B, int K, int dry_rows, int max_blocks,
                                 unetrir_stream_t stream);
int unetrir_auralize_stream_update(void* state, size_t state_bytes, const float* rir, int B, int K, int dry_rows, int max_blocks,
                                   unetrir_stream_t stream);
int unetrir_auralize_stream_push(void* state, size_t state_bytes, int B, int K, int dry_rows, int max_blocks, const float* dry,
                                 long long dry_stride, float* out, long long out_stride, int blocks, unetrir_stream_t stream);

/* ---- sample-rate conversion: a polyphase Kaiser-windowed sinc filter (resample.hip; the table is built on the host by
 *      resample_table.h, the tiling is in the former's header).
 *
 * The ratio rate_out / rate_in reduced to L / M (gcd 1), `zeros` zero crossings Z to each side, a rolloff and a Kaiser beta.  With
 * C = Z max(L, M), s = rolloff min(1, L / M) and W = C / L:
 *   h(tau) = s sinc(s tau) I0(beta sqrt(1 - (tau / W)^2)) / I0(beta)   for |tau| < W, else 0        (sinc(u) = sin(pi u) / (pi u))
 *   y[m] = sum_n h(m M / L - n) x[n]        0 <= m < ceil(N L / M),   x[n] = 0 outside 0 <= n < N
 * (librosa's output length, zero extension, gain 1 at DC both ways, exact phase: every phase is evaluated at its own argument).
 * The table fp32 [L][T], D = ceil(C / L), T = 2 D:  table[p][i] = h((p - (i - D + 1) L) / L), each entry evaluated in fp64 (I0: its
 * power series to convergence) and rounded once, exactly 0 outside the support (the integer test |p - (i - D + 1) L| < C); then
 *   y[m] = sum_{i=0}^{T-1} table[p][i] x[q - D + 1 + i]        (q, p) = divmod(m M, L).
 * unetrir_resample_supported(L, M, zeros): 1 for gcd(L, M) = 1, 1 <= L, M <= 2048, 1 <= zeros <= 64, T <= 8192 and L T <= 2^20, else 0.
 * unetrir_resample_taps: T (0: not supported).  unetrir_resample_out_length: ceil(N L / M) (0: an argument < 1, or beyond 2^62).
 * unetrir_resample_table_f32: table is a HOST array of L T floats; UNETRIR_EINVAL (nothing written) for a null table, an unsupported
 * (L, M, zeros), rolloff outside (0, 1] or beta outside [0, 32].
 *
 * unetrir_resample_f32: x fp32 [B][N], table fp32 [L][T] in DEVICE memory, out fp32 [B][Nout], 1 <= Nout <= ceil(N L / M) - a shorter
 * Nout returns the head of the full result.  The kernel does not interpret the table: T is even, the window of output m starts at
 * x[q - T/2 + 1], and any table may be passed.  One launch on the given stream: no workspace, no atomics, nothing cleared, no host
 * synchronisation (capturable); every element of out is written and nothing else.  Each output is ONE fp32 chain in ascending i from +0,
 *   y[m] = fmaf(table[p][T-1], x[q + T/2], ... fmaf(table[p][0], x[q - T/2 + 1], +0) ...),     x[n] = +0 outside the signal,
 * contraction off, so the bits of an element depend on (x_b, table, L, M, T, m) alone: not on the run, B, the row's place in the batch,
 * Nout or the tiling; on integer data whose partial sums stay below 2^24 the result is exact.  Inputs are taken to be finite.
 * UNETRIR_EINVAL before the device is touched: a null pointer; B, N or Nout < 1; Nout beyond ceil(N L / M); T odd, < 2 or > 8192;
 * gcd(L, M) != 1, L or M outside 1 ... 2048, L T > 2^20; N > 2^49 or B max(N, Nout) > 2^60 (index arithmetic stays within 63 bits);
 * more than 2^31 - 1 workgroups. */
int unetrir_resample_supported(int L, int M, int zeros);
int unetrir_resample_taps(int L, int M, int zeros);
long long unetrir_resample_out_length(long long N, int L, int M);
int unetrir_resample_table_f32(float* table, int L, int M, int zeros, double rolloff, double beta);
int unetrir_resample_f32(const float* x, const float* table, float* out, int B, long long N, int L, int M, int T, long long Nout,
                         unetrir_stream_t stream);

/* ---- scoring of generated impulse responses: the loss block of the evaluation loop (rir_generation.py:185-225) and its per-room
 *      bookkeeping (:227-290, :311-357), on the device and without a read-back.
 *
 * unetrir_eval_metrics_f32: pred / target fp32 NCHW [B][2][H][W] (plane 0 magnitude, plane 1 phase, normalised, padding included),
 * phase_ref nullable [B][2][H][W] = the network INPUT (diff_gen, :173-176, :190-193: the scored phase is pred + phase_ref, plane 1
 * of each, summed in fp32), wav_pred / wav_true fp32 [B][T], nullable as a pair.  out fp64 [B][7]:
 *   0 mean (target - pred)^2 over both planes, always the raw pred (:197)      1 the same over plane 0 (:195)
 *   2 mean over plane 1 of 1 - cos(2 pi (target - p)) (:36-40, :196)            3 20 log10(|pred0 - target0| / |target0|) (:203-205)
 *   4 mean (wav_true - wav_pred)^2 (:215)   5 the same over the first min(n50, T) samples (:218)
 *   6 20 log10(|wav_pred - wav_true| / |wav_true|) (:221-223);   4-6 are NaN without waveforms.
 * fp64 accumulation in a fixed order: the same bits in every run, and a sample's row does not depend on its batch.  A zero
 * numerator gives -inf dB (the reference raises), a zero denominator +inf, both NaN.
 *
 * unetrir_eval_accumulate: folds out [B][7] into acc fp64 [(G+1)][8] (in/out; row 0 global, rows 1..G the groups; columns 0-6
 * running sums of the figures - dB figures are summed as dB, :205-207, :316-317 - column 7 the sample count).  group int32 [B]:
 * the room of each sample, 0..G-1; any other value counts in the global row only.  One workgroup, batch walked in index order. */
int unetrir_eval_metrics_f32(const float* pred, const float* target, const float* phase_ref, int B, int H, int W,
                             const float* wav_pred, const float* wav_true, int T, int n50, double* out, unetrir_stream_t stream);
int unetrir_eval_accumulate(const double* out, const int* group, int B, int G, double* acc, unetrir_stream_t stream);

/* ---- room-acoustic figures of impulse responses: arrival of the direct sound, direct / reverberant and early / late balance, centre
 *      time and early decay time of the predicted and the true waveform, and their errors folded per room - on the device and
 *      without a read-back.  The waveforms are the reference's 0.2 s window (T = 9600 at 48 kHz): where a room's decay outlasts it,
 *      c50, ts and edt are figures of the truncated response - like for like between prediction and truth, not ISO 3382 values.
 *
 * unetrir_acoustic_figures_f32: wav_a fp32 [B][T], wav_b nullable fp32 [B][T] (the pair predicted / true in ONE launch),
 * fig fp64 [B][2][10], or [B][1][10] when wav_b is null.  With e = h*h in fp64, n0 = argmax |h| (lowest index on ties, |h| compared
 * as fp32), s = max(0, n0 - n_pre) and S[n] = sum_{k >= n} e[k] (the Schroeder backward integral), a row of fig is
 *   0 n0      1 E_tot = S[s]      2 E_dir = sum e, s <= n <= min(T-1, n0 + n_dir)      3 E_early = sum e, s <= n < min(T, s + n_early)
 *   4 M1 = sum_{n >= s} (n - s) e[n]      5 N_fit = #{n >= s : 10 S[n] >= E_tot} (the 0 .. -10 dB stretch, contiguous from s)
 *   6 drr = 10 log10(E_dir / (E_tot - E_dir)) dB      7 c50 = 10 log10(E_early / (E_tot - E_early)) dB
 *   8 ts = M1 / E_tot / fs * 1e3 ms      9 edt = -60 / slope s, slope = (N SkL - Sk SL) / (N Sk2 - Sk^2) * fs the least-squares line
 *   through L[k] = 10 log10(S[s+k] / E_tot), k = 0..N_fit-1 (Sk, Sk2 in closed form); NaN when N_fit < 2.
 * Degenerate rows follow IEEE arithmetic: an all-zero row gives NaN, no late energy +inf dB, a flat decay curve edt = -inf.
 * One workgroup per waveform, fp64 accumulation in a fixed order, no atomics, no workspace, one code path for every T >= 1: the same
 * bits in every run, and a waveform's row does not depend on its batch or its place in it.
 *
 * unetrir_acoustic_accumulate: the errors of the B (pred = fig[b][0], true = fig[b][1]) pairs,
 *   0 toa_ms = |n0_p - n0_t| / fs * 1e3   1 drr_db = |drr_p - drr_t|   2 c50_db = |c50_p - c50_t|   3 ts_ms = |ts_p - ts_t|
 *   4 edt_pct = 100 |edt_p - edt_t| / edt_t,
 * into err fp64 [B][5] (nullable; the IEEE value whether it counts or not) and folded into acc fp64 [(G+1)][20] (in/out; row 0
 * global, rows 1..G the groups; per figure four columns: sum of errors, sum of pred values, sum of true values, count; for toa the
 * values are n0 / fs * 1e3).  A figure of a pair counts only when both sides are finite - edt: and both > 0 - and the other figures
 * of that pair still count.  group int32 [B]: 0..G-1; any other value counts in the global row only.  One workgroup, batch walked
 * in index order.
 *
 * UNETRIR_EINVAL before the device is touched: a null required pointer, B <= 0, T <= 0, a negative window, fs <= 0, G < 0. */
int unetrir_acoustic_figures_f32(const float* wav_a, const float* wav_b, int B, int T, int n_pre, int n_dir, int n_early, double fs,
                                 double* fig, unetrir_stream_t stream);
int unetrir_acoustic_accumulate(const double* fig, const int* group, int B, int G, double fs, double* err, double* acc,
                                unetrir_stream_t stream);

/* ---- glue that would otherwise be framework kernels inside the step.
 * bn_inference_affine: BatchNormalization with training=False (rir_generation.py:165): scale = gamma * rsqrt(moving_var + eps),
 *   shift = beta - moving_mean * scale into affine[2*C] (gamma / beta NULL = 1 / 0), consumed by unetrir_bn_apply_*.
 * dropout_mask: the keep mask of Dropout(p) (dl_models/u_net.py:260), already scaled by 1/(1-p): element i of draw
 *   (seed, step) is a fixed function of (seed, step, i) (counter-based generator), so a step is reproducible.
 * index_to_i32: the int32 / int64 information-vector indices as the int32 array the embedding kernels read. */
int unetrir_bn_inference_affine_f32(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                                    float eps, int C, float* affine, unetrir_stream_t stream);
int unetrir_dropout_mask_f32(float* mask, long long n, float p, unsigned long long seed, unsigned long long step,
                             unetrir_stream_t stream);
int unetrir_index_to_i32(const void* idx, int elem_bytes, long long n, int* out, unetrir_stream_t stream);

/* ---- the variational autoencoder (dl_models/vae.py; main_training.py:142-152, :192-201, :257-265, :286-288): what it adds to the
 *      Autoencoder's graph.  fp32; L (latent_space_dim) a multiple of 4; mu / log_var / z / dz / dmu / dlv are [B][L] matrices with
 *      row strides ld_* >= L (multiples of 4), eps is dense [B][L].  Null pointers, B or L <= 0, L % 4 != 0 or a row stride
 *      shorter than L return UNETRIR_EINVAL before the device is touched.
 *
 * unetrir_normal_f32: the draw of SamplingLayer.call (vae.py:38, tf.keras.backend.random_normal(shape=(batch, dim))) as a
 *   counter-based generator - element i of draw (seed, step) is a fixed function of (seed, step, i), so a step is reproducible
 *   and a shorter draw is a prefix of a longer one.  The exact recipe (uint64 arithmetic wraps; GOLD = 0x9E3779B97F4A7C15,
 *   TAG = 0x4E4F524D414C3634; mix64 is the splitmix64 finaliser  z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *   z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^ z >> 31):
 *       key = mix64(mix64(seed * GOLD + step) ^ TAG)      the inner hash is the key of unetrir_dropout_mask_f32 for the same
 *                                                         (seed, step): the noise key is a hash of it, never equal to it
 *       r   = mix64(key + GOLD * (i + 1))                 one hash per output
 *       u1  = ((r >> 40) + 1) / 2^24   in (0, 1]          top 24 bits
 *       u2  = ((r >> 16) & 0xFFFFFF) / 2^24   in [0, 1)   the next 24 bits
 *       out = sqrt(-2 ln u1) * cos(2 pi u2)               Box-Muller in fp32: sqrtf(-2.f * logf(u1)) * cospif(2 u2)
 *   |out| <= sqrt(48 ln 2) = 5.77 (u1 = 2^-24).
 * unetrir_normal_dev_f32: the same draw with draw number *step_base + step_offset read from device memory (step_base = state + 2
 *   of unetrir_step_advance) - the contract of unetrir_dropout_mask_dev_f32: a captured step draws fresh noise on every replay.
 * unetrir_vae_sample_kl_fwd_f32: z = mu + exp(0.5 log_var) eps (vae.py:34-39) and the KL term:
 *   kl_out[1] = sum over all B * L elements of -0.5 (1 + log_var - mu^2 - exp(log_var))  (kl_loss_object, main_training.py:192-194;
 *   the train_loss_kl / val_loss_kl metrics average it, :286-288), kl_out[0] = inv_global_batch * kl_out[1] (compute_kl_loss,
 *   :196-201).  One workgroup, fp64 accumulation in a fixed order: two runs are bit-identical.  log_var is not clamped (the
 *   reference does not).
 * unetrir_vae_sample_kl_bwd_f32: d(loss)/d(mu), d(loss)/d(log_var) of the two Dense heads (vae.py:466-468) from dz = d(data term)/dz:
 *   dmu = dz + inv_global_batch mu;  dlv = dz 0.5 exp(0.5 log_var) eps + inv_global_batch 0.5 (exp(log_var) - 1).  Writes (never
 *   accumulates) both.
 * unetrir_vae_loss_add_f32: loss_out[0] += kl_out[0] - `loss += compute_kl_loss(mean, log_var)` (main_training.py:264-265) onto the
 *   scalar unetrir_sigmoid_loss_* wrote. */
int unetrir_normal_f32(float* out, long long n, unsigned long long seed, unsigned long long step, unetrir_stream_t stream);
int unetrir_normal_dev_f32(float* out, long long n, unsigned long long seed, const unsigned long long* step_base,
                           unsigned long long step_offset, unetrir_stream_t stream);
int unetrir_vae_sample_kl_fwd_f32(const float* mu, int ld_mu, const float* log_var, int ld_lv, const float* eps, int B, int L,
                                  float inv_global_batch, float* z, int ld_z, float* kl_out, unetrir_stream_t stream);
int unetrir_vae_sample_kl_bwd_f32(const float* mu, int ld_mu, const float* log_var, int ld_lv, const float* eps, const float* dz,
                                  int ld_dz, int B, int L, float inv_global_batch, float* dmu, int ld_dmu, float* dlv, int ld_dlv,
                                  unetrir_stream_t stream);
int unetrir_vae_loss_add_f32(const float* kl_out, float* loss_out, unetrir_stream_t stream);

/* ---- the vector quantiser of the VQ-VAE (dl_models/vqvae.py:42-98, VectorQuantizer; built at :514-518): nearest-code search,
 *      straight-through output, commitment + codebook loss, and the gradients of both into the layer's input and its codebook.
 *      PARITY UNPINNED (no TensorFlow here): a restatement of the source text, held to an fp64 restatement and finite differences.
 *      fp32 in both storage modes.  x / y / dy / dx are NHWC matrices of `rows` pixels with C channels and row strides ld_* >= C;
 *      `reshape(x, [-1, D])` (:65) cuts every pixel's C channels into C / D consecutive vectors: vector v = p * (C / D) + j starts
 *      at p * ld + j * D, nothing between C and ld is read or written.  E is the codebook `embeddings` [D][K] (:53-59), dense.
 *      N = rows * C, r = 1 / replicas (0 switches the loss term and its gradients off).
 *      UNETRIR_EINVAL before the device is touched: a null pointer; D % 4 != 0 or D outside [4, 64]; K % 4 != 0 or K outside
 *      [4, 512]; C % D != 0; a row stride < C or not a multiple of 4; rows <= 0 (or rows * C / D >= 2^31); x / y / dy / dx / ws not
 *      16-byte aligned; ws_bytes < unetrir_vq_ws_bytes().
 *
 * unetrir_vq_fwd_f32 (vqvae.py:61-98), ONE launch, one thread per vector, the codebook staged once per workgroup in LDS
 *   (K * (D + 1) * 4 + 2048 bytes: 18.4 KB at K = 256, D = 16; 135 KB at K = 512, D = 64), no distance or one-hot matrix in memory:
 *     idx[v] = the lowest k that minimises  dist_k = fl(n_k - 2 s_k)  (one fmaf), where
 *              s_k = x . E_k  accumulated by fmaf over d = 0 .. D-1 in that order from 0  (vqvae.py:89),
 *              n_k = ||E_k||^2 accumulated the same way, once per workgroup  (:92);
 *              the row-constant ||x||^2 of :91 is DROPPED from the comparison (it changes no argmin in exact arithmetic).
 *              Codes are visited in ascending k and replaced on a strictly smaller distance: ties go to the lowest k, as
 *              tf.argmin does (:97).  A vector with a NaN gets index 0.
 *     y      = fl(x + fl(E[:, idx] - x))   the straight-through output of :84 - two roundings, not E[:, idx]
 *     vq_out[1] = S = sum over all N elements of fl(fl(E[:, idx] - x)^2), summed in fp64: every thread adds its elements in
 *              order, a fixed tree per workgroup, the workgroups' partials (through ws) in a fixed order that depends on the
 *              geometry alone, rounded to fp32 once.  Two runs are bit-identical.
 *     vq_out[0] = fl(scale * vq_out[1]), scale = (float)(r (1 + beta) / N) formed in double: beta * commitment_loss +
 *              codebook_loss (:79-81) as it enters `loss += sum(model.losses) / replicas` (main_training.py:232-233).
 *   ws: unetrir_vq_ws_bytes() bytes that belong to the layer; its first 16 bytes must be zero before the first call and every
 *   call leaves them zero (the arrival counter by which the last workgroup learns that it combines the partials).
   Above 64 KB of LDS (K (D + 1) > 15 872) every call first raises the kernel's dynamic-LDS limit on the current device, a host-side
   call outside the stream: make one call at that size before capturing the layer into a HIP graph.
 * unetrir_vq_bwd_f32, TWO launches, writes (never accumulates) both gradients; dy = d(data term)/dy (straight-through):
 *     dx        = fmaf(cdx, fl(x - E[:, idx]), dy),  cdx = (float)(2 r beta / N)          elementwise
 *     dE[:, k]  = fl(cde * sum_{v : idx[v] == k} fl(E[:, k] - x_v)),  cde = (float)(2 r / N)
 *   the segmented sum without atomics and without a count or offset pass: one workgroup per code scans the indices; its wave w
 *   takes the vectors [64 w + 256 m, 64 w + 256 m + 64), m = 0, 1, ..., adds its matches in ascending vector order in fp32, and
 *   the four waves' partials are added in wave order.  A code nobody chose gets exactly 0.  Two runs are bit-identical.
 *   idx must be what unetrir_vq_fwd_f32 wrote; an index outside [0, K) is clamped for dx and matches no code for dE. */
size_t unetrir_vq_ws_bytes(void);
int unetrir_vq_fwd_f32(const float* x, long long rows, int ld, int C, int D, const float* E, int K, float beta, float r, int32_t* idx,
                       float* y, int ld_y, float* vq_out, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_vq_bwd_f32(const float* x, long long rows, int ld, int C, int D, const int32_t* idx, const float* E, int K, const float* dy,
                       int ld_dy, float beta, float r, float* dx, int ld_dx, float* dE, unetrir_stream_t stream);

/* ---- input staging for a host-fed train step (DataGenerator.__getitem__, datageneratorv2.py:64-102, hands over host arrays):
 *      for k < n: memcpy src[k] -> pinned[k] (page-locked staging owned by the caller), then an asynchronous host -> device copy
 *      pinned[k] -> dev[k] on `stream`.  One call per batch from the producer thread: the foreign call runs without the
 *      interpreter lock, so staging a batch does not hold the lock the thread that launches the step takes ~300 times per step. */
int unetrir_stage_h2d(int n, const void* const* src, void* const* pinned, void* const* dev, const size_t* bytes,
                      unetrir_stream_t stream);

/* ---- a training batch out of the device-resident data set, in one launch: the two loops over `dataset.__getitem__` and the
 *      three np.stack calls of DataGenerator.__getitem__ (datageneratorv2.py:64-102) as a gather.
 *      bank fp32 [N][2][H][W] (row_elems = 2 H W: the padded features of every file), emb_bank int32 [N][emb_len], wav_bank
 *      nullable fp32 [N][wav_len] (the decoded waveforms), room_bank nullable int32 [N]; idx_in / idx_out int32 [B] IN DEVICE
 *      MEMORY: the sample numbers of the input and of the target position of each pair.
 *        spec_in[b] = bank[idx_in[b]]   spec_out[b] = bank[idx_out[b]]   contiguous NCHW fp32 [B][2][H][W], the engine's boundary
 *        emb[b][0] = emb_bank[idx_in[b]]   emb[b][1] = emb_bank[idx_out[b]]          int32 [B][2][emb_len] (:91)
 *        wav_true[b] = wav_bank[idx_out[b]]   room[b] = room_bank[idx_out[b]]        nullable; the target position (what the
 *                                                                                    evaluation scores, rir_generation.py:160-293)
 *      A streaming copy: 16 bytes per lane when row_elems % 4 == 0 and bank / spec_in / spec_out are 16-byte aligned (wav_len and
 *      the waveform pointers likewise, independently), 4 bytes per lane otherwise - the only entry point that takes unaligned
 *      buffers.  Nothing outside the outputs is written.
 *      THE INDICES ARE TRUSTED: the kernel reads row idx of every bank without a range check (N is only validated as a
 *      geometry argument).  The generator produces its index table on the host, checks it against N there, once per epoch,
 *      and uploads it; a caller of this entry point owes the same check.
 *      UNETRIR_EINVAL before the device is touched: a null required pointer (bank, emb_bank, idx_in, idx_out, spec_in, spec_out,
 *      emb), B, N, row_elems or emb_len <= 0, wav_true without wav_bank or the reverse (or wav_len <= 0 with them), room without
 *      room_bank, more than 2^31 - 1 workgroups of 16 KB ((2 ceil(row_elems / 4096) + ceil(wav_len / 4096)) B). */
int unetrir_gather_batch_f32(const float* bank, long long N, long long row_elems, const int32_t* emb_bank, int emb_len,
                             const float* wav_bank, long long wav_len, const int32_t* room_bank, const int32_t* idx_in,
                             const int32_t* idx_out, int B, float* spec_in, float* spec_out, int32_t* emb, float* wav_true,
                             int32_t* room, unetrir_stream_t stream);

/* ---- Griffin-Lim reconstruction from the magnitude alone: PostProcess.griffinlim (postprocess.py:47-50, :130-131,
 *      librosa.griffinlim(S, hop_length, win_length)), the `algorithm='gl'` branch of rir_generation.py:62, :137, :424 - a whole
 *      batch in one call.  PARITY UNPINNED like the feature transforms above: librosa 0.9.x's loop at its defaults,
 *          S = magnitude plane of feat [B][2][H][W], first n_bins x n_frames block, denormalised (denormalize) and NOT clamped;
 *          angles = exp(2 pi i u);  rebuilt = 0;
 *          n_iter times:  tprev = rebuilt;  rebuilt = stft(istft(S angles));
 *                         angles = rebuilt - momentum / (1 + momentum) tprev;  angles /= |angles| + 1e-16;
 *          wav [B][hop_length (n_frames - 1)] = istft(S angles),
 *      stft / istft being exactly the centred Hann pair of unetrir_stft_features_f32 / unetrir_istft_features_f32 (pad_mode 0 =
 *      'reflect', 1 = 'constant').  librosa holds `angles` in complex64; here every state (angles, rebuilt, tprev, the
 *      intermediate frames - all in ws) and all arithmetic are fp64, and the only fp32 values are feat, init_phase and the one
 *      rounding of wav.  n_iter = 0 gives istft(S angles0).
 *      momentum is read as the shortest decimal that rounds to the float given (0.99f means librosa's double 0.99, not
 *      0.9900000095...: the difference reaches the waveform at ~1e-7 of its peak after 32 iterations).
 *      u: init_phase fp32 [B][n_bins][n_frames] in turns, [0, 1) - angles0 = (cospi(2u), sinpi(2u)) in fp64 - or, when it is
 *      NULL, draw (seed, draw) of unetrir_uniform_f32 over that shape.
 *      2 n_iter + 3 launches on `stream` whatever B is; no allocation, no memset, no host synchronisation (capturable in a HIP
 *      graph); fixed summation orders and no atomics: two runs are bit-identical.
 *      UNETRIR_EINVAL before the device is touched: the geometry rules of unetrir_istft_features_f32, n_iter < 0, a negative or non-finite momentum,
 *      pad_mode outside {0, 1}, a null feat / wav / ws, ws_bytes < unetrir_griffinlim_ws_bytes (0 for an invalid geometry).
 *
 * unetrir_uniform_f32: the `rng.rand` of librosa.griffinlim's init='random' as the uniform sibling of unetrir_normal_f32 -
 *   element i of draw (seed, step) is a fixed function of (seed, step, i), a shorter draw is a prefix of a longer one.  Same GOLD
 *   and mix64 as there; TAG = 0x554E4946524D3634:
 *       key = mix64(mix64(seed * GOLD + step) ^ TAG);   r = mix64(key + GOLD * (i + 1));   out = (r >> 40) / 2^24   in [0, 1). */
size_t unetrir_griffinlim_ws_bytes(int B, int n_bins, int n_frames, int n_fft);
int unetrir_griffinlim_f32(const float* feat, int B, int H, int W, int n_bins, int n_frames, int n_fft, int win_length,
                           int hop_length, int pad_mode, int denormalize, int n_iter, float momentum, const float* init_phase,
                           unsigned long long seed, unsigned long long draw, float* wav, void* ws, size_t ws_bytes,
                           unetrir_stream_t stream);
int unetrir_uniform_f32(float* out, long long n, unsigned long long seed, unsigned long long step, unetrir_stream_t stream);

/* ---- the FFT form of the Griffin-Lim reconstruction (griffinlim_fft.hip): the definition above unchanged - the same S, angles0, loop,
 *      window pair, envelope rule, trimming, pad modes, reading of momentum, init_phase / (seed, draw) - with fp32 state and fp32 FFTs
 *      held in LDS (csrc/fft_lds.h) in place of fp64 state and fp64 DFTs.  That is the precision librosa itself keeps its angles in.
 *      The iteration amplifies rounding (fastest with momentum), so there is NO bound per element: measured, the waveform stays within
 *      1e-7 ... 1e-4 of the peak of the fp64 form's and reconstructs the magnitude equally well.  unetrir_griffinlim_f32 is
 *      the form to hold a result to a bound; this one is for evaluation runs, which pay the loop on every batch.
 *      State in ws, all fp32, [b][f][k]: S (the fp64 value of the DFT form rounded once) and three complex planes that take turns as
 *      rebuilt, tprev and the plane being written; angles0 = the fp32 rounding of (cospi(2u), sinpi(2u)) taken in fp64.  S angles is not
 *      stored: every synthesis forms it in its loader as S n(rebuilt - alpha tprev), n(a) = a / (hypotf(a) + 1e-16f), alpha = the fp32
 *      rounding of momentum / (1 + momentum) (launch 0: S angles0; launch 1: tprev = 0).
 *      n_iter + 2 launches on `stream` whatever B is: init, one launch per iteration (a workgroup inverse-transforms the frames that
 *      reach its own frames' windows, overlap-adds them into a run of the waveform in LDS - ascending frame order per sample, fp32 - and
 *      transforms its own frames forward: the intermediate waveform and the windowed frames never reach memory), and a last synthesis
 *      that stores wav.  No allocation, no memset, no host synchronisation (capturable in a HIP graph); fixed summation orders and no
 *      atomics: two runs are bit-identical, and a row's bits depend neither on B nor on its place in the batch.
 *      unetrir_griffinlim_fft_supported: n_fft in {128, 256, 512, 1024}; n_bins = n_fft / 2 + 1; n_frames >= 2; 2 <= win_length <=
 *      n_fft (any value); hop_length >= 1 and 4 hop_length >= win_length (at most four frames reach a sample); hop_length (n_frames -
 *      1) > n_fft / 2 (one reflection reaches into the waveform; asked of both pad modes); hop_length n_frames + n_fft <= 2^31 - 1.
 *      unetrir_griffinlim_fft_ws_bytes = 28 B n_frames n_bins rounded up to a multiple of 8 (7 fp32 planes), 0 for anything
 *      unsupported or B outside 1 ... 65535.
 *      UNETRIR_EINVAL before the device is touched: an unsupported geometry, B outside 1 ... 65535, n_bins > H, n_frames > W,
 *      n_iter < 0, a negative or non-finite momentum, pad_mode outside {0, 1}, a null feat / wav / ws, ws not 8-byte aligned,
 *      ws_bytes < unetrir_griffinlim_fft_ws_bytes. */
int unetrir_griffinlim_fft_supported(int n_bins, int n_frames, int n_fft, int win_length, int hop_length);
size_t unetrir_griffinlim_fft_ws_bytes(int B, int n_bins, int n_frames, int n_fft, int win_length, int hop_length);
int unetrir_griffinlim_fft_f32(const float* feat, int B, int H, int W, int n_bins, int n_frames, int n_fft, int win_length,
                               int hop_length, int pad_mode, int denormalize, int n_iter, float momentum, const float* init_phase,
                               unsigned long long seed, unsigned long long draw, float* wav, void* ws, size_t ws_bytes,
                               unetrir_stream_t stream);

/* ---- output head behind UpSampling2D((2, 2)) (dl_models/u_net.py:247-248, resize_factor_0 = [2, 2]) without the up-sampled tensor
 *      (head_up2.hip): nearest-neighbour x2 followed by Conv2D(2, (6,6), 'same') is a 4x4 'same' convolution (pad 1 before, 2 after)
 *      with 8 output channels (o, a, b) on the coarse grid [B][h][w][C] followed by depth-to-space:
 *          logit[o][2i+a][2j+b] = bias[o] + sum_{u,v,c} K'[(o,a,b)][u][v][c] * x[i+u-1][j+v-1][c]
 *          K'[(o,a,b)][u][v][c] = sum_{dh: (a+dh)>>1 == u} sum_{dw: (b+dw)>>1 == v} K[o][dh][dw][c]      (dh outer, dw inner, ascending)
 *      h, w are the COARSE sizes; the fine grid is [B][2h][2w].  C % 8 == 0.  fp32 accumulation, no atomics.
 *      unetrir_head_up2_supported_*: mask of the passes served for C input channels - 1 forward, 2 data gradient, 4 weight gradient.
 *      fold: w the fp32 master [>=2][6][6][C] (rows 0, 1 read) -> wf fp32 [8][4][4][C], summed in fp32 in the order above; round_bf16 != 0
 *      (the work copy of a bf16 trunk): each sum rounded to bf16 once and stored as that value.
 *      fwd: x [B*h*w][ldx]; wf the folded copy; bias fp32 [>=2] or NULL; y fp32 logits [B*2h*2w][ldy] exactly as unetrir_head6x6_fwd_*
 *      writes them (ldy >= 2; with ldy >= 4 channels 2, 3 zeroed, further ones untouched): the depth-to-space is in the store.
 *      dgrad: dy [B*2h*2w][lddy >= 2] (channels 0, 1 read) -> dx [B*h*w][lddx], columns [0, C) written (rounded once for bf16), no addend.
 *      wgrad: dw[0..1][6][6][C] in the layout of the master (unfold, the transpose of fold, included: a outer, b inner); further rows of a
 *      padded kernel gradient are left untouched.  One slab of partial sums per workgroup in ws (>= unetrir_head_up2_wgrad_ws_bytes,
 *      0 for unsupported arguments), reduced in slab order by a second launch, unfolded by a third; the slab count depends on
 *      (B, h, w, C) alone.  The bias gradient is unetrir_colsum_* of the fine dlogits.
 *      x, wf, dx, dw, ws 16-byte aligned; UNETRIR_EINVAL otherwise, before the device is touched. */
int unetrir_head_up2_supported_f32(int C);
int unetrir_head_up2_supported_bf16(int C);
int unetrir_head_up2_fold(const float* w, int C, float* wf, int round_bf16, unetrir_stream_t stream);
int unetrir_head_up2_fwd_f32(const float* x, int ldx, int B, int h, int w, int C, const float* wf, const float* bias, float* y, int ldy,
                             unetrir_stream_t stream);
int unetrir_head_up2_fwd_bf16(const unetrir_bf16* x, int ldx, int B, int h, int w, int C, const float* wf, const float* bias, float* y,
                              int ldy, unetrir_stream_t stream);
int unetrir_head_up2_dgrad_f32(const float* dy, int lddy, int B, int h, int w, const float* wf, int C, float* dx, int lddx,
                               unetrir_stream_t stream);
int unetrir_head_up2_dgrad_bf16(const unetrir_bf16* dy, int lddy, int B, int h, int w, const float* wf, int C, unetrir_bf16* dx, int lddx,
                                unetrir_stream_t stream);
size_t unetrir_head_up2_wgrad_ws_bytes(int B, int h, int w, int C);
int unetrir_head_up2_wgrad_f32(const float* x, int ldx, int B, int h, int w, int C, const float* dy, int lddy, float* dw, void* ws,
                               size_t ws_bytes, unetrir_stream_t stream);
int unetrir_head_up2_wgrad_bf16(const unetrir_bf16* x, int ldx, int B, int h, int w, int C, const unetrir_bf16* dy, int lddy, float* dw,
                                void* ws, size_t ws_bytes, unetrir_stream_t stream);

/* ---- the room classifier deep_CNN (dl_models/cnn_clas.py:19-53; cnn_clas.hip), fp32 storage, direct arithmetic, no atomics.
 *      Conv2D(3x3, strides 1, padding='valid', activation='relu') (cnn_clas.py:25, :31, :37).  g->H, g->W are the INPUT size (>= 3),
 *      the output is (H - 2) x (W - 2); g->k = 3, g->stride = 1; g->Cin in {4, 16, 32} (4: the two input channels zero-padded as
 *      unetrir_nchw_to_nhwc_pad_f32 writes them), g->Cout in {16, 32, 64}.
 *      fwd:   y = conv(x, w) + bias, max(., 0) when relu != 0; w [Cout][3][3][Cin].
 *      dgrad: dx = the adjoint applied to dy, or to dy * [y > 0] when relu != 0 (y = the stored forward output, may be NULL
 *             otherwise); wt [Cin][3][3][Cout]; ALL of dx [B*H*W][lddx] is written, the two border rings included.
 *      wgrad: dw [Cout][3][3][Cin] and dbias [Cout] from the same (masked) dy.  Partial sums over slabs of whole output rows go to ws
 *             (>= unetrir_conv3x3_valid_wgrad_ws_bytes, 0 for an unsupported geometry) and are added in a fixed order; the split
 *             depends on g alone: with R = B (H - 2) output rows, slabs of ceil(R / min(R, 524288 / (Cin Cout))) rows, each holding
 *             [Cout][3][3][Cin] + [Cout] floats.  Zero input channels (the padding of the first layer) get a zero gradient.
 *      AveragePooling2D(2x2, strides 2, 'valid') (cnn_clas.py:28, :34) of x [B][H][W][C] -> y [B][H/2][W/2][C], H, W >= 2, C % 4 == 0.
 *      affine (nullable): the [2 C] scale / shift unetrir_bn_stats_f32 writes - y = pool(x) * scale + shift, which equals the pooled
 *      BatchNormalization output because the affine is per channel.  bwd: dx [B][H][W][C] = dy / 4 in every pixel of a cell and
 *      exactly 0 in a trailing odd row or column; with BatchNormalization in front, unetrir_bn_bwd_f32 (relu = 0) follows on dx.
 *      GlobalAveragePooling2D (cnn_clas.py:40): y [B][C] = sum over the h w pixels in a fixed order, times 1 / (h w), with the
 *      same optional affine; C <= 1024.  bwd: dx = dy / (h w) in every pixel.
 *      Dense(classes, softmax) + categorical_crossentropy (cnn_clas.py:49, :63) on logits [B][ldl >= classes], 1 <= classes <= 1024:
 *      ce:  probs [B][classes] = softmax; with CE_b = -sum_c y_c log p_c taken as the log-softmax of the max-subtracted logits
 *           (no clipping of p), loss_out[0] = inv_norm sum_b CE_b, loss_out[1] = sum_b CE_b, loss_out[2] = 0; dlogits [B][ldd] =
 *           (p_c sum_k y_k - y_c) inv_norm, columns [classes, ldd) zero; acc_out[0] = rows with argmax(logits) == argmax(target), the
 *           lowest index on ties on both sides, as fp32.  target [B][classes]: one-hot or soft rows.  One workgroup, fp64 row sums.
 *      fwd: probs only.  bwd: dlogits = p_c (dprobs_c - sum_k dprobs_k p_k) from an upstream gradient on the probabilities.
 *      UNETRIR_EINVAL before the device is touched: geometry outside the above, a null required pointer, a pixel stride smaller than
 *      its channel count or no multiple of 4, a pointer of a 16-byte access that is not 16-byte aligned, a workspace too small. */
int unetrir_conv3x3_valid_fwd_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* w, const float* bias, int relu,
                                  float* y, int ldy, unetrir_stream_t stream);
int unetrir_conv3x3_valid_dgrad_f32(const unetrir_conv_geom* g, const float* dy, int lddy, const float* y, int ldy, int relu,
                                    const float* wt, float* dx, int lddx, unetrir_stream_t stream);
size_t unetrir_conv3x3_valid_wgrad_ws_bytes(const unetrir_conv_geom* g);
int unetrir_conv3x3_valid_wgrad_f32(const unetrir_conv_geom* g, const float* x, int ldx, const float* dy, int lddy, const float* y,
                                    int ldy, int relu, float* dw, float* dbias, void* ws, size_t ws_bytes, unetrir_stream_t stream);
int unetrir_avgpool2_fwd_f32(const float* x, int ldx, int B, int H, int W, int C, const float* affine, float* y, int ldy,
                             unetrir_stream_t stream);
int unetrir_avgpool2_bwd_f32(const float* dy, int lddy, int B, int H, int W, int C, float* dx, int lddx, unetrir_stream_t stream);
int unetrir_gap_fwd_f32(const float* x, int ldx, int B, int H, int W, int C, const float* affine, float* y, int ldy,
                        unetrir_stream_t stream);
int unetrir_gap_bwd_f32(const float* dy, int lddy, int B, int H, int W, int C, float* dx, int lddx, unetrir_stream_t stream);
int unetrir_softmax_ce_f32(const float* logits, int ldl, const float* target, int B, int classes, float inv_norm, float* probs,
                           float* dlogits, int ldd, float* loss_out, float* acc_out, unetrir_stream_t stream);
int unetrir_softmax_fwd_f32(const float* logits, int ldl, int B, int classes, float* probs, unetrir_stream_t stream);
int unetrir_softmax_bwd_f32(const float* probs, const float* dprobs, int B, int classes, float* dlogits, int ldd,
                            unetrir_stream_t stream);

/* ---- profiling hooks used by bench.py: when enabled every conv launch is bracketed by HIP
 *      events on its own stream; collect() synchronises those events and returns, per kernel
 *      family, launch count, total milliseconds and total algorithmic FLOPs.  Process-global
 *      (one mutex-protected record list); off by default; the second piece of global state. */
#define UNETRIR_PROF_FAMILIES 8
enum { UNETRIR_FAM_CONV_FWD = 0, UNETRIR_FAM_CONV_DGRAD = 1, UNETRIR_FAM_CONV_WGRAD = 2,
       UNETRIR_FAM_BN = 3, UNETRIR_FAM_OTHER = 4, UNETRIR_FAM_SMALL_CHANNEL = 5,
       UNETRIR_FAM_DOMINANT = 6 /* launches served by the dominant kernel of the bf16 step (conv3x3p), counted here IN ADDITION to their
                                   forward / data-gradient family */ };
int unetrir_prof_enable(int on);      /* 0: off, 1: every family, 2: forward convolutions only (fewer events in the stream) */
int unetrir_prof_collect(int* counts, double* ms, double* flops);

#ifdef __cplusplus
}
#endif
#endif /* UNETRIR_H */
