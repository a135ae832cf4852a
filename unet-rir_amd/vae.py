"""VAE (dl_models/vae.py) on the HIP kernels: the variational autoencoder main_training.py:142-152 builds for name == "vae" - the
Autoencoder's conv / conv-transpose stack with two Dense heads (`mu`, `log_variance`) on the bottleneck, the sampling layer
z = mu + exp(0.5 log_var) eps, a KL term in the loss (main_training.py:192-201, :264-265) and LeakyReLU in the decoder.  Built on
graph.GraphEngine; its own kernels are csrc/vae.hip (the normal draw, the fused sampling + KL forward and backward).
"""
import math

import torch

from . import ops
from .graph import GraphEngine, Node, LEAKY, RELU


class VAEEngine(GraphEngine):
    """One replica of VAE for a fixed per-replica batch size (constructor mirrors dl_models/vae.py:48-57).

    eps is drawn on EVERY forward pass, training or not: SamplingLayer.call (vae.py:34-39) has no `training` switch, so
    `model.model(..., training=False)` of rir_generation.py:165 samples too.  The draw does not depend on the trainer's `dropout`
    flag either.  It is counted in the dropout masks' draw counter (`n_noise_draws` beside `n_dropout_draws`): steps never reuse
    noise, a captured step draws fresh noise on every replay, a checkpoint resumes the sequence, replicas draw from per-rank
    seeds.  `self.masks["eps"]` (float32 [B, latent] on the device), when set, is used instead of the engine's own draw (tests,
    reproducibility); the draw number is consumed all the same.
    There is no kernel_regularizer anywhere in vae.py: l2_names is empty, reg_loss() yields 0."""
    n_dropout_draws = 1          # Dropout(.3) behind decoder_dense (vae.py:303); none on the information-vector branch (:407-418)
    n_noise_draws = 1            # eps of the sampling layer (vae.py:38)

    def __init__(self, H, W, B, conv_filters=(64, 128, 256, 512), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2),
                 latent_space_dim=64, n_neurons=2048, inf_vector_shape=(2, 16), device="cuda:0", n_replicas=1, runtime=None,
                 share=None, dtype="f32", overlap_wgrad=False):
        super().__init__(B, device, n_replicas, runtime, share, dtype, overlap_wgrad)
        self.H, self.W = H, W
        self.filters, self.kernels, self.strides = tuple(conv_filters), tuple(conv_kernels), tuple(conv_strides)
        if any(f % 4 for f in self.filters) or any(s not in (1, 2) for s in self.strides):
            raise ValueError("conv_filters must be multiples of 4 and conv_strides 1 or 2")
        if latent_space_dim % 4 or n_neurons % 4:
            raise ValueError("latent_space_dim and n_neurons must be multiples of 4")
        self.latent, self.n_neurons = latent_space_dim, n_neurons
        self.inf_vector_shape = tuple(inf_vector_shape)
        self.n_idx = int(math.prod(self.inf_vector_shape))
        self.kl_elems = B * self.latent                           # elements the *_loss_kl metrics average over, per replica and step
        self._inv_gb = 1.0 / B
        self._eps_buf = torch.empty((B, self.latent), dtype=torch.float32, device=self.device)
        self._eps_now = self._eps_buf
        # kl_out[0] = compute_kl_loss (sum / global batch), kl_out[1] = the raw sum of kl_loss_object over every (b, l) element
        self.kl_out = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.masks["eps"] = None
        self._build()
        self._finalize_params()
        self._alloc_outputs()

    def _build(self):
        """dl_models/vae.py:257-472."""
        B = self.B
        n = len(self.filters)
        self.x4 = self._reg(Node(ops.new_act(B, self.H, self.W, self.PAD, self.device, dtype=self.adt), needs_grad=False))
        x = self.x4
        for i in range(n):        # encoder: Conv2D -> BatchNormalization -> ReLU (:432-451); no kernel_regularizer
            c = self._conv(x, f"encoder_conv_layer_{i + 1}", self.filters[i], self.kernels[i], self.strides[i], False,
                           pad_in=self.PAD if i == 0 else 0, l2=False)
            x = self._bn_act(c, f"encoder_bn_{i + 1}", RELU)
        h, w, c = x.a.H, x.a.W, x.a.C
        self.shape_before_bottleneck = (h, w, c)
        n_feat = h * w * c
        flat_vec = self._embedding(self.n_idx)                  # Embedding -> Flatten -> Dense, no Dropout (:407-418)
        vec = self._dense(flat_vec, "encoder_inf_dense", self.n_neurons)
        # concatenate([Flatten(x), Flatten(y)]) (:462-465); the concat is a copy of two row blocks into an fp32 node
        cat = self._new(1, 1, n_feat + self.n_neurons, f32=True)
        x_last = x

        def cat_fwd():
            cat.a.base.view(B, -1)[:, :n_feat].copy_(x_last.a.base.view(B, -1))
            cat.a.base.view(B, -1)[:, n_feat:].copy_(vec.a.base.view(B, -1))

        def cat_bwd():
            x_last.g.base.view(B, -1).copy_(cat.g.base.view(B, -1)[:, :n_feat]); x_last.g_set = True
            vec.g.base.view(B, -1).copy_(cat.g.base.view(B, -1)[:, n_feat:]); vec.g_set = True
        self._push(cat_fwd, cat_bwd)
        # the two heads read the same node (:466-468): its gradient is the sum of their data gradients (first writes, second adds)
        mu = self._dense(cat, "mu", self.latent)
        lv = self._dense(cat, "log_variance", self.latent)
        z = self._new(1, 1, self.latent, f32=True)

        def sample_fwd():          # SamplingLayer (:34-39, :470) + kl_loss_object / compute_kl_loss (main_training.py:192-201)
            ops.vae_sample_kl_fwd(mu.a, lv.a, self._eps_now, self._inv_gb, z.a, self.kl_out)

        def sample_bwd():
            ops.vae_sample_kl_bwd(mu.a, lv.a, self._eps_now, z.g, self._inv_gb, mu.g, lv.g)
            mu.g_set = lv.g_set = True
        self._push(sample_fwd, sample_bwd)
        self._mu, self._lv, self._latent, self._n_enc_ops = mu, lv, z, len(self.ops)          # model.encoder ends here (:387-396)
        d = self._dense(z, "decoder_dense", n_feat)               # decoder: Dense -> Dropout -> Reshape (:294-313)
        dd = self._dropout(d, "dec")
        x = self._reshape(dd, h, w, c)
        if self.dtype == "bf16":
            x = self._cast(x)                                  # the Dense branch is fp32, the transposed-conv trunk bf16
        ct = self._conv(x, "decoder_conv_transpose_layer_0", self.filters[-1], self.kernels[-1], 1, True, l2=False)      # stride 1 (:315-333)
        x = self._bn_act(ct, "decoder_bn_0", LEAKY)
        for layer_index in reversed(range(1, n)):                 # _add_conv_transpose_layers (:335-367)
            num = n - layer_index
            ct = self._conv(x, f"decoder_conv_transpose_layer_{num}", self.filters[layer_index - 1], self.kernels[layer_index - 1],
                            self.strides[layer_index - 1], True, l2=False)
            x = self._bn_act(ct, f"decoder_bn_{num}", LEAKY)
        # _add_decoder_output (:369-385): Conv2DTranspose(2, k0, s0, 'same') + sigmoid; Cout padded 2 -> 4
        self.logits = self._conv(x, f"decoder_out_{n}", 2, self.kernels[0], self.strides[0], True, followed_by_bn=False, pad_out=self.PAD,
                                 l2=False)
        if (self.logits.a.H, self.logits.a.W) != (self.H, self.W):
            raise ValueError("decoder output size does not match the input size")

    # ------------------------------------------------------------------ the sampling layer's noise
    def _take_eps(self):
        """eps of this forward pass: masks["eps"] when supplied, else the next draw of the engine's stream.  One draw number is
        consumed either way, so the host counter and the device counter (trainer: n_dropout_draws + n_noise_draws per step) agree."""
        given = self.masks.get("eps")
        dev = self._dev()
        if given is not None:
            if tuple(given.shape) != (self.B, self.latent) or given.dtype != torch.float32 or not given.is_contiguous():
                raise ValueError(f"eps must be a contiguous float32 [{self.B},{self.latent}] tensor")
            self._eps_now = given
        else:
            if dev is None:
                ops.normal(self._eps_buf, self.dropout_seed, self._shared["dropout_step"])
            else:
                ops.normal_dev(self._eps_buf, self.dropout_seed, dev["state"], dev["offset"])
            self._eps_now = self._eps_buf
        if dev is not None:
            dev["offset"] += 1
        self._shared["dropout_step"] += 1

    def _load(self, spec, emb):
        B = self.B
        if tuple(spec.shape) != (B, 2, self.H, self.W) or spec.dtype != torch.float32 or not spec.is_contiguous():
            raise ValueError(f"spec must be a contiguous float32 [{B},2,{self.H},{self.W}] tensor")
        self.set_indices(emb)
        self._last_spec = spec
        ops.nchw_to_nhwc_pad(spec, self.x4.a)

    @staticmethod
    def _dec_mask(dropout_mask):
        if isinstance(dropout_mask, (tuple, list)):
            return dropout_mask[-1]
        return dropout_mask

    def forward(self, spec, emb, dropout_mask=None, target=None, global_batch=None, alpha=0.9):
        """model.decoder(model.encoder([spec, emb])[0]) (vae.py:265-272).  dropout_mask: the decoder keep mask make_dropout_mask()
        returns.  With a target, loss_out[0] ends as compute_loss + compute_kl_loss (main_training.py:263-265) with the KL sum divided
        by `global_batch` (default: this replica's batch); loss_out[1:3] keep their meaning; kl_out holds the KL term alone."""
        self._load(spec, emb)
        self.masks["dec"] = self._dec_mask(dropout_mask)
        self._inv_gb = 1.0 / (self.B if global_batch is None else global_batch)
        self._take_eps()
        self.run_forward()
        pred = self.loss_or_sigmoid(self.logits, target, global_batch, alpha)
        if target is not None:
            ops.vae_loss_add(self.kl_out, self.loss_out)
        return pred

    def loss_from_logits(self, target, global_batch=None, alpha=0.9):
        raise NotImplementedError("the VAE's loss has a KL term that is formed in the forward pass: drive it with Trainer.step / "
                                  "forward(..., target=)")

    def encode(self, spec, emb, dropout_mask=None, global_batch=None):
        """model.encoder([spec, emb]) (vae.py:387-396, :472): (z, mean, log_var), each [B, latent_space_dim] (copies).  Draws eps."""
        self._load(spec, emb)
        self._inv_gb = 1.0 / (self.B if global_batch is None else global_batch)
        self._take_eps()
        self.run_forward(0, self._n_enc_ops)
        B, L = self.B, self.latent
        return tuple(n_.a.base.view(B, L).clone() for n_ in (self._latent, self._mu, self._lv))

    def decode(self, z, dropout_mask=None):
        """model.decoder(z) (vae.py:274-284): z [B, latent_space_dim] -> prediction [B,2,H,W] (NCHW buffer)."""
        if tuple(z.shape) != (self.B, self.latent) or z.dtype != torch.float32:
            raise ValueError(f"z must be float32 [{self.B},{self.latent}]")
        self._latent.a.base.view(self.B, self.latent).copy_(z)
        self.masks["dec"] = self._dec_mask(dropout_mask)
        self.run_forward(self._n_enc_ops, None)
        return self.loss_or_sigmoid(self.logits, None, None, 0.9)

    def make_dropout_mask(self, generator=None):
        h, w, c = self.shape_before_bottleneck
        return self.dropout_mask(h * w * c, generator, 0).view(self.B, 1, 1, h * w * c)       # the shape of the node it multiplies
