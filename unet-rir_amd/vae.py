"""VAE (dl_models/vae.py) on the HIP kernels: the variational autoencoder main_training.py:142-152 builds for name == "vae" - the
Autoencoder's conv / conv-transpose stack with two Dense heads (`mu`, `log_variance`) on the bottleneck, the sampling layer
z = mu + exp(0.5 log_var) eps, a KL term in the loss (main_training.py:192-201, :264-265) and LeakyReLU in the decoder.  Built on
ae.AEFamilyEngine; its own kernels are csrc/vae.hip (the normal draw, the fused sampling + KL forward and backward).
"""
import torch

from . import ops
from .ae import AEFamilyEngine
from .graph import LEAKY


class VAEEngine(AEFamilyEngine):
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

    MASKS = (None, "dec")
    DEFAULTS = ((64, 128, 256, 512), 64, 2048)

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        B = self.B
        self.kl_elems = B * self.latent                           # elements the *_loss_kl metrics average over, per replica and step
        self._inv_gb = 1.0 / B
        self._eps_buf = torch.empty((B, self.latent), dtype=torch.float32, device=self.device)
        self._eps_now = self._eps_buf
        # kl_out[0] = compute_kl_loss (sum / global batch), kl_out[1] = the raw sum of kl_loss_object over every (b, l) element
        self.kl_out = torch.zeros(4, dtype=torch.float32, device=self.device)
        self.masks["eps"] = None

    def _build(self):
        """dl_models/vae.py:257-472."""
        x = self._conv_encoder(self._input(), l2=False)
        cat = self._join_vector(x, "encoder_inf_dense")            # no Dropout on the information vector (:407-418)
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
        self._mu, self._lv = mu, lv
        self._conv_decoder(self._decoder_entry(z), LEAKY, l2=False)          # model.encoder ends at z (:387-396)

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

    def _prepare_forward(self, global_batch):
        self._inv_gb = 1.0 / (self.B if global_batch is None else global_batch)
        self._take_eps()

    def forward(self, spec, emb, dropout_mask=None, target=None, global_batch=None, alpha=0.9):
        """model.decoder(model.encoder([spec, emb])[0]) (vae.py:265-272).  dropout_mask: the decoder keep mask make_dropout_mask()
        returns.  With a target, loss_out[0] ends as compute_loss + compute_kl_loss (main_training.py:263-265) with the KL sum divided
        by `global_batch` (default: this replica's batch); loss_out[1:3] keep their meaning; kl_out holds the KL term alone."""
        pred = super().forward(spec, emb, None, self._mask_pair(dropout_mask)[1], target, global_batch, alpha)
        if target is not None:
            ops.vae_loss_add(self.kl_out, self.loss_out)
        return pred

    def loss_from_logits(self, target, global_batch=None, alpha=0.9):
        raise NotImplementedError("the VAE's loss has a KL term that is formed in the forward pass: drive it with Trainer.step / "
                                  "forward(..., target=)")

    def encode(self, spec, emb, dropout_mask=None, global_batch=None):
        """model.encoder([spec, emb]) (vae.py:387-396, :472): (z, mean, log_var), each [B, latent_space_dim] (copies).  Draws eps."""
        z = super().encode(spec, emb, dropout_mask, global_batch)
        return (z,) + tuple(n_.a.base.view(self.B, self.latent).clone() for n_ in (self._mu, self._lv))

    def make_dropout_mask(self, generator=None):
        (mask,) = super().make_dropout_mask(generator)
        return mask.view(self.B, 1, 1, -1)       # the shape of the node it multiplies
