"""VQ-VAE (dl_models/vqvae.py) on the HIP kernels: the Autoencoder's conv / conv-transpose stack with a vector quantiser at the
bottleneck - Dense -> Dropout -> Reshape(h, w, 2) -> Conv2D(1x1) -> VectorQuantizer (vqvae.py:490-520) - whose output, a feature
map, is what the decoder's first transposed convolution reads (:333-371).  Built on ae.AEFamilyEngine; its own kernels are
csrc/vq.hip (search + straight-through output + loss term in one launch, the input and codebook gradients in two).
PARITY UNPINNED like the rest of the family: a restatement of the source text (tests/vqvae_ref.py), not a run of it.
"""
import torch

from . import ops
from .ae import AEFamilyEngine
from .graph import RELU, Node

VQ_BETA = 0.25           # VectorQuantizer(beta=0.25) (dl_models/vqvae.py:43); the model passes no other (:516)
VQ_VOCAB, VQ_EMB_DIM = 1500, 128          # Embedding(1500, 128) (:453)


class VQVAEEngine(AEFamilyEngine):
    """One replica of VQVAE for a fixed per-replica batch size (constructor mirrors dl_models/vqvae.py:107-116; DEFAULTS is the
    model of its __main__ block, :522-531 - main_training.py does not build this class).

    The quantiser has no `training` switch (:61-85): inference quantises too.  It is fp32 in both storage modes; a bf16 trunk is
    cast behind it.  Its loss term beta * commitment + codebook loss (:79-81) is a model loss: `loss += sum(model.losses) /
    replicas` (main_training.py:232-233).  With a target, forward() adds it - vq_out[0], already divided by n_replicas - to
    loss_out[0] on the device, and backward(include_reg=False) leaves its gradients out as it does those of the l2 terms.  The
    include_reg switch governs the GRADIENTS only: the value in loss_out[0] carries the term whatever the switch says (it is
    formed in the forward pass, before backward() is told), and reg_loss() does not carry it - it stays the l2 sum, which is 0
    here (no kernel_regularizer anywhere in vqvae.py: l2_names is empty) - so Trainer.last_loss() = loss_out[0] + reg_out[0]
    counts the term once.
    vq_out = (the term as it enters the loss, S = sum (q - x)^2 over this replica's elements); vq_indices: the chosen codes,
    int32 [B * h * w * C / latent_space_dim] in the order of tf.reshape(x, [-1, embedding_dim]) (:65)."""
    n_dropout_draws = 1          # Dropout(.3) behind the bottleneck Dense (vqvae.py:511): the model's only one
    MASKS = ("bottleneck", None)
    DEFAULTS = ((32, 64, 128, 256), 16, 320)

    def _build(self):
        """dl_models/vqvae.py:316-520."""
        x = self._conv_encoder(self._input(), l2=False)                       # Conv2D -> BN -> ReLU, no regularizer (:469-488)
        h, w, c = self.shape_before_bottleneck = (x.a.H, x.a.W, x.a.C)
        D, K = self.latent, c                                               # VectorQuantizer(conv_filters[-1], latent_space_dim) (:516)
        if c % D or not 4 <= D <= 64 or not 4 <= K <= 512:
            raise ValueError("the quantiser needs conv_filters[-1] % latent_space_dim == 0, 4 <= latent_space_dim <= 64, conv_filters[-1] <= 512")
        if (h * w * 2) % 4:
            raise ValueError("the bottleneck Dense(h * w * 2) needs an even number of bottleneck pixels")
        # information vector (:445-455): Embedding -> Dense on the UNFLATTENED [B, 2, 16, 128] tensor, i.e. per position; no Dropout;
        # Flatten at the join (:505)
        cat = self._join_vector_per_position(x, "encoder_inf_dense", VQ_VOCAB, VQ_EMB_DIM)
        d = self._dropout(self._dense(cat, "dense", h * w * 2), self.MASKS[0])        # Dense(prod(shape)) -> Dropout(.3) (:508-511)
        q = self._vq(self._conv(self._pad2(d, h, w), "conv2d", c, 1, 1, followed_by_bn=False, pad_in=4, l2=False), K, D)   # (:512-518)
        self._latent, self._n_enc_ops = q, len(self.ops)                     # model.encoder ends at the quantiser's output (:434)
        if self.dtype == "bf16":
            q = self._cast(q)                                               # the quantiser is fp32, the transposed-conv trunk bf16
        self._conv_decoder(q, RELU, l2=False)                               # no Dense / Dropout / Reshape at the entry (:343-423)

    def _vq(self, x: Node, K, D):
        """VectorQuantizer (:42-98) over the fp32 node x; the codebook `embeddings` [D, K] is an ordinary parameter."""
        name = "vector_quantizer.embeddings"
        self._param(name, (D, K), "codebook", (D, K))
        y = self._new(x.a.H, x.a.W, x.a.C, f32=True)
        self._vq_in = x
        self.vq_elems = x.a.P * x.a.C                        # N: the elements the two means run over, per replica and step
        self.vq_indices = torch.zeros(self.vq_elems // D, dtype=torch.int32, device=self.device)
        self.vq_out = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._vq_ws = ops.vq_workspace(self.device)

        def fwd():
            ops.vq_fwd(x.a, D, self.p[name], VQ_BETA, 1.0 / self.n_replicas, self.vq_indices, y.a, self.vq_out, self._vq_ws)

        def bwd():           # straight-through: dx = dy + the commitment term's gradient; writes both
            ops.vq_bwd(x.a, D, self.vq_indices, self.p[name], y.g, VQ_BETA, (1.0 / self.n_replicas) if self.include_reg else 0.0,
                       x.g, self.g[name])
            x.g_set = True
        self._push(fwd, bwd)
        return y

    # ------------------------------------------------------------------ passes
    def forward(self, spec, emb, dropout_mask=None, target=None, global_batch=None, alpha=0.9):
        """model.decoder(model.encoder([spec, emb])) (vqvae.py:330).  dropout_mask: the bottleneck keep mask make_dropout_mask()
        returns.  With a target, loss_out[0] ends as compute_loss + the quantiser's model loss / replicas; loss_out[1:3] keep
        their meaning; vq_out holds the term alone."""
        pred = super().forward(spec, emb, self._mask_pair(dropout_mask)[1], None, target, global_batch, alpha)
        if target is not None:
            ops.vae_loss_add(self.vq_out, self.loss_out)
        return pred

    def loss_from_logits(self, target, global_batch=None, alpha=0.9):
        raise NotImplementedError("the VQ-VAE's loss has the quantiser's term, which is formed in the forward pass: drive it with "
                                  "Trainer.step / forward(..., target=)")

    def encode(self, spec, emb, dropout_mask=None, global_batch=None):
        """model.encoder([spec, emb]) (vqvae.py:434): the quantised tensor, NHWC [B, h, w, conv_filters[-1]] (a copy)."""
        m = self._mask_pair(dropout_mask)[1]
        return super().encode(spec, emb, None if m is None else (m, None), global_batch)

    def make_dropout_mask(self, generator=None):
        (mask,) = super().make_dropout_mask(generator)
        return mask.view(self.B, 1, 1, -1)       # the shape of the node it multiplies
