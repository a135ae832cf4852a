"""The reference's autoencoder family on graph.GraphEngine: what Autoencoder (dl_models/autoencoder.py), ResAE (resae.py) and VAE
(vae.py) have in common - AEFamilyEngine - and the Autoencoder itself: the conv / conv-transpose BatchNorm-ReLU stack with a Dense
latent that main_training.py:118-129 builds for name == "ae" (SURVEY.md 8(f) rank 4).  No kernel of its own.
"""
import math

import torch

from .graph import GraphEngine, Node, RELU


class AEFamilyEngine(GraphEngine):
    """One replica of an encoder -> Dense latent -> decoder model for a fixed per-replica batch size.  The three models share the
    constructor surface of their reference classes, the information vector joined to the flattened encoder output, the decoder
    entry (Dense -> Dropout -> Reshape), the padded two-channel output layer, and forward / encode / decode over one op list cut
    at the latent node.  A subclass writes `_build` from these pieces and names its two Dropout layers in MASKS."""
    n_dropout_draws = 2               # two Dropout layers: two masks per step
    MASKS = (None, "dec")             # names in self.masks of the encoder-side Dropout and the decoder's (None: there is none)
    DEFAULTS = None                   # (conv_filters, latent_space_dim, n_neurons) main_training.py builds the model with

    def __init__(self, H, W, B, conv_filters=None, conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2), latent_space_dim=None,
                 n_neurons=None, inf_vector_shape=(2, 16), device="cuda:0", n_replicas=1, runtime=None, share=None, dtype="f32",
                 overlap_wgrad=False):
        """Mirrors dl_models/autoencoder.py:41-46, res_ae.py:41-50, vae.py:48-57; an argument left None takes the class's DEFAULTS."""
        super().__init__(B, device, n_replicas, runtime, share, dtype, overlap_wgrad)
        filters, latent, neurons = self.DEFAULTS
        self.H, self.W = H, W
        self.filters = tuple(filters if conv_filters is None else conv_filters)
        self.kernels, self.strides = tuple(conv_kernels), tuple(conv_strides)
        self.latent = latent if latent_space_dim is None else latent_space_dim
        self.n_neurons = neurons if n_neurons is None else n_neurons
        if any(f % 4 for f in self.filters) or any(s not in (1, 2) for s in self.strides):
            raise ValueError("conv_filters must be multiples of 4 and conv_strides 1 or 2")
        if self.latent % 4 or self.n_neurons % 4:
            raise ValueError("latent_space_dim and n_neurons must be multiples of 4")
        self.inf_vector_shape = tuple(inf_vector_shape)
        self.n_idx = int(math.prod(self.inf_vector_shape))
        self._build()
        self._finalize_params()
        self._alloc_outputs()

    # ------------------------------------------------------------------ pieces of _build
    def _conv_encoder(self, x: Node, l2):
        """Conv2D -> BatchNormalization -> ReLU per level (autoencoder.py:384-402, vae.py:432-451; the VAE has no kernel_regularizer)."""
        for i in range(len(self.filters)):
            c = self._conv(x, f"encoder_conv_layer_{i + 1}", self.filters[i], self.kernels[i], self.strides[i], False,
                           pad_in=self.PAD if i == 0 else 0, l2=l2)
            x = self._bn_act(c, f"encoder_bn_{i + 1}", RELU)
        return x

    def _join_vector(self, x: Node, name, dropout=None):
        """concatenate([Flatten(x), y]) with y = Embedding -> Flatten -> Dense(n_neurons) `name` (-> Dropout `dropout`) of the
        information vector (autoencoder.py:357-369, :404-417; res_ae.py:411-420, :516-530; vae.py:407-418, :462-465)."""
        self.shape_before_bottleneck = (x.a.H, x.a.W, x.a.C)
        vec = self._dense(self._embedding(self.n_idx), name, self.n_neurons)
        if dropout is not None:
            vec = self._dropout(vec, dropout)
        return self._concat(x, vec)

    def _join_vector_per_position(self, x: Node, name, vocab, dim):
        """concatenate([Flatten(x), Flatten(y)]) with y = Embedding(vocab, dim) -> Dense(n_neurons) `name` on the UNFLATTENED
        [B, *inf_vector_shape, dim] tensor, i.e. per position: a 1x1 convolution over the positions with a Dense layer's Keras
        layout; no Dropout; Flatten at the join (vqvae.py:445-455, :505; diff_vae.py:416-417, :463-465)."""
        self.shape_before_bottleneck = (x.a.H, x.a.W, x.a.C)
        e = self._reshape(self._embedding(self.n_idx, vocab=vocab, dim=dim), 1, self.n_idx, dim)
        v = self._conv(e, name, self.n_neurons, 1, 1, followed_by_bn=False, l2=False)
        (kspec,) = [s_ for s_ in self.specs_fwd if s_.name == name + ".kernel"]
        kspec.kind, kspec.keras_shape = "dense", (dim, self.n_neurons)
        return self._concat(x, self._reshape(v, 1, 1, self.n_idx * self.n_neurons))

    def _decoder_entry(self, z: Node):
        """model.encoder ends at `z`; the decoder opens with Dense -> Dropout -> Reshape (autoencoder.py:245-265, res_ae.py:247-268,
        vae.py:294-313)."""
        self._latent, self._n_enc_ops = z, len(self.ops)
        h, w, c = self.shape_before_bottleneck
        d = self._dense(z, "decoder_dense", h * w * c)
        x = self._reshape(self._dropout(d, self.MASKS[1]), h, w, c)
        if self.dtype == "bf16":
            x = self._cast(x)                                  # the Dense branch is fp32, the transposed-conv trunk bf16
        return x

    def _conv_decoder(self, x: Node, act, l2):
        """Conv2DTranspose -> BatchNormalization -> activation: a stride-1 layer, then the encoder's levels mirrored
        (autoencoder.py:267-320: ReLU, l2; vae.py:315-367: LeakyReLU, no regularizer), then the output layer."""
        n = len(self.filters)
        ct = self._conv(x, "decoder_conv_transpose_layer_0", self.filters[-1], self.kernels[-1], 1, True, l2=l2)
        x = self._bn_act(ct, "decoder_bn_0", act)
        for layer_index in reversed(range(1, n)):
            num = n - layer_index
            ct = self._conv(x, f"decoder_conv_transpose_layer_{num}", self.filters[layer_index - 1], self.kernels[layer_index - 1],
                            self.strides[layer_index - 1], True, l2=l2)
            x = self._bn_act(ct, f"decoder_bn_{num}", act)
        self._output_layer(x, f"decoder_out_{n}")

    def _output_layer(self, x: Node, name):
        """_add_decoder_output (autoencoder.py:322-335, res_ae.py:373-389, vae.py:369-385): Conv2DTranspose(2, k0, s0, 'same') in front
        of the sigmoid; Cout padded 2 -> PAD, no l2."""
        self.logits = self._conv(x, name, 2, self.kernels[0], self.strides[0], True, followed_by_bn=False, pad_out=self.PAD, l2=False)
        if (self.logits.a.H, self.logits.a.W) != (self.H, self.W):
            raise ValueError("decoder output size does not match the input size")

    # ------------------------------------------------------------------ passes
    @staticmethod
    def _mask_pair(dropout_mask):
        """(encoder-side mask, decoder mask) of what make_dropout_mask() returned: a pair, or the decoder's mask alone."""
        if isinstance(dropout_mask, (tuple, list)):
            return (dropout_mask[0] if len(dropout_mask) > 1 else None), dropout_mask[-1]
        return None, dropout_mask

    def _latent_shape(self):
        """What model.encoder returns, from the latent node: [B, latent_space_dim] for a Dense latent, NHWC [B, h, w, C] for a
        feature map (vqvae.VQVAEEngine)."""
        a = self._latent.a
        return (self.B, a.C) if a.H == a.W == 1 else (self.B, a.H, a.W, a.C)

    def _prepare_forward(self, global_batch):
        """Called between the input conversion and the op list of forward / encode (VAEEngine draws its noise here)."""

    def forward(self, spec, emb, mask_a=None, mask_b=None, target=None, global_batch=None, alpha=0.9, dropout_mask=None):
        """mask_a, mask_b: the keep masks of the two Dropout layers MASKS names; dropout_mask: the same as make_dropout_mask()
        returns them (the trainer's calling convention)."""
        if dropout_mask is not None:
            mask_a, mask_b = self._mask_pair(dropout_mask)
        if target is not None:
            self._check_batch(target, "target")
        self.load_input(spec, emb)
        if self.MASKS[0] is not None:
            self.masks[self.MASKS[0]] = mask_a
        if self.MASKS[1] is not None:
            self.masks[self.MASKS[1]] = mask_b
        self._prepare_forward(global_batch)
        self.run_forward()
        return self.loss_or_sigmoid(target, global_batch, alpha)

    def encode(self, spec, emb, dropout_mask=None, global_batch=None):
        """model.encoder([spec, emb]) (autoencoder.py:337-346, res_ae.py:62, :391-403): the latent vector [B, latent_space_dim] (a copy)."""
        self.load_input(spec, emb)
        if self.MASKS[0] is not None:
            self.masks[self.MASKS[0]] = self._mask_pair(dropout_mask)[0]
        self._prepare_forward(global_batch)
        self.run_forward(0, self._n_enc_ops)
        return self._latent.a.base.view(self._latent_shape()).clone()

    def decode(self, z, dropout_mask=None):
        """model.decoder(z) (autoencoder.py:222-233, res_ae.py:63, :233-245, vae.py:274-284): z [B, latent_space_dim] -> prediction
        [B,2,H,W] (NCHW buffer)."""
        shape = self._latent_shape()
        if tuple(z.shape) != shape or z.dtype != torch.float32:
            raise ValueError(f"z must be float32 [{','.join(str(n) for n in shape)}]")
        self._latent.a.base.view(shape).copy_(z)
        if self.MASKS[1] is not None:
            self.masks[self.MASKS[1]] = self._mask_pair(dropout_mask)[1]
        self.run_forward(self._n_enc_ops, None)
        return self.loss_or_sigmoid(None, None, 0.9)

    def make_dropout_mask(self, generator=None):
        """One keep mask per Dropout layer MASKS names, in that order, each as wide as the node it multiplies."""
        names = [n for n in self.MASKS if n is not None]
        return tuple(self.dropout_mask(self.mask_width[n], generator, slot) for slot, n in enumerate(names))


class AutoencoderEngine(AEFamilyEngine):
    """Autoencoder (dl_models/autoencoder.py:210-417): Dropout on the information vector and behind decoder_dense."""
    MASKS = ("inf", "dec")
    DEFAULTS = ((64, 128, 256, 512), 64, 2048)

    def _build(self):
        x = self._conv_encoder(self._input(), l2=True)
        z = self._dense(self._join_vector(x, "encoder_inf_dense", dropout="inf"), "encoder_output", self.latent)
        self._conv_decoder(self._decoder_entry(z), RELU, l2=True)
