"""AENet (dl_models/ae_net.py) on graph.GraphEngine: the U-Net skeleton - five encoder levels, skip concats, convolutional_block_1
units, feature-block modes 0-3, the 6x6 head - with `Conv2D` / `Conv2DTranspose(k=2, strides=2)` in place of the strided pair
(:273-279, :301-307; csrc/conv2x2.hip on a bf16 trunk), the autoencoder family's bottleneck - Flatten || Dense of the information
vector -> Dense -> Dropout -> Reshape -> 1x1 conv (:224-228, :253-268) - and a clipped-ReLU output `relu(out, max_value=1)` (:249).
PARITY UNPINNED like every graph here: the pin is tests/aenet_ref.py, a restatement of the source text.
"""
from .unet_graph import UNetGraphEngine

AE_VOCAB, AE_EMB_DIM = 2500, 256          # Embedding(2500, 256) (dl_models/ae_net.py:264)
AE_VEC_UNITS = 64 * 32                    # Dense(64*32) (:266)


class AENetEngine(UNetGraphEngine):
    """One replica of AENet for a fixed per-replica batch size.  Level 1 is Conv2D(F0, 2, strides=1) on the padded input (TF pads
    bottom / right by 1; the tap-table kernel), levels 2-5 and the decoder's way up are the 2x2 stride-2 layers, which alone carry
    l2(0.001).  Two Dropout(.5) layers, two masks per step (MASKS, in graph order).  H and W must halve exactly four times."""
    n_dropout_draws = 2
    dropout_p = 0.5               # Dropout(.5) (dl_models/ae_net.py:258, :267)
    output_act = "relu1"
    MASKS = ("vec", "rec")

    def __init__(self, H, W, B, F0=32, mode=0, batchnorm=True, inf_vector_shape=(2, 16), device="cuda:0", n_replicas=1,
                 runtime=None, share=None, dtype="f32", overlap_wgrad=False, generic_conv2x2=False):
        """generic_conv2x2: keep every 2x2 stride-2 layer on the tap-table kernels (A/B measurements)."""
        if H % 16 or W % 16:
            raise ValueError(f"AENet needs H and W to be multiples of 16 (four exact halvings), got {H} x {W}")
        self.generic_conv2x2 = generic_conv2x2
        super().__init__(H, W, B, F0=F0, k=2, depth=4, mode=mode, batchnorm=batchnorm, inf_vector_shape=inf_vector_shape, device=device,
                         n_replicas=n_replicas, runtime=runtime, share=share, dtype=dtype, overlap_wgrad=overlap_wgrad)

    def _build(self):
        """AENet._build (dl_models/ae_net.py:197-251)."""
        D, ch = self.depth, self.ch
        x = self._input()
        skips = []
        for l in range(1, D + 2):
            c = ch[l - 1]
            if l == 1:
                d = self._conv(x, "enc1.down", c, 2, 1, followed_by_bn=False, pad_in=self.PAD, l2=True)
            else:
                d = self._conv2x2(x, f"enc{l}.down", c, generic=self.generic_conv2x2)
            if l <= D:         # the block output is the skip: written straight into the lower half of the concat buffer
                cat = self._new(d.a.H, d.a.W, 2 * c)
                skip, up = self._view(cat, 0, c), self._view(cat, c, c)
                x = self._feature_block(d, f"enc{l}", out=skip)
                skips.append((cat, up))
            else:
                x = self._feature_block(d, f"enc{l}")
        h5, w5, cL = x.a.H, x.a.W, x.a.C
        # vector_block (:263-268), concatenate([Flatten(enc5), vec]) (:225-226), recover_shape (:253-261)
        v = self._dense(self._embedding(self.n_idx, "vec.embedding", vocab=AE_VOCAB, dim=AE_EMB_DIM), "vec.dense", AE_VEC_UNITS)
        cat = self._concat(x, self._dropout(v, "vec"))
        r = self._dropout(self._dense(cat, "rec.dense", h5 * w5 * 2), "rec")
        x = self._conv(self._pad2(r, h5, w5), "rec.conv", cL, 1, 1, followed_by_bn=False, pad_in=4, l2=False)
        if self.dtype == "bf16":
            x = self._cast(x)                       # the Dense branch is fp32, the trunk bf16
        for l in range(D, 0, -1):
            c = ch[l - 1]
            cat, up = skips[l - 1]
            self._conv2x2(x, f"dec{l}.up", c, transpose=True, out=up, generic=self.generic_conv2x2)
            a = self._conv_bn_relu(cat, f"dec{l}.cb1a", c, 3)
            x = self._feature_block(a, f"dec{l}")
        self.logits = self._head6x6(x, "head")

    def forward(self, spec, emb, dropout_mask=None, target=None, global_batch=None, alpha=0.9):
        """dropout_mask: the pair make_dropout_mask() returns (None: no Dropout)."""
        if target is not None:
            self._check_batch(target, "target")
        self.load_input(spec, emb)
        self.masks["vec"], self.masks["rec"] = (None, None) if dropout_mask is None else dropout_mask
        self.run_forward()
        return self.loss_or_sigmoid(target, global_batch, alpha)

    def make_dropout_mask(self, generator=None):
        """One keep mask per Dropout layer, in graph order, each as wide as the node it multiplies."""
        return tuple(self.dropout_mask(self.mask_width[n], generator, slot).view(self.B, 1, 1, -1) for slot, n in enumerate(self.MASKS))
