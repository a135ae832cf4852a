"""DiffUNet (dl_models/diff_u_net.py) on graph.GraphEngine: the generator that predicts a phase DIFFERENCE (rir_generation.py:51-63,
:173-176; main_training.py:214-217).  AENet's skeleton - five encoder levels on `Conv2D` / `Conv2DTranspose(k=2, strides=2)`, skip
concats, convolutional_block_1 units, feature-block modes 0-3 - with the U-Net's bottleneck join `Add()([encoding_5_out, vector_out])`
(:228) of a vector block without a 1x1 convolution (:251-260) and a LINEAR two-channel 1x1 head (:247): a difference of two phases
in [0, 1] lies in [-1, 1], which neither a sigmoid nor a clipped ReLU can put out.  The head's kernels on a bf16 trunk are
csrc/head1x1.hip.  PARITY UNPINNED like every graph here: the pin is tests/diffunet_ref.py, a restatement of the source text.
"""
from .unet_graph import UNetGraphEngine

DIFF_VOCAB, DIFF_EMB_DIM = 1500, 128          # Embedding(1500, 128) (dl_models/diff_u_net.py:255)


class DiffUNetEngine(UNetGraphEngine):
    """One replica of DiffUNet for a fixed per-replica batch size.  Level 1 is Conv2D(F0, 2, strides=1) on the padded input (TF pads
    bottom / right by 1; the tap-table kernel), levels 2-5 and the decoder's way up are the 2x2 stride-2 layers, which with level 1
    alone carry l2(0.001) (:266-272, :294-300).  One Dropout(.5) layer (:258).  H and W must halve exactly four times.
    head_passes: the passes of the head that run on csrc/head1x1.hip (bf16 trunk), as c22_passes records the 2x2 layers'."""
    n_dropout_draws = 1
    dropout_p = 0.5               # Dropout(.5) (dl_models/diff_u_net.py:258)
    output_act = "linear"         # Conv2D(2, (1, 1), activation='linear') (:247)
    MASKS = ("vec",)

    def __init__(self, H, W, B, F0=32, mode=0, batchnorm=True, inf_vector_shape=(2, 16), device="cuda:0", n_replicas=1,
                 runtime=None, share=None, dtype="f32", overlap_wgrad=False, generic_conv2x2=False, generic_head=False):
        """generic_conv2x2, generic_head: keep every 2x2 stride-2 layer / the head on the tap-table kernels (A/B measurements)."""
        if H % 16 or W % 16:
            raise ValueError(f"DiffUNet needs H and W to be multiples of 16 (four exact halvings), got {H} x {W}")
        self.generic_conv2x2, self.generic_head = generic_conv2x2, generic_head
        super().__init__(H, W, B, F0=F0, k=2, depth=4, mode=mode, batchnorm=batchnorm, inf_vector_shape=inf_vector_shape, device=device,
                         n_replicas=n_replicas, runtime=runtime, share=share, dtype=dtype, overlap_wgrad=overlap_wgrad)

    def _build(self):
        """DiffUNet._build (dl_models/diff_u_net.py:200-249)."""
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
        # vector_block (:251-260): Embedding -> Flatten -> Dense(h5 w5 16 F0) -> Dropout(.5) -> Reshape; no 1x1 convolution behind it
        v = self._dense(self._embedding(self.n_idx, "vec.embedding", vocab=DIFF_VOCAB, dim=DIFF_EMB_DIM), "encoder_inf_dense", h5 * w5 * cL)
        x = self._add(x, self._reshape(self._dropout(v, "vec"), h5, w5, cL))          # Add()([encoding_5_out, vector_out]) (:228)
        for l in range(D, 0, -1):
            c = ch[l - 1]
            cat, up = skips[l - 1]
            self._conv2x2(x, f"dec{l}.up", c, transpose=True, out=up, generic=self.generic_conv2x2)
            a = self._conv_bn_relu(cat, f"dec{l}.cb1a", c, 3)
            x = self._feature_block(a, f"dec{l}")
        # UpSampling2D((1, 1)) is the identity (:246)
        self.logits = self._head1x1(x, "head", generic=self.generic_head)
        self.vec_dim = h5 * w5 * cL

    def make_dropout_mask(self, generator=None):
        """The keep mask of the vector block's Dropout(.5), in the shape of the node it multiplies."""
        return self.dropout_mask(self.mask_width["vec"], generator).view(self.B, 1, 1, -1)
