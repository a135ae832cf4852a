"""ResAE (dl_models/res_ae.py) on the same HIP kernels: the second operator graph of BASELINE.json configs[4].

Residual bottleneck blocks (1x1 -> kxk -> 1x1 Conv2D / Conv2DTranspose, BatchNormalization, LeakyReLU(0.3), Add), a Dense
latent that concatenates the information vector, and a mirrored Conv2DTranspose decoder, built on ae.AEFamilyEngine.
"""
from .ae import AEFamilyEngine
from .graph import Node, LEAKY


class ResAEEngine(AEFamilyEngine):
    """ResAE (dl_models/res_ae.py:210-530): Dropout behind the latent Dense and behind decoder_dense."""
    MASKS = ("latent", "dec")
    DEFAULTS = ((32, 64, 128, 256), 32, 1024)

    def _res_block(self, x: Node, name, f, k, stride, transpose, with_skip, pad_in=0):
        """res_conv / res_identity and the Conv2DTranspose twins (dl_models/res_ae.py:310-371, :453-514)."""
        tag = "conv" if with_skip else "id"
        c1 = self._conv(x, f"{name}_{tag}.1", f, 1, stride if with_skip else 1, transpose, pad_in=pad_in)
        a1 = self._bn_act(c1, f"{name}_{tag}.1", LEAKY)
        c2 = self._conv(a1, f"{name}_{tag}.2", f, k, 1, transpose)
        a2 = self._bn_act(c2, f"{name}_{tag}.2", LEAKY)
        c3 = self._conv(a2, f"{name}_{tag}.3", f, 1, 1, transpose)
        if with_skip:
            cs = self._conv(x, f"{name}_conv.s", f, 1, stride, transpose, pad_in=pad_in)
            skip = self._bn_act(cs, f"{name}_conv.s", 0)
        else:
            skip = x
        return self._bn_act(c3, f"{name}_{tag}.3", LEAKY, addend=skip)

    def _build(self):
        n = len(self.filters)
        x = self._input()
        for i in range(n):        # encoder: _add_conv_layers (:424-451)
            x = self._res_block(x, f"e_res_{i + 1}", self.filters[i], self.kernels[i], self.strides[i], False, True, pad_in=self.PAD if i == 0 else 0)
            x = self._res_block(x, f"e_res_{i + 1}", self.filters[i], self.kernels[i], 1, False, False)
        z = self._dense(self._join_vector(x, "e_dense_vector"), "e_out", self.latent)       # -> Dense(latent) -> Dropout (:516-530)
        x = self._decoder_entry(self._dropout(z, "latent"))
        x = self._res_block(x, "d_res_0", self.filters[-1], self.kernels[-1], 1, True, True)
        x = self._res_block(x, "d_res_0", self.filters[-1], self.kernels[-1], 1, True, False)
        for layer_index in reversed(range(1, n)):                # _add_conv_transpose_layers (:272-308)
            name = f"d_res_{n - layer_index}"
            f, k = self.filters[layer_index - 1], self.kernels[layer_index]      # the kernel index is the reference's own (:303-307)
            x = self._res_block(x, name, f, k, self.strides[layer_index - 1], True, True)
            x = self._res_block(x, name, f, k, 1, True, False)
        self._output_layer(x, "d_out")
