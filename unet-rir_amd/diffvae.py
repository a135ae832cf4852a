"""DiffVAE (dl_models/diff_vae.py) on the HIP kernels: the VAE that predicts a phase DIFFERENCE (rir_generation.py:51-63; the target
of main_training.py:214-217).  It is vae.VAEEngine - conv / conv-transpose stack, `mu` / `log_variance` heads, sampling layer, KL term,
Dropout(.3) behind decoder_dense, LeakyReLU decoder, no regulariser - with the information vector of the VQ-VAE, Embedding(1500, 128)
-> Dense(n_neurons) per position (:416-417), and a LINEAR output (:385): a difference of two phases in [0, 1] lies in [-1, 1].
PARITY UNPINNED like the rest of the family: the pin is tests/diffvae_ref.py, a restatement of the source text.
"""
from .vae import VAEEngine

DIFF_VOCAB, DIFF_EMB_DIM = 1500, 128          # Embedding(1500, 128) (dl_models/diff_vae.py:416)


class DiffVAEEngine(VAEEngine):
    """One replica of DiffVAE for a fixed per-replica batch size (constructor mirrors dl_models/diff_vae.py:48-57; DEFAULTS is the
    model of its __main__ block, :476-485).  Everything VAEEngine says about eps, the KL term and loss_out holds here."""
    output_act = "linear"         # Activation("linear") (dl_models/diff_vae.py:385)
    DEFAULTS = ((32, 64, 128, 256), 16, 1280)

    def _join_vector(self, x, name, dropout=None):
        """The Dense layer sits on the unflattened embedding (:416-417); Flatten at the join (:463-465)."""
        return self._join_vector_per_position(x, name, DIFF_VOCAB, DIFF_EMB_DIM)
