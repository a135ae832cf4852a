"""What the loss terms on the reconstructed waveform share: the geometry of the prediction they look at, and - for the terms that take
the waveform itself (`DecayLoss`, `SpectralLoss`) - the buffers, the call and the vector-Jacobian product of `PostProcess`
(csrc/istft_bwd.hip) that carries their gradient from the waveform to the prediction.

A term is `WaveTerm` plus its constructor arguments, its result vector under a public name, and one launch:

    class MyLoss(WaveTerm):
        out_len = 2                                                # fp64 entries of the result vector `self.out`
        my_out = property(lambda self: self.out)
        def ws_bytes(self, B): ...                                 # workspace of a batch of B
        def _launch(self, wav_pred, wav_true, dwav, add, global_batch, loss_out): ...
"""
import math

import torch

from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH

_NO_FLOOR = object()


def set_geometry(term, des_shape, n_fft, win_length, hop_length, *, floor_db=_NO_FLOOR, **weights):
    """The checked settings every term keeps: the weights (finite, >= 0) under their names, `floor_db` in (0, 200] where the term has
    one, and the geometry of the model's prediction (what `PostProcess` inverts), which fixes the waveform's length T."""
    for name, v in weights.items():
        if not (v >= 0.0) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number >= 0")
        setattr(term, name, float(v))
    if floor_db is not _NO_FLOOR:
        if not math.isfinite(floor_db) or not (0.0 < floor_db <= 200.0):
            raise ValueError("floor_db must be in (0, 200]")
        term.floor_db = float(floor_db)
    term.des_shape = (int(des_shape[0]), int(des_shape[1]))
    term.n_fft, term.win_length, term.hop_length = int(n_fft), int(win_length), int(hop_length)
    term.T = term.hop_length * (term.des_shape[1] - 1)


class WaveTerm:
    """A loss on (wav_pred, wav_true), fp32 [B, T], with its gradient on the waveform or on the prediction."""
    out_len = 0

    def __init__(self, floor_db, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH, **weights):
        set_geometry(self, des_shape, n_fft, win_length, hop_length, floor_db=floor_db, **weights)
        self.out = None                 # fp64 [out_len] on the device: the sums of the last call
        self._ws = None
        self._dwav = None
        self._dpred = None

    def ws_bytes(self, B):
        raise NotImplementedError

    def _launch(self, wav_pred, wav_true, dwav, add, global_batch, loss_out):
        """The term's kernels.  dwav: where the cotangent on the waveform goes (None: the loss alone); add: the caller gave that buffer
        and the cotangent is added to what it holds."""
        raise NotImplementedError

    def prepare(self, device, B=None):
        """Everything the calls need that does not depend on the batch, and with B the workspace and the cotangent as well (a HIP graph
        capture must not allocate)."""
        if self.out is None or self.out.device != torch.device(device):
            self.out = torch.zeros(self.out_len, dtype=torch.float64, device=device)
            self._ws = ops.Workspace(device)
            self._dwav = self._dpred = None
        if B is not None:
            self._ws.reserve(self.ws_bytes(B))
            if self._dwav is None or self._dwav.shape[0] != B:
                self._dwav = torch.empty((B, self.T), dtype=torch.float32, device=device)

    def __call__(self, wav_pred, wav_true, *, pred=None, phase_ref=None, dpred=None, accumulate=False, dwav=None, global_batch=None,
                 loss_out=None, backward=True):
        """wav_pred, wav_true fp32 [B, T] -> dwav (a buffer this object keeps; with dwav= given, the term's cotangent is ADDED to that
        buffer and it is returned), or with pred fp32 [B, 2, H, W] (wav_pred = PostProcess(pred); phase_ref: the network input of a
        phase-difference model) dpred: the given buffer or one this object keeps, written, or with accumulate added to.  None with
        backward=False (the loss alone: no gradient, no vector-Jacobian product).  loss_out: a float32 device vector whose element 0
        grows by weight / global_batch * sum_b Q_b."""
        self.prepare(wav_pred.device)
        add = dwav is not None
        if backward and not add:
            if self._dwav is None or self._dwav.shape != wav_pred.shape:
                self._dwav = torch.empty_like(wav_pred)
            dwav = self._dwav
        self._launch(wav_pred, wav_true, dwav if backward else None, add, global_batch, loss_out)
        if not backward:
            return None
        if pred is None:
            return dwav
        if dpred is None:
            if accumulate:
                raise ValueError("accumulate=True adds to a dpred the caller gives")
            if self._dpred is None or self._dpred.shape != pred.shape:
                self._dpred = torch.empty_like(pred)
            dpred = self._dpred
        ops.istft_features_bwd(pred, dwav, dpred, self.des_shape[0], self.des_shape[1], self.n_fft, self.win_length, self.hop_length,
                               phase_ref=phase_ref, accumulate=accumulate)
        return dpred
