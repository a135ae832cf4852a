"""A loss on the energy decay curve of the waveform (csrc/decayloss.hip), with its gradient on the waveform or - through the
vector-Jacobian product of `PostProcess` (csrc/istft_bwd.hip) - on the prediction.

`Evaluator(acoustics=True)` grades DRR, C50, centre time and EDT, all read off Schroeder's backward integral; `WaveLoss` trains on a
squared error the first few hundred samples dominate.  `DecayLoss` is the term that says "decay at the room's rate": per sample, with
S_x[t] = sum_{s >= t} x[s]^2, E0 = S_y[0] and delta = 10^(-floor_db / 10),

    c_x[t] = 10 log10(S_x[t] / E0 + delta),   Q_b = mean_t (c_y^[t] - c_y[t])^2   (dB^2; a sample with a silent target counts nothing),
    L = weight / global_batch * sum_b Q_b

in two launches, fp64 inside; one more launch carries the gradient from the waveform to the prediction.  `Trainer(...,
decay_loss=DecayLoss(...))` adds the term to the train step; the object also works on its own:

    dl = DecayLoss(weight=0.01)
    dwav = dl(wav_pred, wav_true)                                  # fp32 [B, T]; dl.decay_out = (sum_b Q_b, samples counted) on the device
    dpred = dl(wav_pred, wav_true, pred=pred)                      # fp32 [B, 2, H, W], wav_pred = PostProcess(pred)
    engine.backward(dpred=dpred)
"""
import math

import torch

from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH


class DecayLoss:
    def __init__(self, weight=1.0, floor_db=60.0, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH):
        """floor_db: the curves are floored at -floor_db relative to the target's energy: the fit ends where the window has nothing left
        to say."""
        if not (weight >= 0.0) or not math.isfinite(weight):
            raise ValueError("weight must be a finite number >= 0")
        if not math.isfinite(floor_db) or not (0.0 < floor_db <= 200.0):
            raise ValueError("floor_db must be in (0, 200]")
        self.weight, self.floor_db = float(weight), float(floor_db)
        self.des_shape = (int(des_shape[0]), int(des_shape[1]))
        self.n_fft, self.win_length, self.hop_length = int(n_fft), int(win_length), int(hop_length)
        self.T = self.hop_length * (self.des_shape[1] - 1)
        self.decay_out = None           # fp64 [2] on the device: (sum_b Q_b, samples counted) of the last call
        self._ws = None
        self._dwav = None
        self._dpred = None

    def prepare(self, device, B=None):
        """Everything the calls need that does not depend on the batch, and with B the workspace and the cotangent as well (a HIP graph
        capture must not allocate)."""
        if self.decay_out is None or self.decay_out.device != torch.device(device):
            self.decay_out = torch.zeros(2, dtype=torch.float64, device=device)
            self._ws = ops.Workspace(device)
            self._dwav = self._dpred = None
        if B is not None:
            self._ws.reserve(ops.decay_loss_ws_bytes(B, self.T))
            if self._dwav is None or self._dwav.shape[0] != B:
                self._dwav = torch.empty((B, self.T), dtype=torch.float32, device=device)

    def __call__(self, wav_pred, wav_true, *, pred=None, phase_ref=None, dpred=None, accumulate=False, global_batch=None, loss_out=None,
                 backward=True):
        """wav_pred, wav_true fp32 [B, T] -> dwav (a buffer this object keeps), or with pred fp32 [B, 2, H, W] (wav_pred =
        PostProcess(pred); phase_ref: the network input of a phase-difference model) dpred: the given buffer or one this object keeps,
        written, or with accumulate added to.  None with backward=False (the loss alone: no gradient, no vector-Jacobian product).
        loss_out: a float32 device vector whose element 0 grows by weight / global_batch * sum_b Q_b."""
        self.prepare(wav_pred.device)
        dwav = None
        if backward:
            if self._dwav is None or self._dwav.shape != wav_pred.shape:
                self._dwav = torch.empty_like(wav_pred)
            dwav = self._dwav
        ops.decay_loss(wav_pred, wav_true, self.decay_out, self._ws, floor_db=self.floor_db, weight=self.weight, global_batch=global_batch,
                       dwav=dwav, loss_out=loss_out)
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
