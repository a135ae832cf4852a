"""A loss on the waveform the prediction reconstructs to, with its gradient on the prediction (csrc/waveloss.hip).

The models are trained on the normalised spectrogram, but `Evaluator` grades the impulse response `PostProcess` makes of it
(rir_generation.py:207-223).  `WaveLoss` is the missing link back: per sample, y^ = PostProcess(pred) and

    E_b = sum_t w[t] (y^[t] - y[t])^2,   D_b = T ("mse") or sum_t w[t] y[t]^2 ("energy": the squared misalignment ratio of
    rir_generation.py:221-223),   L = weight / global_batch * sum_b E_b / D_b      (a sample with D_b == 0 counts nothing)

in three launches for the loss and d L / d pred (two for the loss alone), fp64 inside.  `Trainer(..., wave_loss=WaveLoss(...))` adds the
term to the train step; the object also works on its own with any NCHW prediction:

    wl = WaveLoss(weight=0.1, norm="energy")
    dpred = wl(pred, wav_true)                   # fp32 [B, 2, H, W]; wl.wave_out = (sum_b E_b / D_b, sum_b E_b) on the device
    engine.backward(dpred=dpred)
"""
import torch

from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH
from .waveterm import set_geometry


class WaveLoss:
    def __init__(self, weight=1.0, norm="mse", time_weight=None, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH,
                 hop_length=HOP_LENGTH):
        """time_weight: per-sample weights w[t], length hop_length * (des_shape[1] - 1) (None: ones) - e.g. a step over the first 50 ms."""
        if norm not in ops.WAVE_NORMS:
            raise ValueError(f"norm must be one of {sorted(ops.WAVE_NORMS)}")
        set_geometry(self, des_shape, n_fft, win_length, hop_length, weight=weight)
        self.norm = norm
        if time_weight is not None:
            time_weight = (time_weight.detach().to(torch.float32).clone() if isinstance(time_weight, torch.Tensor)
                           else torch.tensor(time_weight, dtype=torch.float32)).contiguous()
            if tuple(time_weight.shape) != (self.T,):
                raise ValueError(f"time_weight must have {self.T} samples")
        self.time_weight = time_weight
        self.wave_out = None            # fp64 [2] on the device: (sum_b E_b / D_b, sum_b E_b) of the last call
        self.wav_pred = None            # fp32 [B, T]: the reconstruction of the last call with want_wav=True
        self._ws = None
        self._dpred = None

    def prepare(self, device, B=None):
        """Everything the calls need that does not depend on the prediction's shape, and with B the workspace as well (a HIP graph
        capture must not allocate)."""
        if self.wave_out is None or self.wave_out.device != torch.device(device):
            self.wave_out = torch.zeros(2, dtype=torch.float64, device=device)
            self._ws = ops.Workspace(device)
            self._dpred = self.wav_pred = None
            if self.time_weight is not None:
                self.time_weight = self.time_weight.to(device)
        if B is not None:
            self._ws.reserve(ops.wave_loss_ws_bytes(B, self.des_shape[1], self.hop_length))

    def __call__(self, pred, wav_true, *, phase_ref=None, spec_target=None, alpha=0.9, inv_norm=None, phase_weight=None,
                 global_batch=None, loss_out=None, dpred=None, want_wav=False, backward=True):
        """pred fp32 [B, 2, H, W], wav_true fp32 [B, T] -> dpred (the given buffer, or one this object keeps), None with
        backward=False (the loss alone: two launches).  phase_ref: the network input of a phase-difference model.  spec_target (+ alpha,
        inv_norm, phase_weight): also add the spectrogram loss's gradient on pred, as an engine's backward(dpred=...) replaces the loss
        kernel's.  loss_out: a float32 device vector whose element 0 grows by weight / global_batch * sum_b E_b / D_b."""
        self.prepare(pred.device)
        if backward and dpred is None:
            if self._dpred is None or self._dpred.shape != pred.shape:
                self._dpred = torch.empty_like(pred)
            dpred = self._dpred
        if want_wav and (self.wav_pred is None or self.wav_pred.shape[0] != pred.shape[0]):
            self.wav_pred = torch.empty((pred.shape[0], self.T), dtype=torch.float32, device=pred.device)
        ops.wave_loss(pred, wav_true, self.wave_out, self._ws, self.des_shape[0], self.des_shape[1], self.n_fft, self.win_length,
                      self.hop_length, norm=self.norm, weight=self.weight, global_batch=global_batch, time_weight=self.time_weight,
                      phase_ref=phase_ref, spec_target=spec_target, alpha=alpha, inv_norm=inv_norm, phase_weight=phase_weight,
                      dpred=dpred if backward else None, wav_pred=self.wav_pred if want_wav else None, loss_out=loss_out)
        return dpred if backward else None
