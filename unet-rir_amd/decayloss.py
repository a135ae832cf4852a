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
from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH
from .waveterm import WaveTerm


class DecayLoss(WaveTerm):
    out_len = 2
    decay_out = property(lambda self: self.out, doc="fp64 [2] on the device: (sum_b Q_b, samples counted) of the last call")

    def __init__(self, weight=1.0, floor_db=60.0, des_shape=STFT_SHAPE, n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH):
        """floor_db: the curves are floored at -floor_db relative to the target's energy: the fit ends where the window has nothing left
        to say."""
        super().__init__(floor_db, des_shape, n_fft, win_length, hop_length, weight=weight)

    def ws_bytes(self, B):
        return ops.decay_loss_ws_bytes(B, self.T)

    def _launch(self, wav_pred, wav_true, dwav, add, global_batch, loss_out):
        if add:
            raise ValueError("DecayLoss: the kernel writes its cotangent and cannot add to one; a dwav= the caller gives is not taken")
        ops.decay_loss(wav_pred, wav_true, self.out, self._ws, floor_db=self.floor_db, weight=self.weight, global_batch=global_batch,
                       dwav=dwav, loss_out=loss_out)
