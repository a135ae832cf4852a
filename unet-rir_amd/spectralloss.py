"""The multi-resolution STFT loss on the waveform (csrc/spectralloss.hip), with its gradient on the waveform or - through the
vector-Jacobian product of `PostProcess` (csrc/istft_bwd.hip) - on the prediction.

The networks predict amplitude and phase as two independent planes at one resolution (n_fft 256, window 128, hop 64).  A pair that is
the STFT of no signal costs nothing under the spectrogram loss and little under `WaveLoss`; looked at with a different window it shows at
once.  `SpectralLoss` is the spectral-convergence plus log-magnitude pair of Parallel WaveGAN / DDSP / auraloss on the RECONSTRUCTED
waveform at resolutions other than the model's own, in the squared (smooth) forms: per sample and resolution, with E0 the target's
energy, P0 = (sum w^2) E0 / T, delta = 10^(-floor_db / 10) and M_x = sqrt(|X|^2 + delta P0),

    SC = sum (M_y^ - M_y)^2 / sum M_y^2,   LM = mean (ln M_y^ - ln M_y)^2,   Q_b = mean_r (sc_weight SC + log_weight LM)
    L = weight / global_batch * sum_b Q_b              (a sample with a silent target counts nothing)

in four launches with the gradient, two without, fp64 on the matrix cores; one more launch carries the gradient from the waveform to the
prediction.  `method="fft"` runs the same definition on fp32 FFTs held in LDS (csrc/spectralloss_fft.hip; n_fft 128, 256, 512 or 1024):
several times cheaper and with a workspace without spectra, at an fp32 transform's error instead of the fp64 form's derived bound - for a
term that is paid every step; `"dft"` is the form for the end of training, where y^ approaches y and M_y^ - M_y cancels.
`Trainer(..., spectral_loss=SpectralLoss(...))` adds the term to the train step; the object also works on its own:

    sl = SpectralLoss(weight=0.1)
    dwav = sl(wav_pred, wav_true)                                  # fp32 [B, T]; sl.spectral_out = (sum SC, sum LM, samples counted)
    dpred = sl(wav_pred, wav_true, pred=pred)                      # fp32 [B, 2, H, W], wav_pred = PostProcess(pred)
    engine.backward(dpred=dpred)
"""
from . import ops
from .features import HOP_LENGTH, N_FFT, STFT_SHAPE, WIN_LENGTH
from .waveterm import WaveTerm

# one resolution finer in time than the model's own (256, 128, 64), one finer in frequency and one much finer
RESOLUTIONS = ((128, 64, 32), (512, 256, 128), (1024, 512, 256))


class SpectralLoss(WaveTerm):
    out_len = 3
    spectral_out = property(lambda self: self.out,
                            doc="fp64 [3] on the device: (sum_b mean_r SC, sum_b mean_r LM, samples counted) of the last call")

    def __init__(self, weight=1.0, resolutions=RESOLUTIONS, sc_weight=1.0, log_weight=1.0, floor_db=60.0, des_shape=STFT_SHAPE,
                 n_fft=N_FFT, win_length=WIN_LENGTH, hop_length=HOP_LENGTH, *, method="dft"):
        """resolutions: 1 to 8 triples (n_fft, win_length, hop_length) of the loss's own transforms.  floor_db: the magnitudes are
        smoothed at -floor_db relative to the power a bin would carry with the target's energy spread evenly.  des_shape, n_fft,
        win_length, hop_length: the geometry of the model's prediction (what `PostProcess` inverts), which fixes T.  method: "dft"
        (fp64 DFTs on the matrix cores) or "fft" (fp32 FFTs in LDS)."""
        if method not in ("dft", "fft"):
            raise ValueError(f'method must be "dft" or "fft", not {method!r}')
        self.method = method
        super().__init__(floor_db, des_shape, n_fft, win_length, hop_length, weight=weight, sc_weight=sc_weight, log_weight=log_weight)
        self.resolutions = tuple(tuple(int(v) for v in r) for r in resolutions)
        if not 1 <= len(self.resolutions) <= 8 or any(len(r) != 3 for r in self.resolutions):
            raise ValueError("resolutions: 1 to 8 triples (n_fft, win_length, hop_length)")
        for n, w, h in self.resolutions:
            if not (n % 2 == 0 and 16 <= n <= 1024 and 2 <= w <= n and h >= 1):
                raise ValueError(f"resolution {(n, w, h)}: n_fft even in 16 ... 1024, 2 <= win_length <= n_fft, hop_length >= 1")
        if method == "fft":
            for r in self.resolutions:
                if not ops.spectral_loss_fft_supported(self.T, *r):
                    raise ValueError(f'resolution {r} at {self.T} samples: method="fft" takes n_fft 128, 256, 512 or 1024 with '
                                     f'n_fft / 2 + 1 <= T <= 16384; use method="dft"')
        self._op = "spectral_loss_fft" if method == "fft" else "spectral_loss"       # looked up in ops at every call

    def ws_bytes(self, B):
        need = getattr(ops, self._op + "_ws_bytes")(B, self.T, self.resolutions)
        if not need:
            raise ValueError(f"SpectralLoss: the kernels do not take waveforms of {self.T} samples at {self.resolutions}")
        return need

    def _launch(self, wav_pred, wav_true, dwav, add, global_batch, loss_out):
        getattr(ops, self._op)(wav_pred, wav_true, self.out, self._ws, self.resolutions, floor_db=self.floor_db, sc_weight=self.sc_weight,
                               log_weight=self.log_weight, weight=self.weight, global_batch=global_batch, dwav=dwav,
                               accumulate=add and dwav is not None, loss_out=loss_out)
