"""Test infrastructure: the stand-in for ``unet_rir_amd.ops.spectral_loss_fft`` on the simulated runtime, installed over
tests/spectral_loss_cpu_ops.py.  The schedule is what these tests are about, not the rounding: it computes from the fp64 closed form of
tests/spectral_loss_ref.py like the DFT form's stand-in, stores what the kernels store (fp32 dwav, written or added to; fp64
spectral_out; loss_out[0] += the term in fp32) and reports its reads and writes to the race check under its own name."""
import numpy as np
import torch

import cpu_ops
import spectral_loss_cpu_ops
import spectral_loss_ref as SR


def _supported(T, n, w, h):
    return n in (128, 256, 512, 1024) and 2 <= w <= n and h >= 1 and n // 2 + 1 <= T <= 16384


class SpectralFftCpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.calls = []          # ("spectral_fft", global_batch, with gradient, accumulate) per call

    def spectral_loss_fft_supported(self, T, n_fft, win_length, hop_length):
        return _supported(T, n_fft, win_length, hop_length)

    def spectral_loss_fft_ws_bytes(self, B, T, resolutions):
        if B <= 0 or not 1 <= len(resolutions) <= 8 or not all(_supported(T, *r) for r in resolutions):
            return 0
        doubles, floats = 3, 0
        for n, w, h in resolutions:
            F = 1 + T // h
            doubles += 3 * (-(-F // (2048 // n))) + 4
            floats += F * w
        return 8 * B * doubles + 8 * (-(-(4 * B * floats) // 8))

    def spectral_loss_fft(self, wav_pred, wav_true, spectral_out, ws, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0,
                          global_batch=None, dwav=None, accumulate=False, loss_out=None):
        ws.reserve(self.spectral_loss_fft_ws_bytes(*wav_pred.shape, resolutions))
        self.rt.touch([wav_pred, wav_true, loss_out] + ([dwav] if accumulate else []), [spectral_out, ws, dwav, loss_out], "spectral_loss_fft")
        gb = wav_pred.shape[0] if global_batch is None else global_batch
        self.calls.append(("spectral_fft", gb, dwav is not None, bool(accumulate)))
        cf = SR.closed_form(wav_pred.detach().numpy(), wav_true.detach().numpy(), resolutions, floor_db, sc_weight, log_weight, weight, gb)
        spectral_out.copy_(torch.from_numpy(cf["spectral_out"]))
        if dwav is not None:
            g = torch.from_numpy(cf["dwav"])
            dwav.copy_(((dwav.double() + g) if accumulate else g).float())
        if loss_out is not None:
            loss_out[0] += float(np.float32(cf["loss"]))


def install(monkeypatch, rt, base=cpu_ops):
    import unet_rir_amd
    impl = spectral_loss_cpu_ops.install(monkeypatch, rt, base)
    s = SpectralFftCpuOps(rt)
    for name in ("spectral_loss_fft_supported", "spectral_loss_fft_ws_bytes", "spectral_loss_fft"):
        if not hasattr(unet_rir_amd.ops, name):
            raise AttributeError(f"unet_rir_amd.ops has no function {name}")
        monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(s, name)))
    impl.spectral_fft = s
    return impl
