"""Test infrastructure: the stand-in for ``unet_rir_amd.ops.spectral_loss`` on the simulated runtime, installed over
tests/decay_loss_cpu_ops.py.  It computes from the fp64 closed form of tests/spectral_loss_ref.py, stores what the kernels store (fp32
dwav, written or added to; fp64 spectral_out; loss_out[0] += the term in fp32) and reports its reads and writes to the race check."""
import numpy as np
import torch

import cpu_ops
import decay_loss_cpu_ops
import spectral_loss_ref as SR


def _supported(T, n, w, h):
    return n % 2 == 0 and 16 <= n <= 1024 and 2 <= w <= n and h >= 1 and n // 2 + 1 <= T <= 16384


class SpectralCpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.calls = []          # ("spectral", global_batch, with gradient, accumulate) per call

    def spectral_loss_supported(self, T, n_fft, win_length, hop_length):
        return _supported(T, n_fft, win_length, hop_length)

    def spectral_loss_ws_bytes(self, B, T, resolutions):
        if B <= 0 or not 1 <= len(resolutions) <= 8 or not all(_supported(T, *r) for r in resolutions):
            return 0
        per_row = 3
        for n, w, h in resolutions:
            F, K = 1 + T // h, n // 2 + 1
            per_row += 3 * (-(-F // 16)) * (-(-(n // 2) // 64)) + 4 + 4 * F * K + F * w
        return 8 * B * per_row

    def spectral_loss(self, wav_pred, wav_true, spectral_out, ws, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0,
                      global_batch=None, dwav=None, accumulate=False, loss_out=None):
        ws.reserve(self.spectral_loss_ws_bytes(*wav_pred.shape, resolutions))
        self.rt.touch([wav_pred, wav_true, loss_out] + ([dwav] if accumulate else []), [spectral_out, ws, dwav, loss_out], "spectral_loss")
        gb = wav_pred.shape[0] if global_batch is None else global_batch
        self.calls.append(("spectral", gb, dwav is not None, bool(accumulate)))
        cf = SR.closed_form(wav_pred.detach().numpy(), wav_true.detach().numpy(), resolutions, floor_db, sc_weight, log_weight, weight, gb)
        spectral_out.copy_(torch.from_numpy(cf["spectral_out"]))
        if dwav is not None:
            g = torch.from_numpy(cf["dwav"])
            dwav.copy_(((dwav.double() + g) if accumulate else g).float())
        if loss_out is not None:
            loss_out[0] += float(np.float32(cf["loss"]))


def install(monkeypatch, rt, base=cpu_ops):
    import unet_rir_amd
    impl = decay_loss_cpu_ops.install(monkeypatch, rt, base)
    s = SpectralCpuOps(rt)
    for name in ("spectral_loss_supported", "spectral_loss_ws_bytes", "spectral_loss"):
        if not hasattr(unet_rir_amd.ops, name):
            raise AttributeError(f"unet_rir_amd.ops has no function {name}")
        monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(s, name)))
    impl.spectral = s
    return impl
