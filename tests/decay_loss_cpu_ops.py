"""Test infrastructure: the stand-ins for ``unet_rir_amd.ops.decay_loss`` and ``ops.istft_features_bwd`` on the simulated runtime,
installed over tests/wave_loss_cpu_ops.py.  They compute from the fp64 closed forms of tests/decay_loss_ref.py, store what the kernels
store (fp32 dwav and dpred, fp64 decay_out, loss_out[0] += the term in fp32) and report their reads and writes to the race check."""
import numpy as np
import torch

import cpu_ops
import decay_loss_ref as DR
import wave_loss_cpu_ops


class DecayCpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.calls = []          # ("decay", global_batch, with gradient) and ("vjp", accumulate, with phase_ref) per call

    def decay_loss_supported(self, T):
        return 1 <= T <= 16384

    def decay_loss_ws_bytes(self, B, T):
        return 16 * B if B > 0 and self.decay_loss_supported(T) else 0

    def decay_loss(self, wav_pred, wav_true, decay_out, ws, floor_db=60.0, weight=1.0, global_batch=None, dwav=None, loss_out=None):
        ws.reserve(self.decay_loss_ws_bytes(*wav_pred.shape))
        self.rt.touch([wav_pred, wav_true, loss_out], [decay_out, ws, dwav, loss_out], "decay_loss")
        gb = wav_pred.shape[0] if global_batch is None else global_batch
        self.calls.append(("decay", gb, dwav is not None))
        cf = DR.closed_form(wav_pred.detach().numpy(), wav_true.detach().numpy(), floor_db, weight, gb)
        decay_out.copy_(torch.from_numpy(cf["decay_out"]))
        if dwav is not None:
            dwav.copy_(torch.from_numpy(cf["dwav"]).float())
        if loss_out is not None:
            loss_out[0] += float(np.float32(cf["loss"]))

    def istft_features_bwd(self, pred, dwav, dpred, n_bins, n_frames, n_fft=256, win_length=128, hop_length=64, phase_ref=None,
                           accumulate=False):
        self.rt.touch([pred, dwav, phase_ref] + ([dpred] if accumulate else []), [dpred], "istft_features_bwd")
        self.calls.append(("vjp", bool(accumulate), phase_ref is not None))
        n = lambda t: None if t is None else t.detach().numpy()
        g = torch.from_numpy(DR.vjp_closed_form(n(pred), n(dwav), (n_bins, n_frames), n_fft, win_length, hop_length, phase_ref=n(phase_ref))["grad"])
        if accumulate:
            nb, nf = n_bins, n_frames
            dpred[:, :, :nb, :nf] = (dpred[:, :, :nb, :nf].double() + g[:, :, :nb, :nf]).float()
        else:
            dpred.copy_(g.float())


def install(monkeypatch, rt, base=cpu_ops):
    import unet_rir_amd
    impl = wave_loss_cpu_ops.install(monkeypatch, rt, base)
    d = DecayCpuOps(rt)
    for name in ("decay_loss_supported", "decay_loss_ws_bytes", "decay_loss", "istft_features_bwd"):
        if not hasattr(unet_rir_amd.ops, name):
            raise AttributeError(f"unet_rir_amd.ops has no function {name}")
        monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(d, name)))
    impl.decay = d
    return impl
