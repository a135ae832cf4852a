"""Test infrastructure: the stand-in for ``unet_rir_amd.ops.wave_loss`` on the simulated runtime, installed over tests/cpu_ops.py (or a
family's own stand-ins).  It computes from the fp64 closed form of tests/wave_loss_ref.py, stores what the kernels store (fp32 dpred and
waveform, fp64 wave_out, loss_out[0] += the term in fp32) and reports its reads and writes to the race check."""
import numpy as np
import torch

import cpu_ops
import wave_loss_ref as WR


class WaveCpuOps:
    WAVE_NORMS = {"mse": 0, "energy": 1}

    def __init__(self, rt):
        self.rt = rt
        self.calls = []          # (global_batch, with gradient, fused) per call

    def wave_loss_ws_bytes(self, B, n_frames, hop_length):
        T = hop_length * (n_frames - 1)
        return 8 * (B * T + 2 * B * -(-T // 64) + B)

    def wave_loss(self, pred, wav_true, wave_out, ws, n_bins, n_frames, n_fft=256, win_length=128, hop_length=64, norm="mse", weight=1.0,
                  global_batch=None, time_weight=None, phase_ref=None, spec_target=None, alpha=0.9, inv_norm=None, phase_weight=None,
                  dpred=None, wav_pred=None, loss_out=None):
        fused = spec_target is not None and dpred is not None
        ws.reserve(self.wave_loss_ws_bytes(pred.shape[0], n_frames, hop_length))
        self.rt.touch([pred, wav_true, time_weight, phase_ref] + ([spec_target, phase_weight] if fused else []) + [loss_out],
                      [wave_out, ws, dpred, wav_pred, loss_out], "wave_loss")
        gb = pred.shape[0] if global_batch is None else global_batch
        self.calls.append((gb, dpred is not None, fused))
        n = lambda t: None if t is None else t.detach().numpy()
        kw = dict(spec_target=n(spec_target), alpha=alpha, inv_norm=inv_norm, phase_weight=n(phase_weight)) if fused else {}
        cf = WR.closed_form(n(pred), n(wav_true), (n_bins, n_frames), n_fft, win_length, hop_length, norm=norm, weight=weight, global_batch=gb,
                            time_weight=n(time_weight), phase_ref=n(phase_ref), **kw)
        wave_out.copy_(torch.from_numpy(cf["wave_out"]))
        if dpred is not None:
            dpred.copy_(torch.from_numpy(cf["grad"]).float())
        if wav_pred is not None:
            wav_pred.copy_(torch.from_numpy(cf["wav"]).float())
        if loss_out is not None:
            loss_out[0] += float(np.float32(cf["loss"]))


def install(monkeypatch, rt, base=cpu_ops):
    import unet_rir_amd
    impl = base.install(monkeypatch, rt)
    w = WaveCpuOps(rt)
    for name in ("wave_loss_ws_bytes", "wave_loss"):
        if not hasattr(unet_rir_amd.ops, name):
            raise AttributeError(f"unet_rir_amd.ops has no function {name}")
        monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(w, name)))
    impl.wave = w
    return impl
