"""Time the multi-resolution STFT loss (ops.spectral_loss: csrc/spectralloss.hip, fp64 on the matrix cores) against the same definition
written as torch.stft expressions kept on the device under autograd, in fp64 and in fp32 / complex64 (independent implementations,
not the code under test), and the bf16 train step of the default U-Net with a WaveLoss alone against the same step with the spectral
term on top, and with a decay and a spectral term sharing one vector-Jacobian product against the two carried separately
(informational; README.md and DESIGN.md quote the file this writes).

    python scripts/time_spectral_loss.py [--calls 50] [--warmup 10] [--out profiles/spectral_loss.json]

Workload: batch 32, T = 9600 (129 x 151 bins x frames inside 144 x 160 planes, n_fft 256, win 128, hop 64), the default resolutions
(128, 64, 32), (512, 256, 128), (1024, 512, 256), floor 60 dB.  All forms alternate call by call inside one timed loop of one process;
per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time
to enqueue one call, and the device kernels per call torch.profiler sees.  The kernels' results are also compared with the torch
twins' (sanity figures, not a parity test - that is tests/test_spectral_loss_gpu.py)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U
from unet_rir_amd import features as F
from unet_rir_amd.spectralloss import RESOLUTIONS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_wave_loss import count_launches, summary  # noqa: E402

DEV = "cuda:0"
B, H, W = 32, 144, 160
NB, NF = F.STFT_SHAPE
T = F.HOP_LENGTH * (NF - 1)
WEIGHT, FLOOR_DB = 0.1, 60.0


def windows(dtype):
    out = []
    for n, w, h in RESOLUTIONS:
        win = torch.zeros(n, dtype=dtype, device=DEV)
        win[(n - w) // 2:(n - w) // 2 + w] = torch.hann_window(w, periodic=True, dtype=dtype, device=DEV)
        out.append(win)
    return out


def torch_spectral(wav_pred, wav_true, wins):
    """weight / B * sum_b mean_r (SC + LM) in torch expressions, in the dtype of the windows"""
    dt = wins[0].dtype
    p, t = wav_pred.to(dt), wav_true.to(dt)
    delta = 10.0 ** (-FLOOR_DB / 10.0)
    e0 = (t * t).sum(dim=1)
    total = 0.0
    for (n, w, h), win in zip(RESOLUTIONS, wins):
        dp0 = (delta * (win * win).sum() * e0 / T)[:, None, None]
        stft = lambda x: torch.stft(x, n_fft=n, hop_length=h, win_length=n, window=win, center=True, pad_mode="reflect", onesided=True,
                                    return_complex=True)
        sp, st = stft(p), stft(t)
        mp = torch.sqrt(sp.real ** 2 + sp.imag ** 2 + dp0)
        my = torch.sqrt(st.real ** 2 + st.imag ** 2 + dp0)
        sc = ((mp - my) ** 2).sum(dim=(1, 2)) / (my ** 2).sum(dim=(1, 2))
        lm = ((torch.log(mp) - torch.log(my)) ** 2).mean(dim=(1, 2))
        total = total + (sc + lm).sum()
    return WEIGHT / B / len(RESOLUTIONS) * total


class TwoAdjoints:
    """A decay and a spectral term behind `Trainer(spectral_loss=)`, each carried onto dpred by a vector-Jacobian product of its own:
    what the shared adjoint of `Trainer(decay_loss=, spectral_loss=)` is measured against."""

    def __init__(self, dl, sl):
        self.dl, self.sl = dl, sl
        self.des_shape, self.n_fft, self.win_length, self.hop_length = sl.des_shape, sl.n_fft, sl.win_length, sl.hop_length

    def prepare(self, device, B=None):
        self.dl.prepare(device, B)
        self.sl.prepare(device, B)

    def __call__(self, wav_pred, wav_true, dwav=None, **kw):
        self.dl(wav_pred, wav_true, **kw)
        return self.sl(wav_pred, wav_true, **kw)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spectral_loss.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    t = torch.arange(T, dtype=torch.float32)
    wav_true = (torch.randn((B, T), generator=gen) * torch.exp(-t / 700.0)[None, :]).to(DEV)
    pred = F.PreProcess()((torch.randn((B, T), generator=gen) * torch.exp(-t / 900.0)[None, :]).to(DEV))      # a plausible prediction
    wav_pred = F.PostProcess().post_process(pred, nhwc=False).clone()
    ws_bytes = U.ops.spectral_loss_ws_bytes(B, T, RESOLUTIONS)
    ws = U.ops.Workspace(DEV, ws_bytes)
    spectral_out = torch.zeros(3, dtype=torch.float64, device=DEV)
    dwav = torch.empty_like(wav_pred)
    wav_leaf = wav_pred.clone().requires_grad_(True)
    w64, w32 = windows(torch.float64), windows(torch.float32)

    def torch_pair(wins):
        wav_leaf.grad = None
        torch_spectral(wav_leaf, wav_true, wins).backward()

    def torch_forward(wins):
        with torch.no_grad():
            return torch_spectral(wav_pred, wav_true, wins)

    spectral = lambda dw: U.ops.spectral_loss(wav_pred, wav_true, spectral_out, ws, RESOLUTIONS, floor_db=FLOOR_DB, weight=WEIGHT, dwav=dw)
    # the whole train step, bf16 storage, the default U-Net (bench.py's flagship geometry), in this process
    spec_in, emb, spec_out = next(iter(U.synthetic_batches(1, B, H, W, DEV)))
    sl = lambda: U.SpectralLoss(weight=WEIGHT, floor_db=FLOOR_DB)
    dl = lambda: U.DecayLoss(weight=0.01, floor_db=FLOOR_DB)
    steps = {}
    for name, kw in (("step_bf16_wave", {}), ("step_bf16_wave_spectral", dict(spectral_loss=sl())),
                     ("step_bf16_wave_decay", dict(decay_loss=dl())),
                     ("step_bf16_wave_decay_spectral_shared", dict(decay_loss=dl(), spectral_loss=sl())),
                     ("step_bf16_wave_decay_spectral_two_adjoints", dict(spectral_loss=TwoAdjoints(dl(), sl())))):
        eng = U.UNetEngine(H, W, B, device=DEV, dtype="bf16")
        tr = U.Trainer(eng, wave_loss=U.WaveLoss(weight=0.5, norm="energy"), **kw)
        steps[name] = (lambda tr=tr: tr.step(spec_in, emb, spec_out, wav_true=wav_true))
    spectral(dwav)
    forms = {"spectral_pair": lambda: spectral(dwav), "spectral_forward": lambda: spectral(None),
             "torch_f64_pair": lambda: torch_pair(w64), "torch_f64_forward": lambda: torch_forward(w64),
             "torch_c64_pair": lambda: torch_pair(w32), "torch_c64_forward": lambda: torch_forward(w32), **steps}
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    dev_ms, host_us = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.calls):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            host_us[name].append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            dev_ms[name].append(e0.elapsed_time(e1))
    spectral(dwav)
    torch_pair(w64)
    g64 = wav_leaf.grad.clone()
    torch_pair(w32)
    g32 = wav_leaf.grad.clone()
    torch.cuda.synchronize()
    # useful arithmetic: 2 flop per multiply-add; the analysis forms Re and Im of two waveforms, the adjoint one real synthesis from two planes
    macs = sum((1 + T // h) * (n // 2 + 1) * w for n, w, h in RESOLUTIONS)
    flop_analysis, flop_adjoint = B * macs * 2 * 2 * 2, B * macs * 2 * 2
    res = {"workload": {"batch": B, "samples": T, "resolutions": [list(r) for r in RESOLUTIONS], "floor_db": FLOOR_DB, "weight": WEIGHT},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "workspace_bytes": ws_bytes,
           "dwav_max_abs_difference_over_peak_f64": float((dwav - g64).abs().max() / g64.abs().max()),
           "torch_c64_dwav_max_abs_difference_over_peak_f64": float((g32 - g64).abs().max() / g64.abs().max()),
           "loss_kernels": float(WEIGHT / B * (spectral_out[0] + spectral_out[1])), "loss_torch_f64": float(torch_forward(w64)),
           "loss_torch_c64": float(torch_forward(w32)), "gflop_analysis": flop_analysis / 1e9, "gflop_adjoint": flop_adjoint / 1e9}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        print(name, json.dumps(res[name]))
    res["spectral_pair"]["launches_per_call_by_construction"] = 4
    res["spectral_forward"]["launches_per_call_by_construction"] = 2
    m = lambda k: res[k]["device_ms_median"]
    res["spectral_pair"]["useful_tflop_per_s"] = (flop_analysis + flop_adjoint) / (m("spectral_pair") * 1e-3) / 1e12
    res["spectral_forward"]["useful_tflop_per_s"] = flop_analysis / (m("spectral_forward") * 1e-3) / 1e12
    res["torch_f64_pair_over_spectral_pair"] = m("torch_f64_pair") / m("spectral_pair")
    res["torch_c64_pair_over_spectral_pair"] = m("torch_c64_pair") / m("spectral_pair")
    res["torch_f64_forward_over_spectral_forward"] = m("torch_f64_forward") / m("spectral_forward")
    res["torch_c64_forward_over_spectral_forward"] = m("torch_c64_forward") / m("spectral_forward")
    res["step_added_ms"] = m("step_bf16_wave_spectral") - m("step_bf16_wave")
    res["step_added_share_of_the_step"] = res["step_added_ms"] / m("step_bf16_wave")
    res["shared_adjoint_saves_ms"] = m("step_bf16_wave_decay_spectral_two_adjoints") - m("step_bf16_wave_decay_spectral_shared")
    res["step_spread_ms_p10_p90"] = {k: [res[k]["device_ms_p10"], res[k]["device_ms_p90"]] for k in steps}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
