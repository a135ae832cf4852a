"""Time the waveform-domain loss (ops.wave_loss: csrc/waveloss.hip, fp64) against the same loss and gradient written as torch
expressions kept on the device (torch.istft under autograd, fp32 / complex64: an independent implementation, not the code under
test), and the bf16 train step of the default U-Net with and without a WaveLoss (informational; README.md and DESIGN.md quote the
file this writes).

    python scripts/time_wave_loss.py [--calls 50] [--warmup 10] [--out profiles/wave_loss.json]

Workload: batch 32, 129 x 151 bins x frames inside 144 x 160 planes (dataset.py:62-70), n_fft 256, win 128, hop 64, T = 9600,
norm "energy", no time weight.  All forms alternate call by call inside one timed loop; per form: the median, minimum, maximum and the
10th / 90th percentile of the device time between two HIP events, the median host time to enqueue one call, and the device kernels
per call torch.profiler sees.  The kernels' gradient is also compared with the torch twin's (complex64: a sanity figure, not a parity
test - that is tests/test_wave_loss_gpu.py)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U
from unet_rir_amd import features as F

DEV = "cuda:0"
B, H, W = 32, 144, 160
NB, NF = F.STFT_SHAPE
N_FFT, WIN, HOP = F.N_FFT, F.WIN_LENGTH, F.HOP_LENGTH
T = HOP * (NF - 1)
WEIGHT = 0.5


def torch_loss(pred, wav_true, window):
    """weight / B * sum_b E_b / D_b ("energy") of the reconstruction, in torch expressions"""
    amp = (10.0 ** ((pred[:, 0, :NB, :NF] * 100.0 - 100.0) / 20.0) - 1e-5) * 128.0
    ph = torch.remainder(pred[:, 1, :NB, :NF] * (2.0 * math.pi), 2.0 * math.pi) - math.pi
    y = torch.istft(torch.polar(amp, ph), N_FFT, HOP, WIN, window, center=True)
    return WEIGHT / B * (((y - wav_true) ** 2).sum(dim=1) / (wav_true ** 2).sum(dim=1)).sum()


def count_launches(fn, n):
    """Device kernels per call seen by torch.profiler over n calls (None when the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        return round(len(kernels) / n, 2) if kernels else None
    except Exception as exc:                                    # the measurement is optional; say why it is missing
        print("launch count not available:", exc, file=sys.stderr)
        return None


def summary(dev_ms, host_us):
    q = statistics.quantiles(dev_ms, n=10)
    return {"device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "device_ms_max": max(dev_ms),
            "device_ms_p10": q[0], "device_ms_p90": q[-1], "host_enqueue_us_median": statistics.median(host_us)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "wave_loss.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    t = torch.arange(T, dtype=torch.float32)
    wav_true = (torch.randn((B, T), generator=gen) * torch.exp(-t / 700.0)[None, :]).to(DEV)
    pred = F.PreProcess()((torch.randn((B, T), generator=gen) * torch.exp(-t / 900.0)[None, :]).to(DEV))      # a plausible prediction
    window = torch.hann_window(WIN, periodic=True, device=DEV)
    ws = U.ops.Workspace(DEV, U.ops.wave_loss_ws_bytes(B, NF, HOP))
    wave_out = torch.zeros(2, dtype=torch.float64, device=DEV)
    dpred = torch.empty_like(pred)
    leaf = pred.clone().requires_grad_(True)

    def torch_pair():
        leaf.grad = None
        torch_loss(leaf, wav_true, window).backward()

    def torch_forward():
        with torch.no_grad():
            return torch_loss(pred, wav_true, window)

    kernels = lambda dp: U.ops.wave_loss(pred, wav_true, wave_out, ws, NB, NF, N_FFT, WIN, HOP, norm="energy", weight=WEIGHT, dpred=dp)
    # the whole train step, bf16 storage, the default U-Net (bench.py's flagship geometry), with and without the term
    spec_in, emb, spec_out = next(iter(U.synthetic_batches(1, B, H, W, DEV)))
    steps = {}
    for name, wl in (("step_bf16_plain", None), ("step_bf16_wave", U.WaveLoss(weight=WEIGHT, norm="energy"))):
        eng = U.UNetEngine(H, W, B, device=DEV, dtype="bf16")
        tr = U.Trainer(eng, wave_loss=wl)
        steps[name] = (lambda tr=tr, wl=wl: tr.step(spec_in, emb, spec_out, wav_true=wav_true if wl is not None else None))
    forms = {"kernels_pair": lambda: kernels(dpred), "kernels_forward": lambda: kernels(None), "torch_pair": torch_pair,
             "torch_forward": torch_forward, **steps}
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
    kernels(dpred)
    torch_pair()
    torch.cuda.synchronize()
    res = {"workload": {"batch": B, "planes": [H, W], "n_bins": NB, "n_frames": NF, "n_fft": N_FFT, "win_length": WIN, "hop_length": HOP,
                        "samples": T, "norm": "energy", "weight": WEIGHT},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "workspace_bytes": U.ops.wave_loss_ws_bytes(B, NF, HOP),
           "gradient_max_abs_difference_over_peak": float((dpred - leaf.grad).abs().max() / leaf.grad.abs().max()),
           "loss_kernels": float(WEIGHT / B * wave_out[0]), "loss_torch": float(torch_forward())}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        print(name, json.dumps(res[name]))
    res["kernels_pair"]["launches_per_call_by_construction"] = 3
    res["kernels_forward"]["launches_per_call_by_construction"] = 2
    m = lambda k: res[k]["device_ms_median"]
    res["torch_pair_over_kernels_pair"] = m("torch_pair") / m("kernels_pair")
    res["torch_forward_over_kernels_forward"] = m("torch_forward") / m("kernels_forward")
    res["step_added_ms"] = m("step_bf16_wave") - m("step_bf16_plain")
    res["step_spread_ms_p10_p90"] = {k: [res[k]["device_ms_p10"], res[k]["device_ms_p90"]] for k in ("step_bf16_plain", "step_bf16_wave")}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
