"""Time the Griffin-Lim reconstruction of a batch (ops.griffinlim: csrc/griffinlim.hip, fp64) against the same loop written as
torch.stft / torch.istft expressions on the device in complex64 - librosa's own precision, and an independent implementation, not
the code under test (informational; README.md and DESIGN.md quote the file this writes).

    python scripts/time_griffinlim.py [--calls 50] [--warmup 10] [--out profiles/griffinlim.json]

Workload: batch 32, 129 x 151 bins x frames inside 144 x 160 planes (dataset.py:62-70), n_fft 256, win 128, hop 64, n_iter 32,
momentum 0.99, given initial phases.  The two forms alternate call by call inside one timed loop; per form: the median, minimum,
maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time to enqueue one call, and
the device kernels per call torch.profiler sees.  The kernel path's output is also compared with the torch loop's (complex64
drifts to ~1e-5 of the peak, so this is a sanity figure, not a parity test - that is tests/test_griffinlim_gpu.py)."""
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
N_ITER, MOMENTUM = 32, 0.99


def torch_loop(feat, u, window):
    """librosa.griffinlim in torch expressions, complex64 state as librosa keeps it."""
    S = (10.0 ** ((feat[:, 0, :NB, :NF] * 100.0 - 100.0) / 20.0) - 1e-5) * 128.0
    angles = torch.polar(torch.ones_like(u), 2.0 * math.pi * u)
    rebuilt = torch.zeros_like(angles)
    alpha = MOMENTUM / (1.0 + MOMENTUM)
    for _ in range(N_ITER):
        tprev = rebuilt
        inverse = torch.istft(S * angles, N_FFT, HOP, WIN, window, center=True)
        rebuilt = torch.stft(inverse, N_FFT, HOP, WIN, window, center=True, pad_mode="reflect", return_complex=True)
        angles = rebuilt - alpha * tprev
        angles = angles / (angles.abs() + 1e-16)
    return torch.istft(S * angles, N_FFT, HOP, WIN, window, center=True)


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "griffinlim.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    t = torch.arange(HOP * (NF - 1), dtype=torch.float32)
    wav_in = (torch.randn((B, t.numel()), generator=gen) * torch.exp(-t / 700.0)[None, :]).to(DEV)
    feat = F.PreProcess()(wav_in)
    u = torch.rand((B, NB, NF), generator=gen).to(DEV)
    window = torch.hann_window(WIN, periodic=True, device=DEV)
    wav = torch.empty((B, HOP * (NF - 1)), dtype=torch.float32, device=DEV)
    ws = U.ops.Workspace(DEV, U.ops.griffinlim_ws_bytes(B, NB, NF, N_FFT))

    forms = {"kernels_fp64": lambda: U.ops.griffinlim(feat, wav, NB, NF, N_FFT, WIN, HOP, ws, n_iter=N_ITER, momentum=MOMENTUM,
                                                       init_phase=u),
             "torch_loop_complex64": lambda: torch_loop(feat, u, window)}
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
    y_t = torch_loop(feat, u, window)
    forms["kernels_fp64"]()
    torch.cuda.synchronize()
    res = {"workload": {"batch": B, "planes": [H, W], "n_bins": NB, "n_frames": NF, "n_fft": N_FFT, "win_length": WIN,
                        "hop_length": HOP, "n_iter": N_ITER, "momentum": MOMENTUM},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "workspace_bytes": U.ops.griffinlim_ws_bytes(B, NB, NF, N_FFT),
           "max_abs_difference_over_peak": float((wav - y_t).abs().max() / y_t.abs().max())}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        print(name, json.dumps(res[name]))
    res["kernels_fp64"]["launches_per_call_by_construction"] = 2 * N_ITER + 3
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
