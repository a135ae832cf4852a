"""Time the two forms of the Griffin-Lim reconstruction of a batch against each other: ops.griffinlim (csrc/griffinlim.hip: fp64 state,
fp64 DFTs on the matrix cores, 2 n_iter + 3 launches) and ops.griffinlim_fft (csrc/griffinlim_fft.hip: fp32 state, fp32 FFTs held in LDS,
n_iter + 2 launches) (informational; README.md and DESIGN.md quote the file this writes).

    python scripts/time_griffinlim_fft.py [--calls 50] [--warmup 10] [--out profiles/griffinlim_fft.json]

Workload, the protocol of scripts/time_griffinlim.py: batch 32, 129 x 151 bins x frames inside 144 x 160 planes (dataset.py:62-70), n_fft
256, win 128, hop 64, n_iter 32, momentum 0.99, given initial phases.  The two forms alternate call by call inside one timed loop; per form:
the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time to enqueue
one call, the device kernels per call torch.profiler sees, the workspace, and the largest and the RMS error of the batch against the fp64
restatement tests/griffinlim_ref.py on the same fp32 inputs, both over the peak of the row (sanity figures, not a parity test - those are
tests/test_griffinlim_gpu.py and tests/test_griffinlim_fft_gpu.py), with the spectral convergence || |stft(y)| - S || / || S || of both."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import unet_rir_amd as U
from unet_rir_amd import features as F

DEV = "cuda:0"
B, H, W = 32, 144, 160
NB, NF = F.STFT_SHAPE
N_FFT, WIN, HOP = F.N_FFT, F.WIN_LENGTH, F.HOP_LENGTH
N_ITER, MOMENTUM = 32, 0.99


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "griffinlim_fft.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    import griffinlim_ref as GR
    gen = torch.Generator(); gen.manual_seed(1)
    t = torch.arange(HOP * (NF - 1), dtype=torch.float32)
    wav_in = (torch.randn((B, t.numel()), generator=gen) * torch.exp(-t / 700.0)[None, :]).to(DEV)
    feat = F.PreProcess()(wav_in)
    u = torch.rand((B, NB, NF), generator=gen).to(DEV)
    ops = U.ops
    need = {"dft_fp64": ops.griffinlim_ws_bytes(B, NB, NF, N_FFT), "fft_fp32": ops.griffinlim_fft_ws_bytes(B, NB, NF, N_FFT, WIN, HOP)}
    wav = {k: torch.empty((B, HOP * (NF - 1)), dtype=torch.float32, device=DEV) for k in need}
    ws = {k: ops.Workspace(DEV, n) for k, n in need.items()}
    kw = dict(n_iter=N_ITER, momentum=MOMENTUM, init_phase=u)
    forms = {"dft_fp64": lambda: ops.griffinlim(feat, wav["dft_fp64"], NB, NF, N_FFT, WIN, HOP, ws["dft_fp64"], **kw),
             "fft_fp32": lambda: ops.griffinlim_fft(feat, wav["fft_fp32"], NB, NF, N_FFT, WIN, HOP, ws["fft_fp32"], **kw)}
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
    res = {"workload": {"batch": B, "planes": [H, W], "n_bins": NB, "n_frames": NF, "n_fft": N_FFT, "win_length": WIN,
                        "hop_length": HOP, "n_iter": N_ITER, "momentum": MOMENTUM},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        res[name]["workspace_bytes"] = need[name]
    res["dft_fp64"]["launches_per_call_by_construction"] = 2 * N_ITER + 3
    res["fft_fp32"]["launches_per_call_by_construction"] = N_ITER + 2
    res["speedup_device_median"] = res["dft_fp64"]["device_ms_median"] / res["fft_fp32"]["device_ms_median"]
    # both against the fp64 restatement on this batch, on the host
    feat_h, u_h = feat.cpu().numpy(), u.cpu().numpy()
    ref = np.stack([GR.feature_to_wav(feat_h[b], u_h[b], (NB, NF), N_FFT, WIN, HOP, n_iter=N_ITER, momentum=MOMENTUM) for b in range(B)])
    S = np.stack([GR.FO.denormalize(feat_h[b, 0, :NB, :NF].astype(np.float64), 0.0)[0] for b in range(B)])
    peak = np.abs(ref).max(axis=1, keepdims=True)
    conv_ref = [GR.spectral_convergence(ref[b], S[b], N_FFT, WIN, HOP) for b in range(B)]
    res["fp64_restatement"] = {"spectral_convergence_mean": float(np.mean(conv_ref))}
    for name in forms:
        y = wav[name].cpu().numpy().astype(np.float64)
        d = (y - ref) / peak
        conv = [GR.spectral_convergence(y[b], S[b], N_FFT, WIN, HOP) for b in range(B)]
        res[name].update({"max_error_over_peak": float(np.abs(d).max()), "rms_error_over_peak": float(np.sqrt((d * d).mean())),
                          "spectral_convergence_mean": float(np.mean(conv)),
                          "spectral_convergence_max_relative_difference_from_fp64": float(max(abs(c - r) / r for c, r in zip(conv, conv_ref)))})
        print(name, json.dumps(res[name]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
