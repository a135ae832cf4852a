"""Time `auralize` (csrc/auralize.hip: direct form on the fp32 matrix cores, one launch) against the same convolution written as torch
expressions kept on the device: a grouped torch.nn.functional.conv1d, and torch.fft.rfft . irfft (informational; README.md and
DESIGN.md quote the file this writes).  Nothing is expected in advance: by operation count the FFT form needs far less arithmetic at
K = 9600, and the file records whichever way it comes out.

    python scripts/time_auralize.py [--calls 50] [--warmup 10] [--out profiles/auralize.json]

Workload: B = 32 impulse responses of K = 9600 taps (the reference's 0.2 s at 48 kHz), a dry signal of N = 96 000 and 480 000 samples
(2 s and 10 s), x shared by the rows and one x per row, the full N + K - 1 output samples.  All forms of one N alternate call by call
inside one timed loop; per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events,
the median host time to enqueue one call, and the device kernels per call torch.profiler sees.  A torch form whose single call takes
longer than --slow-ms is timed --slow-calls times instead (its entry says so); one that raises is recorded with its error.  The FFT
form transforms at the next power of two >= N + K - 1.  The kernel's share of the fp32 matrix peak counts the 2 B K N useful flops
against 157.3 TFLOP/s."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

import unet_rir_amd as U

DEV = "cuda:0"
B, K = 32, 9600
NS = (96000, 480000)
PEAK_FP32_MATRIX = 157.3e12


def conv1d_form(h, x):
    """y = h * x as a grouped correlation with the flipped responses: x padded by K - 1 zeros on both sides"""
    w = h.flip(1).unsqueeze(1)                                    # [B, 1, K]
    if x.dim() == 1:
        return F.conv1d(F.pad(x, (K - 1, K - 1)).view(1, 1, -1), w)[0]
    return F.conv1d(F.pad(x, (K - 1, K - 1)).unsqueeze(0), w, groups=B)[0]


def fft_form(h, x):
    n = x.shape[-1] + K - 1
    size = 1 << (n - 1).bit_length()
    return torch.fft.irfft(torch.fft.rfft(h, size) * torch.fft.rfft(x, size), size)[:, :n]


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
    q = statistics.quantiles(dev_ms, n=10) if len(dev_ms) >= 2 else [dev_ms[0], dev_ms[0]]
    return {"calls": len(dev_ms), "device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "device_ms_max": max(dev_ms),
            "device_ms_p10": q[0], "device_ms_p90": q[-1], "host_enqueue_us_median": statistics.median(host_us)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e6
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def measure(N, a, gen):
    t = torch.arange(K, dtype=torch.float32)
    h = (torch.randn((B, K), generator=gen) * torch.exp(-t / 1500.0)[None, :]).to(DEV)       # decaying noise: a plausible response
    xr = torch.randn((B, N), generator=gen).mul_(0.1).to(DEV)
    xs = xr[0].contiguous()
    out = torch.empty((B, N + K - 1), dtype=torch.float32, device=DEV)
    forms = {"kernel_shared": lambda: U.auralize(h, xs, out=out), "kernel_rows": lambda: U.auralize(h, xr, out=out),
             "conv1d_shared": lambda: conv1d_form(h, xs), "conv1d_rows": lambda: conv1d_form(h, xr),
             "fft_shared": lambda: fft_form(h, xs), "fft_rows": lambda: fft_form(h, xr)}
    res, calls = {}, {}
    for name in list(forms):                                      # first call: does it run, and is it slow
        try:
            ms, _ = timed(forms[name])
            ms, _ = timed(forms[name])
            calls[name] = a.calls if ms <= a.slow_ms else a.slow_calls
            if ms > a.slow_ms:
                print(f"N={N} {name}: {ms:.1f} ms per call, timed {a.slow_calls} times", file=sys.stderr)
        except Exception as exc:
            res[name] = {"error": f"{type(exc).__name__}: {exc}"[:400]}
            print(f"N={N} {name} failed: {exc}", file=sys.stderr)
            del forms[name]
            torch.cuda.synchronize()
    for i in range(a.warmup):
        for name, fn in forms.items():
            if i < calls[name]:
                fn()
    torch.cuda.synchronize()
    dev_ms, host_us = {k: [] for k in forms}, {k: [] for k in forms}
    for i in range(a.calls):
        for name, fn in forms.items():
            if i < calls[name]:
                ms, host = timed(fn)
                dev_ms[name].append(ms)
                host_us[name].append(host)
    ref = fft_form(h.double(), xr.double())
    peak = float(ref.abs().max())
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 2 if calls[name] < a.calls else 4)
        if name.endswith("_rows"):
            res[name]["max_abs_difference_from_fp64_fft_over_peak"] = float((fn().double() - ref).abs().max()) / peak
        print(N, name, json.dumps(res[name]))
    flops = 2.0 * B * K * N
    for name in ("kernel_shared", "kernel_rows"):
        res[name]["launches_per_call_by_construction"] = 1
        res[name]["useful_tflops"] = flops / (res[name]["device_ms_median"] * 1e-3) / 1e12
        res[name]["share_of_fp32_matrix_peak"] = flops / (res[name]["device_ms_median"] * 1e-3) / PEAK_FP32_MATRIX
    m = lambda k: res[k].get("device_ms_median")
    for other in ("conv1d", "fft"):
        for mode in ("shared", "rows"):
            if m(f"{other}_{mode}") is not None:
                res[f"{other}_{mode}_over_kernel_{mode}"] = m(f"{other}_{mode}") / m(f"kernel_{mode}")
    res["useful_flops"] = flops
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--slow-ms", type=float, default=200.0)
    ap.add_argument("--slow-calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "auralize.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    res = {"workload": {"batch": B, "taps": K, "dry_samples": list(NS), "output": "full", "fft_size": "next power of two"},
           "calls": a.calls, "warmup": a.warmup, "slow_ms": a.slow_ms, "slow_calls": a.slow_calls,
           "device": torch.cuda.get_device_name(0), "fp32_matrix_peak_tflops": PEAK_FP32_MATRIX / 1e12}
    for N in NS:
        res[f"N={N}"] = measure(N, a, gen)
        with open(a.out, "w") as f:                               # after every N: a later failure keeps the earlier figures
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
