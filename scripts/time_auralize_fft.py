"""Time the two forms of `auralize` - method="direct" (csrc/auralize.hip: one fma per tap on the fp32 matrix cores) and method="fft"
(csrc/auralize_fft.hip: partitioned overlap-save, FFTs in LDS) - against the same convolution written as torch.fft.rfft . irfft on the
device (README.md and DESIGN.md quote the file this writes).

    python scripts/time_auralize_fft.py [--calls 50] [--warmup 10] [--out profiles/auralize_fft.json]

Workload: B = 32 impulse responses of K = 9600 taps (the reference's 0.2 s at 48 kHz), a dry signal of N = 96 000 and 480 000 samples
(2 s and 10 s), x shared by the rows and one x per row, the full N + K - 1 output samples.  The three forms of one layout alternate call
by call inside one timed loop; per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP
events, the median host time to enqueue one call, the device kernels per call torch.profiler sees, the bytes of scratch memory a call
needs (the workspace of the FFT form; for the torch expression the growth of the allocator's peak over one call, output excluded), and
the largest and the RMS error against the same expression in fp64 on one batch.  The torch form transforms at the next power of two
>= N + K - 1.  A sweep over K = 32, 256, 1024, 4096 at N = 96 000 (x shared) locates the crossover between the two forms of the library."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U

DEV = "cuda:0"
B, K = 32, 9600
NS = (96000, 480000)
SWEEP_K = (32, 256, 1024, 4096)


def torch_form(h, x):
    n = x.shape[-1] + h.shape[-1] - 1
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
    q = statistics.quantiles(dev_ms, n=10)
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


def alternate(forms, a):
    """Every form called in turn: a.warmup rounds untimed, then a.calls timed rounds -> {name: summary}"""
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    dev_ms, host_us = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.calls):
        for name, fn in forms.items():
            ms, host = timed(fn)
            dev_ms[name].append(ms)
            host_us[name].append(host)
    return {name: summary(dev_ms[name], host_us[name]) for name in forms}


def scratch_bytes(fn):
    """Growth of the allocator's peak over one call, minus what the call returns"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    y = fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base - y.numel() * y.element_size()


def data(k, N, gen):
    t = torch.arange(k, dtype=torch.float32)
    h = (torch.randn((B, k), generator=gen) * torch.exp(-t / 1500.0)[None, :]).to(DEV)       # decaying noise: a plausible response
    xr = torch.randn((B, N), generator=gen).mul_(0.1).to(DEV)
    return h, xr, xr[0].contiguous()


def measure(N, a, gen):
    h, xr, xs = data(K, N, gen)
    out = torch.empty((B, N + K - 1), dtype=torch.float32, device=DEV)
    ref = torch_form(h.double(), xr.double())
    res = {}
    for mode, x in (("shared", xs), ("rows", xr)):
        forms = {"direct": lambda x=x: U.auralize(h, x, out=out), "fft": lambda x=x: U.auralize(h, x, out=out, method="fft"),
                 "torch_fft": lambda x=x: torch_form(h, x)}
        r = alternate(forms, a)
        for name, fn in forms.items():
            r[name]["launches_per_call"] = count_launches(fn, 4)
            y = fn().double()
            want = ref if mode == "rows" else None
            if want is None:
                want = torch_form(h.double(), x.double())
            r[name]["max_abs_error_vs_fp64"] = float((y - want).abs().max())
            r[name]["rms_error_vs_fp64"] = float((y - want).pow(2).mean().sqrt())
            r[name]["rms_of_fp64_result"] = float(want.pow(2).mean().sqrt())
            del y, want
        stride = 0 if mode == "shared" else N
        r["direct"]["scratch_bytes"] = 0
        r["fft"]["scratch_bytes"] = U.ops.auralize_fft_ws_bytes(B, K, N, stride, N + K - 1)
        r["torch_fft"]["scratch_bytes"] = scratch_bytes(forms["torch_fft"])
        r["direct"]["launches_per_call_by_construction"] = 1
        r["fft"]["launches_per_call_by_construction"] = 2
        m = lambda k: r[k]["device_ms_median"]
        r["direct_over_fft"] = m("direct") / m("fft")
        r["torch_fft_over_fft"] = m("torch_fft") / m("fft")
        res[mode] = r
        for name in forms:
            print(N, mode, name, json.dumps(r[name]))
    return res


def sweep(a, gen):
    N = NS[0]
    res = {}
    for k in SWEEP_K:
        h, _, xs = data(k, N, gen)
        out = torch.empty((B, N + k - 1), dtype=torch.float32, device=DEV)
        r = alternate({"direct": lambda: U.auralize(h, xs, out=out), "fft": lambda: U.auralize(h, xs, out=out, method="fft")}, a)
        res[f"K={k}"] = {"direct_ms_median": r["direct"]["device_ms_median"], "fft_ms_median": r["fft"]["device_ms_median"],
                         "direct_ms_p10_p90": [r["direct"]["device_ms_p10"], r["direct"]["device_ms_p90"]],
                         "fft_ms_p10_p90": [r["fft"]["device_ms_p10"], r["fft"]["device_ms_p90"]],
                         "direct_over_fft": r["direct"]["device_ms_median"] / r["fft"]["device_ms_median"]}
        print("sweep", k, json.dumps(res[f"K={k}"]))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "auralize_fft.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    res = {"workload": {"batch": B, "taps": K, "dry_samples": list(NS), "output": "full", "torch_fft_size": "next power of two",
                        "fft_block": U.ops.auralize_fft_block(K)},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for N in NS:
        res[f"N={N}"] = measure(N, a, gen)
        with open(a.out, "w") as f:                               # after every N: a later failure keeps the earlier figures
            json.dump(res, f, indent=1)
            f.write("\n")
    res[f"sweep_N={NS[0]}_shared"] = sweep(a, gen)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
