"""Time the resampler (csrc/resample.hip through `unet_rir_amd.Resampler`) against the same table through torch on the device and against
a device-to-device copy of the bytes it has to move (README.md and DESIGN.md quote the file this writes).

    python scripts/time_resample.py [--calls 50] [--warmup 10] [--out profiles/resample.json]

Workload: 10 s of audio, B = 1 and 32 rows, 44100 -> 48000 (L / M = 160 / 147), 48000 -> 16000 (1 / 3) and 16000 -> 48000 (3 / 1), both
presets.  Three forms alternate call by call inside one timed loop:

  kernel      `Resampler.__call__` into a preallocated output: one launch
  torch       the SAME fp32 table as one strided convolution: output m = j L + r reads x from j M + o(r) on, o(r) = (r M) div L, so row
              (r M) mod L of the table is laid into a weight of T + M - 1 taps at offset o(r), channel r;
              F.conv1d(pad(x), weight[:, None, :], stride=M) gives z[b, r, j], and y = z.permute(0, 2, 1).reshape(B, -1)[:, :Nout]
              (the pad, the convolution and the interleave are all timed: that is the expression a user would write)
  copy        dst.copy_(src) of 4 B (N + Nout) bytes: what reading x once and writing y once costs on this device

Per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time to
enqueue one call and the device kernels per call torch.profiler sees; for kernel and torch the largest error against the torch form in
fp64 on the first row; the algorithm's 2 B Nout T floating-point operations and 4 B (N + Nout) bytes, and the rates they come to."""
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
SECONDS = 10
BATCHES = (1, 32)
RATES = ((44100, 48000), (48000, 16000), (16000, 48000))
PRESETS = ("kaiser_best", "kaiser_fast")


def torch_weight(table, L, M):
    """fp32 [L, T + M - 1]: channel r holds row (r M) mod L of the table from tap o(r) = (r M) div L on"""
    T = table.shape[1]
    w = torch.zeros((L, T + M - 1), dtype=table.dtype, device=table.device)
    for r in range(L):
        o = (r * M) // L
        w[r, o:o + T] = table[(r * M) % L]
    return w


def torch_form(x, w, L, M, T, Nout):
    periods = -(-Nout // L)
    need = (periods - 1) * M + w.shape[1]                       # samples of the padded signal the last period reads
    left = T // 2 - 1
    xp = F.pad(x, (left, max(0, need - left - x.shape[1])))
    z = F.conv1d(xp[:, None, :], w[:, None, :], stride=M)[:, :, :periods]
    return z.permute(0, 2, 1).reshape(x.shape[0], -1)[:, :Nout]


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


def measure(rate_in, rate_out, res_type, B, a, gen):
    r = U.Resampler(rate_in, rate_out, res_type, device=DEV)
    L, M, T = r.L, r.M, r.taps
    N = SECONDS * rate_in
    Nout = r.out_length(N)
    x = torch.randn((B, N), generator=gen).mul_(0.1).to(DEV)
    out = torch.empty((B, Nout), dtype=torch.float32, device=DEV)
    w = torch_weight(r.table, L, M)
    src = torch.empty(B * (N + Nout), dtype=torch.float32, device=DEV).normal_()
    dst = torch.empty_like(src)
    forms = {"kernel": lambda: r(x, out=out), "torch": lambda: torch_form(x, w, L, M, T, Nout), "copy": lambda: dst.copy_(src)}
    res = alternate(forms, a)
    want = torch_form(x[:1].double(), w.double(), L, M, T, Nout)
    for name in ("kernel", "torch"):
        res[name]["launches_per_call"] = count_launches(forms[name], 4)
        y = forms[name]()[:1].double()
        res[name]["max_abs_error_vs_fp64"] = float((y - want).abs().max())
    res["kernel"]["launches_per_call_by_construction"] = 1
    res["rms_of_fp64_result"] = float(want.pow(2).mean().sqrt())
    flops, nbytes = 2 * B * Nout * T, 4 * B * (N + Nout)
    m = lambda k: res[k]["device_ms_median"]
    res.update({"L": L, "M": M, "taps": T, "N": N, "Nout": Nout, "flops": flops, "bytes": nbytes,
                "kernel_tflops": flops / m("kernel") * 1e-9, "kernel_gbytes_per_s": nbytes / m("kernel") * 1e-6,
                "copy_gbytes_per_s": 2 * nbytes / m("copy") * 1e-6,          # a copy reads and writes every byte
                "torch_over_kernel": m("torch") / m("kernel"), "copy_over_kernel": m("copy") / m("kernel"),
                "kernel_beyond_spread_of_torch": res["kernel"]["device_ms_p90"] < res["torch"]["device_ms_p10"]})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "resample.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    res = {"workload": {"seconds": SECONDS, "batches": list(BATCHES), "rates": [list(r) for r in RATES], "presets": list(PRESETS)},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for rate_in, rate_out in RATES:
        for res_type in PRESETS:
            for B in BATCHES:
                key = f"{rate_in}->{rate_out} {res_type} B={B}"
                res[key] = measure(rate_in, rate_out, res_type, B, a, gen)
                print(key, json.dumps(res[key]))
                with open(a.out, "w") as f:                       # after every case: a later failure keeps the earlier figures
                    json.dump(res, f, indent=1)
                    f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
