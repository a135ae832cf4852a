"""Time `auralize_path` (csrc/auralize_fft.hip: a moving listener by crossfaded overlap-save) against what a user could do without it
(README.md and DESIGN.md quote the file this writes).

    python scripts/time_auralize_path.py [--calls 50] [--warmup 10] [--out profiles/auralize_path.json] [--ab-lib OTHER_BUILD.so]

Workload: a path of R = 32 responses of K = 9600 taps (the reference's 0.2 s at 48 kHz) for B = 1 and B = 8 microphones, one dry signal
of N = 96 000 and 480 000 samples (2 s and 10 s) shared by the rows, the full N + K - 1 output samples, the nodes spread evenly over the
output (tau_r = round(r (L - 1) / (R - 1))).  Four forms alternate call by call inside one timed loop:

    path         auralize_path(rir, dry, times, out=out)
    composition  what the parent of this feature offers: auralize(rir.view(B R, K), dry, method="fft") - R full-length renders - followed
                 by the gain-weighted sum as a torch expression, (y.view(B, R, L) * gains).sum(1); the fp32 gains [R, L] are made once,
                 outside the timed loop
    stationary   auralize(rir[:, 0], dry, method="fft", out=out): one response per row at the same N - the floor
    path_resident  ops.auralize_path_f32(rir, times_dev, dry, out, ws=ws): the same two launches with the schedule already on the device
                 and a caller's workspace, as a loop or a captured graph calls it - `path` without the host checks of the schedule,
                 its upload and the allocation of the workspace

per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time
to enqueue one call, the device kernels per call torch.profiler sees, and the bytes of scratch memory a call needs (the workspace; for
the composition the growth of the allocator's peak over one call, output excluded).  The ratios composition / path and path /
stationary are those of the medians; `path_beats_composition_beyond_spread` says whether path's 90th percentile is below the
composition's 10th.  The largest difference between path and composition over the peak of the result is recorded as a sanity figure.

--ab-lib: another build of the library with a variant of the render kernel.  The record's was one that forms the products of two
neighbouring nodes from one reading of x's spectra (a second accumulator; it lost and is not in the source).  The C
entry points of both builds then alternate in one more loop per size: `nodes_ab` holds median, 10th and 90th percentile in ms of this
build (`nodes1`) and the other (`nodes2`) and whether the two outputs are the same bits."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U

DEV = "cuda:0"
K, R = 9600, 32
BS = (1, 8)
NS = (96000, 480000)


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


def schedule(L):
    return [int(round(r * (L - 1) / (R - 1))) for r in range(R)]


def gains(times, L):
    """fp32 [R, L] on the device: the hat functions over the nodes"""
    tau = np.asarray(times, dtype=np.int64)
    n = np.arange(L, dtype=np.int64)
    g = np.zeros((R, L))
    g[0, n <= tau[0]] = 1.0
    g[R - 1, n >= tau[R - 1]] = 1.0
    for r in range(R - 1):
        m = (n >= tau[r]) & (n < tau[r + 1])
        a = (n[m] - tau[r]) / float(tau[r + 1] - tau[r])
        g[r, m] = 1.0 - a
        g[r + 1, m] = a
    return torch.from_numpy(g.astype(np.float32)).to(DEV)


def entry(lib_path):
    """unetrir_auralize_path_f32 of another build"""
    return U._lib.bind(C.CDLL(lib_path), "unetrir_auralize_path_f32")


def nodes_ab(other, h, x, times, B, N, a):
    L = N + K - 1
    td = torch.tensor(times, dtype=torch.int32, device=DEV)
    need = U.ops.auralize_path_ws_bytes(B, R, K, N, 0, L)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    outs = {"nodes1": torch.empty((B, L), dtype=torch.float32, device=DEV), "nodes2": torch.empty((B, L), dtype=torch.float32, device=DEV)}
    fns = {"nodes1": U._lib.lib().unetrir_auralize_path_f32, "nodes2": other}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(name):
        rc = fns[name](h.data_ptr(), td.data_ptr(), x.data_ptr(), outs[name].data_ptr(), B, R, K, N, 0, L, ws.data_ptr(), need, stream)
        if rc:
            raise SystemExit(f"{name}: error {rc}")

    r = alternate({name: (lambda name=name: call(name)) for name in fns}, a)
    res = {name: [r[name]["device_ms_median"], r[name]["device_ms_p10"], r[name]["device_ms_p90"]] for name in fns}
    res["same_bits"] = bool(torch.equal(outs["nodes1"], outs["nodes2"]))
    return res


def measure(B, N, a, gen, other):
    L = N + K - 1
    t = torch.arange(K, dtype=torch.float32)
    h = (torch.randn((B, R, K), generator=gen) * torch.exp(-t / 1500.0)[None, None, :]).to(DEV)      # decaying noise: plausible responses
    x = torch.randn((N,), generator=gen).mul_(0.1).to(DEV)
    times = schedule(L)
    G = gains(times, L)
    out = torch.empty((B, L), dtype=torch.float32, device=DEV)
    out_b = torch.empty((B, L), dtype=torch.float32, device=DEV)
    h0 = h[:, 0].contiguous()

    def composition():
        y = U.auralize(h.view(B * R, K), x, method="fft")
        return (y.view(B, R, L) * G).sum(1)

    td = torch.tensor(times, dtype=torch.int32, device=DEV)
    ws = U.ops.Workspace(h.device, U.ops.auralize_path_ws_bytes(B, R, K, N, 0, L))
    out_r = torch.empty((B, L), dtype=torch.float32, device=DEV)
    forms = {"path": lambda: U.auralize_path(h, x, times, out=out), "composition": composition,
             "stationary": lambda: U.auralize(h0, x, out=out_b, method="fft"),
             "path_resident": lambda: U.ops.auralize_path_f32(h, td, x, out_r, ws=ws)}
    r = alternate(forms, a)
    for name, fn in forms.items():
        r[name]["launches_per_call"] = count_launches(fn, 4)
    r["path"]["launches_per_call_by_construction"] = 2
    r["path_resident"]["launches_per_call_by_construction"] = 2
    r["stationary"]["launches_per_call_by_construction"] = 2
    r["path"]["scratch_bytes"] = r["path_resident"]["scratch_bytes"] = U.ops.auralize_path_ws_bytes(B, R, K, N, 0, L)
    r["stationary"]["scratch_bytes"] = U.ops.auralize_fft_ws_bytes(B, K, N, 0, L)
    r["composition"]["scratch_bytes"] = scratch_bytes(composition)
    ref = composition()
    got = U.auralize_path(h, x, times)
    r["largest_difference_path_composition_over_peak"] = float((got - ref).abs().max() / ref.abs().max())
    del ref, got
    m = lambda k: r[k]["device_ms_median"]
    r["composition_over_path"] = m("composition") / m("path")
    r["path_over_stationary"] = m("path") / m("stationary")
    r["composition_over_path_resident"] = m("composition") / m("path_resident")
    r["path_resident_over_stationary"] = m("path_resident") / m("stationary")
    r["path_beats_composition_beyond_spread"] = bool(r["path"]["device_ms_p90"] < r["composition"]["device_ms_p10"])
    r["node_spacing_samples"] = (L - 1) / (R - 1)
    if other is not None:
        r["nodes_ab"] = nodes_ab(other, h, x, times, B, N, a)
    for name in list(forms) + ["composition_over_path", "path_over_stationary", "composition_over_path_resident",
                               "path_resident_over_stationary", "path_beats_composition_beyond_spread"] + (
            ["nodes_ab"] if other is not None else []):
        print(B, N, name, json.dumps(r[name]))
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "auralize_path.json"))
    ap.add_argument("--ab-lib", default=None)
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    other = entry(a.ab_lib) if a.ab_lib else None
    res = {"workload": {"taps": K, "nodes": R, "batches": list(BS), "dry_samples": list(NS), "dry": "shared", "output": "full",
                        "schedule": "tau_r = round(r (L - 1) / (R - 1))", "block": U.ops.auralize_fft_block(K)},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for B in BS:
        for N in NS:
            res[f"B={B} N={N}"] = measure(B, N, a, gen, other)
            with open(a.out, "w") as f:                           # after every size: a later failure keeps the earlier figures
                json.dump(res, f, indent=1)
                f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
