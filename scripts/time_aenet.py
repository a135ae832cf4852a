"""Time the 2x2 stride-2 kernels (csrc/conv2x2.hip) against the generic entry points on the same buffers, layer by layer
(informational; README.md and DESIGN.md quote the record).  No threshold: the record is the deliverable.

    python scripts/time_aenet.py [--samples 50] [--warmup 10] [--out profiles/aenet.json]

Layers: every Conv2D(k=2, strides=2) and Conv2DTranspose(k=2, strides=2) of the default AENet (dl_models/ae_net.py:206-243 with
number_filters_0 = 32) at 144 x 160, batch 32, bf16 storage - the transposed ones writing into the upper half of their concat
buffer, as the decoder does - in all three passes (forward, data gradient, weight gradient with the l2 term).
Per (layer, pass) the two variants ALTERNATE in one process, twice each (new, generic, new, generic): every run is the median over
--samples samples, after --warmup warm-ups, of the device time between two HIP events around REPS back-to-back calls, divided by
REPS.  `spread` is the relative distance between the two medians of the same variant, `not_slower` says whether the new kernel's
slower median is within the generic kernel's faster median times (1 + the larger spread).  `bytes` is what the algorithm has to
move (both activation tensors once, the kernel once, the fp32 weight gradient once), `hbm_share` that over the time as a share of
the 8.0 TB/s HBM3E rate (6.29 TB/s is what a float4 copy reaches) - the algorithm's bytes over the time, NOT achieved HBM traffic: the
same 10-70 MB buffers are used call after call, so the deep layers' tensors stay in L2 / Infinity Cache.  `offered` is what unetrir_conv2x2s2_*supported_bf16 answers
for the layer: the rule in csrc/api.hip (C22_GEMM_MAX_K) was set from this record and must agree with its `not_slower` column.
Whole step: `Trainer.step` of the default AENetEngine (144 x 160, batch 32, bf16) with the 2x2 layers on the passes the predicate
offers and with every one of them forced to the generic kernels (generic_conv2x2=True), the two engines alternating in one process:
median device time per step, host time to enqueue a step, device kernels per step."""
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
H, W, B, F0 = 144, 160, 32, 32
REPS = 5
HBM_PEAK = 8.0e12


def layers():
    """(name, transposed, H, W of the layer input, Cin, Cout) of the default model."""
    out, h, w = [], H, W
    for l in range(2, 6):
        out.append((f"enc{l}.down", False, h, w, F0 << (l - 2), F0 << (l - 1)))
        h, w = h // 2, w // 2
    for l in range(4, 0, -1):
        out.append((f"dec{l}.up", True, h, w, F0 << l, F0 << (l - 1)))
        h, w = 2 * h, 2 * w
    return out


def event_us(fn, samples, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / REPS)
    return statistics.median(us)


def compare(new, old, nbytes, samples, warmup):
    runs = {"conv2x2": [], "generic": []}
    for _ in range(2):
        runs["conv2x2"].append(event_us(new, samples, warmup))
        runs["generic"].append(event_us(old, samples, warmup))
    spread = {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}
    rec = {"conv2x2_us": runs["conv2x2"], "generic_us": runs["generic"], "spread": spread, "bytes": nbytes,
           "hbm_share": {k: nbytes / (min(v) * 1e-6) / HBM_PEAK for k, v in runs.items()},
           "generic_over_conv2x2": min(runs["generic"]) / min(runs["conv2x2"]),
           "not_slower": max(runs["conv2x2"]) <= min(runs["generic"]) * (1.0 + max(spread.values()))}
    return rec


def layer(name, tr, h, w, ci, co, samples, warmup):
    ops = U.ops
    gen = torch.Generator(device=DEV); gen.manual_seed(h * 1000 + ci)
    rnd = lambda *sh: ((torch.rand(sh, device=DEV, generator=gen) - 0.5) * 2).to(torch.bfloat16)
    g = ops.geom(B, h, w, ci, co, 2, 2)
    ho, wo = (2 * h, 2 * w) if tr else (h // 2, w // 2)
    x, gx = ops.Act(rnd(B, h, w, ci)), ops.Act(rnd(B, h, w, ci))
    if tr:          # into the upper half of the concat buffer
        y, gy = ops.Act(rnd(B, ho, wo, 2 * co), co, co), ops.Act(rnd(B, ho, wo, 2 * co), co, co)
    else:
        y, gy = ops.Act(rnd(B, ho, wo, co)), ops.Act(rnd(B, ho, wo, co))
    offered = ops.conv2x2s2_supported(g, x, y, transpose=tr)       # the passes the library's predicate keeps on the new kernels
    assert offered & ops.C22_WGRAD, name
    rows, cols = (ci, co) if tr else (co, ci)           # primary layout [rows][2][2][cols]
    w32 = (torch.rand((rows, 4, cols), device=DEV, generator=gen) - 0.5) * 0.2
    same, swapped = torch.empty((rows, 4, cols), dtype=torch.bfloat16, device=DEV), torch.zeros((cols, 4, rows), dtype=torch.bfloat16, device=DEV)
    ops.cast_weight_bf16(w32, same, rows, 4, cols, cols)
    ops.transpose_cast_weight_bf16(w32, swapped, rows, 4, cols, rows)
    bias = torch.rand(co, device=DEV, generator=gen)
    dw, ws = torch.empty_like(w32), ops.Workspace(DEV)
    if tr:
        fwd = (lambda: ops.conv2x2s2_transpose_fwd(g, x, swapped, bias, y), lambda: ops.conv2d_transpose_fwd(g, x, swapped, bias, y))
        dgrad = (lambda: ops.conv2x2s2_transpose_dgrad(g, gy, same, gx), lambda: ops.conv2d_transpose_dgrad(g, gy, same, gx))
        wgrad = (lambda: ops.conv2x2s2_transpose_wgrad(g, x, gy, dw, ws, reg=2e-3, w=w32),
                 lambda: ops.conv2d_transpose_wgrad(g, x, gy, dw, ws, reg=2e-3, w=w32))
    else:
        fwd = (lambda: ops.conv2x2s2_fwd(g, x, same, bias, y), lambda: ops.conv2d_fwd(g, x, same, bias, y))
        dgrad = (lambda: ops.conv2x2s2_dgrad(g, gy, swapped, gx), lambda: ops.conv2d_dgrad(g, gy, swapped, gx))
        wgrad = (lambda: ops.conv2x2s2_wgrad(g, x, gy, dw, ws, reg=2e-3, w=w32), lambda: ops.conv2d_wgrad(g, x, gy, dw, ws, reg=2e-3, w=w32))
    act_bytes = 2 * (B * h * w * ci + B * ho * wo * co)
    rec = {"transposed": tr, "input": [B, h, w, ci], "output": [B, ho, wo, co],
           "offered": {"forward": bool(offered & ops.C22_FWD), "data_gradient": bool(offered & ops.C22_DGRAD),
                       "weight_gradient": bool(offered & ops.C22_WGRAD)},
           "forward": compare(*fwd, act_bytes + 2 * 4 * ci * co, samples, warmup),
           "data_gradient": compare(*dgrad, act_bytes + 2 * 4 * ci * co, samples, warmup),
           "weight_gradient": compare(*wgrad, act_bytes + 2 * 4 * 4 * ci * co, samples, warmup)}
    print(name, json.dumps(rec))
    return rec


def whole_step(samples, warmup):
    gen = torch.Generator(); gen.manual_seed(1)
    data = (torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
            torch.rand((B, 2, H, W), generator=gen).to(DEV))
    trainers = {}
    for name, generic in (("conv2x2", False), ("generic", True)):
        eng = U.AENetEngine(H, W, B, F0=F0, device=DEV, dtype="bf16", generic_conv2x2=generic)
        eng.reset_parameters(torch.Generator().manual_seed(0))
        trainers[name] = U.Trainer(eng, lr=5e-7)
    runs = {k: {"ms": [], "host_us": []} for k in trainers}
    for _ in range(2):
        for name, tr in trainers.items():
            for _ in range(warmup):
                tr.step(*data)
            torch.cuda.synchronize()
            dev_ms, host_us = [], []
            for _ in range(samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                tr.step(*data)
                host_us.append((time.perf_counter() - t0) * 1e6)
                e1.record()
                torch.cuda.synchronize()
                dev_ms.append(e0.elapsed_time(e1))
            runs[name]["ms"].append(statistics.median(dev_ms))
            runs[name]["host_us"].append(statistics.median(host_us))
    rec = {"geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0, "storage": "bf16"}}
    for name, tr in trainers.items():
        rec[name] = {"step_ms": runs[name]["ms"], "host_enqueue_us": runs[name]["host_us"], "launches_per_step": count_launches(lambda: tr.step(*data), 4),
                     "passes": dict(tr.engine.c22_passes), "loss": float(tr.engine.loss_out[0])}
    rec["generic_over_conv2x2"] = min(rec["generic"]["step_ms"]) / min(rec["conv2x2"]["step_ms"])
    print("whole_step", json.dumps(rec))
    return rec


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aenet.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    if a.samples < 50 or a.warmup < 10:
        print("note: fewer than 50 samples or 10 warm-ups - not the record's conditions", file=sys.stderr)
    res = {"samples": a.samples, "warmup": a.warmup, "reps_per_sample": REPS, "device": torch.cuda.get_device_name(0), "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0, "storage": "bf16"}, "hbm_peak_bytes_per_s": HBM_PEAK,
           "layers": {n: layer(n, tr, h, w, ci, co, a.samples, a.warmup) for n, tr, h, w, ci, co in layers()}}
    res["whole_step"] = whole_step(a.samples, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
