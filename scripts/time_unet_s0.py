"""Time the folded up-sampling head (csrc/head_up2.hip: UpSampling2D((2, 2)) -> Conv2D(2, (6,6)), dl_models/u_net.py:247-248) against
its literal twin on the same data, and the whole bf16 step of BASELINE.json configs[1]'s model at resize_factor_0 = [2, 2] beside
[1, 1] (informational; README.md and DESIGN.md quote the record).  The record decides what unetrir_head_up2_supported_* offers: a pass
stays in the mask only if its `not_slower` is true at the default head.

    python scripts/time_unet_s0.py [--samples 50] [--warmup 10] [--out profiles/unet_s0.json]

(a) Head of number_filters_0 = 64 at 256 x 256 (coarse 128 x 128), batch 32, both storage types.  New: head_up2_fwd / _dgrad / _wgrad on
the coarse tensor.  Twin: the up-sampled tensor materialised (torch repeat_interleave on both axes, written into a preallocated
buffer; the data gradient's 2 x 2 sum likewise) and the 6x6 head kernels at the fine size - head6x6_fwd, head6x6_wgrad and the data
gradient the engines use there (bf16: head6x6_dgrad on the matrix cores; fp32: the tap-table kernel).  Per pass the two variants
ALTERNATE in one process, twice each (new, twin, new, twin): every run is the median over --samples samples, after --warmup warm-ups,
of the device time between two HIP events around REPS back-to-back calls, divided by REPS.  `spread` is the relative distance between
the two medians of one variant, `not_slower` says whether the new kernel's slower median is within the twin's faster median times
(1 + the larger spread).  `bytes` is what the folded algorithm has to move (the coarse activations or their gradient once, the fine
logits or their gradients once) and `copy_share` that over the time as a share of the rate a device-to-device copy of the coarse
activation tensor reaches in the same process - the algorithm's bytes over the time, NOT achieved HBM traffic.
(b) `Trainer.step` of UNetEngine(256, 256, 32, F0=64, bf16, overlap) at s0 = 2 and s0 = 1, alternating in one process: median
device time per step."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U

DEV = "cuda:0"
H, W, B, F0 = 256, 256, 32, 64
REPS = 5


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


def compare(new, old, nbytes, copy_rate, samples, warmup):
    runs = {"head_up2": [], "twin": []}
    for _ in range(2):
        runs["head_up2"].append(event_us(new, samples, warmup))
        runs["twin"].append(event_us(old, samples, warmup))
    spread = {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}
    return {"head_up2_us": runs["head_up2"], "twin_us": runs["twin"], "spread": spread, "bytes": nbytes,
            "bytes_per_s": {k: nbytes / (min(v) * 1e-6) for k, v in runs.items()},
            "copy_share": {k: nbytes / (min(v) * 1e-6) / copy_rate for k, v in runs.items()},
            "twin_over_head_up2": min(runs["twin"]) / min(runs["head_up2"]),
            "not_slower": max(runs["head_up2"]) <= min(runs["twin"]) * (1.0 + max(spread.values()))}


def head(storage, samples, warmup):
    ops = U.ops
    dt, PAD, es = (torch.float32, 4, 4) if storage == "f32" else (torch.bfloat16, 8, 2)
    Cc, h, w = F0, H // 2, W // 2
    gen = torch.Generator(device=DEV); gen.manual_seed(7)
    rnd = lambda *sh: ((torch.rand(sh, device=DEV, generator=gen) - 0.5) * 2).to(dt)
    x, gx = ops.Act(rnd(B, h, w, Cc)), ops.Act(rnd(B, h, w, Cc))
    xup, gxup = ops.new_act(B, H, W, Cc, DEV, dtype=dt), ops.new_act(B, H, W, Cc, DEV, dtype=dt)
    y = ops.new_act(B, H, W, 4, DEV)
    gy = ops.Act(rnd(B, H, W, PAD))
    gy.base[..., 2:] = 0
    wm = torch.zeros((PAD, 6, 6, Cc), device=DEV)
    wm[:2] = (torch.rand((2, 6, 6, Cc), device=DEV, generator=gen) - 0.5) * 0.2
    bias = torch.zeros(PAD, device=DEV)
    wf = torch.zeros(ops.head_up2_folded_elems(Cc), device=DEV)
    ops.head_up2_fold(wm, wf, Cc, storage == "bf16")
    g = ops.geom(B, H, W, Cc, PAD, 6, 1)
    wt = wm.permute(3, 1, 2, 0).contiguous()                    # [C][6][6][PAD] for the tap-table data gradient
    wt16 = wt.to(torch.bfloat16)
    dw, ws = torch.zeros_like(wm), ops.Workspace(DEV)
    scratch = torch.empty_like(x.base)
    copy_us = event_us(lambda: scratch.copy_(x.base), samples, warmup)
    P, Pf = B * h * w, B * H * W
    copy_rate = 2.0 * es * P * Cc / (copy_us * 1e-6)
    up_view = xup.base.view(B, h, 2, w, 2, Cc)

    def upsample():
        up_view.copy_(x.base.view(B, h, 1, w, 1, Cc).expand(B, h, 2, w, 2, Cc))

    def twin_fwd():
        upsample()
        ops.head6x6_fwd(xup, wm, bias, y)

    def twin_dgrad():
        if storage == "bf16" and ops.head6x6_dgrad_supported(W, Cc):
            ops.head6x6_dgrad(gy, wm, gxup)
        else:
            ops.conv2d_dgrad(g, gy, wt16 if storage == "bf16" else wt, gxup)
        cells = gxup.base.view(B, h, 2, w, 2, Cc)               # the adjoint of the up-sampling: the sum over every 2 x 2 cell
        if storage == "f32":
            torch.sum(cells, dim=(2, 4), out=gx.base)
        else:
            gx.base.copy_(cells.sum(dim=(2, 4), dtype=torch.float32))

    def twin_wgrad():
        upsample()
        ops.head6x6_wgrad(xup, gy, dw, ws)
    act = es * P * Cc
    rec = {"input": [B, h, w, Cc], "storage": storage, "offered": ops.head_up2_supported(Cc, storage),
           "workspace_bytes": ops.head_up2_wgrad_ws_bytes(B, h, w, Cc),
           "copy": {"median_us": copy_us, "bytes": 2 * act, "bytes_per_s": copy_rate},
           "forward": compare(lambda: ops.head_up2_fwd(x, wf, bias, y), twin_fwd, act + 16 * Pf, copy_rate, samples, warmup),
           "dgrad": compare(lambda: ops.head_up2_dgrad(gy, wf, gx), twin_dgrad, act + es * PAD * Pf, copy_rate, samples, warmup),
           "wgrad": compare(lambda: ops.head_up2_wgrad(x, gy, dw, ws), twin_wgrad, act + es * PAD * Pf, copy_rate, samples, warmup)}
    print(f"head {storage}", json.dumps(rec), flush=True)
    return rec


def whole_step(samples, warmup):
    gen = torch.Generator(); gen.manual_seed(1)
    data = (torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
            torch.rand((B, 2, H, W), generator=gen).to(DEV))
    trainers = {}
    for name, s0 in (("s0_2", 2), ("s0_1", 1)):
        eng = U.UNetEngine(H, W, B, F0=F0, k=3, depth=4, s0=s0, device=DEV, dtype="bf16", overlap_wgrad=True)
        eng.reset_parameters(torch.Generator().manual_seed(0))
        trainers[name] = U.Trainer(eng, lr=5e-7)
    runs = {k: [] for k in trainers}
    for _ in range(2):
        for name, tr in trainers.items():
            for _ in range(warmup):
                tr.step(*data)
            torch.cuda.synchronize()
            dev_ms = []
            for _ in range(samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                tr.step(*data)
                e1.record()
                torch.cuda.synchronize()
                dev_ms.append(e0.elapsed_time(e1))
            runs[name].append(statistics.median(dev_ms))
    rec = {"geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0, "kernels": 3, "depth": 4, "storage": "bf16", "overlap": True}}
    for name, tr in trainers.items():
        rec[name] = {"step_ms": runs[name], "loss": float(tr.engine.loss_out[0])}
    rec["spread"] = {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}
    rec["s0_1_over_s0_2"] = min(runs["s0_1"]) / min(runs["s0_2"])
    print("whole_step", json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "unet_s0.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    if a.samples < 50 or a.warmup < 10:
        print("note: fewer than 50 samples or 10 warm-ups - not the record's conditions", file=sys.stderr)
    res = {"samples": a.samples, "warmup": a.warmup, "reps_per_sample": REPS, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0},
           "note": "bytes = the folded algorithm's, not measured traffic; the twin materialises the up-sampled tensor (4 x the coarse one) "
                   "with torch copies, which its times include",
           "head": {st: head(st, a.samples, a.warmup) for st in ("bf16", "f32")}}
    res["whole_step"] = whole_step(a.samples, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
