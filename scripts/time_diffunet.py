"""Time the 1x1 two-channel head kernels (csrc/head1x1.hip) against the generic path on the same buffers, and the whole step of the
default DiffUNet with either head (informational; README.md and DESIGN.md quote the record).  The record decides what
unetrir_head1x1_supported offers: a pass stays in the mask only if its `not_slower` is true at the default head (C = 32).

    python scripts/time_diffunet.py [--samples 50] [--warmup 10] [--out profiles/diffunet.json]

Head: Conv2D(2, (1, 1)) of the default DiffUNet (dl_models/diff_u_net.py:247 with number_filters_0 = 32) at 144 x 160, batch 32, bf16
storage, and once more with C = 64.  Forward: head1x1_fwd against the tap-table forward with the 2 output channels padded to 8.
Backward: head1x1_bwd (one sweep + the slab sum) against tap-table data gradient + weight gradient + colsum.
Per pass the two variants ALTERNATE in one process, twice each (new, generic, new, generic): every run is the median over --samples
samples, after --warmup warm-ups, of the device time between two HIP events around REPS back-to-back calls, divided by REPS.  `spread`
is the relative distance between the two medians of the same variant, `not_slower` says whether the new kernel's slower median is
within the generic path's faster median times (1 + the larger spread).  `bytes` is what the algorithm has to move (forward: the
activations once, the fp32 logits once; backward: the activations, the bf16 logit gradients and the data gradient once) and
`copy_share` that over the time as a share of the rate a device-to-device copy of the activation tensor reaches in the same process
(2 x its bytes over the copy's median time) - the algorithm's bytes over the time, NOT achieved HBM traffic: the same 47-94 MB buffers
are used call after call and fit the Infinity Cache, for both variants and for the copy alike.
Whole step: `Trainer.step` (diff_loss=True) of the default DiffUNetEngine (144 x 160, batch 32, bf16) with the head on the passes the
predicate offers and with generic_head=True, the two engines alternating in one process: median device time per step."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U

DEV = "cuda:0"
H, W, B, F0 = 144, 160, 32, 32
REPS = 5
PAD = 8


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
    runs = {"head1x1": [], "generic": []}
    for _ in range(2):
        runs["head1x1"].append(event_us(new, samples, warmup))
        runs["generic"].append(event_us(old, samples, warmup))
    spread = {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}
    return {"head1x1_us": runs["head1x1"], "generic_us": runs["generic"], "spread": spread, "bytes": nbytes,
            "bytes_per_s": {k: nbytes / (min(v) * 1e-6) for k, v in runs.items()},
            "copy_share": {k: nbytes / (min(v) * 1e-6) / copy_rate for k, v in runs.items()},
            "generic_over_head1x1": min(runs["generic"]) / min(runs["head1x1"]),
            "not_slower": max(runs["head1x1"]) <= min(runs["generic"]) * (1.0 + max(spread.values()))}


def head(Cc, samples, warmup):
    ops = U.ops
    gen = torch.Generator(device=DEV); gen.manual_seed(Cc)
    rnd = lambda *sh: ((torch.rand(sh, device=DEV, generator=gen) - 0.5) * 2).to(torch.bfloat16)
    P = B * H * W
    g = ops.geom(B, H, W, Cc, PAD, 1, 1)
    x, gx = ops.Act(rnd(B, H, W, Cc)), ops.Act(rnd(B, H, W, Cc))
    y32, y16 = ops.new_act(B, H, W, 4, DEV), ops.new_act(B, H, W, PAD, DEV, dtype=torch.bfloat16)
    gy = ops.Act(rnd(B, H, W, PAD))
    gy.base[..., 2:] = 0
    w32 = torch.zeros((PAD, 1, 1, Cc), device=DEV)
    w32[:2] = (torch.rand((2, 1, 1, Cc), device=DEV, generator=gen) - 0.5) * 0.2
    same, swapped = torch.empty((PAD, 1, Cc), dtype=torch.bfloat16, device=DEV), torch.zeros((Cc, 1, PAD), dtype=torch.bfloat16, device=DEV)
    ops.cast_weight_bf16(w32, same, PAD, 1, Cc, Cc)
    ops.transpose_cast_weight_bf16(w32, swapped, PAD, 1, Cc, PAD)
    bias = torch.zeros(PAD, device=DEV)
    dw, db, ws = torch.zeros_like(w32), torch.zeros(PAD, device=DEV), ops.Workspace(DEV)
    scratch = torch.empty_like(x.base)
    copy_us = event_us(lambda: scratch.copy_(x.base), samples, warmup)
    copy_rate = 2.0 * 2 * P * Cc / (copy_us * 1e-6)

    def generic_bwd():
        ops.conv2d_dgrad(g, gy, swapped, gx)
        ops.conv2d_wgrad(g, x, gy, dw, ws, w=w32)
        ops.colsum(gy, db, ws)
    act = 2 * P * Cc
    rec = {"input": [B, H, W, Cc], "offered": ops.head1x1_supported(Cc), "workspace_bytes": ops.head1x1_bwd_ws_bytes(B, H, W, Cc),
           "copy": {"median_us": copy_us, "bytes": 2 * act, "bytes_per_s": copy_rate},
           "forward": compare(lambda: ops.head1x1_fwd(x, w32, bias, y32), lambda: ops.conv2d_fwd(g, x, same, bias, y16),
                              act + 16 * P, copy_rate, samples, warmup),
           "backward": compare(lambda: ops.head1x1_bwd(x, gy, w32, gx, dw, db, ws), generic_bwd, 2 * act + 2 * PAD * P, copy_rate, samples, warmup)}
    print(f"head C={Cc}", json.dumps(rec))
    return rec


def whole_step(samples, warmup):
    gen = torch.Generator(); gen.manual_seed(1)
    data = (torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
            torch.rand((B, 2, H, W), generator=gen).to(DEV))
    trainers = {}
    for name, generic in (("head1x1", False), ("generic", True)):
        eng = U.DiffUNetEngine(H, W, B, F0=F0, device=DEV, dtype="bf16", generic_head=generic)
        eng.reset_parameters(torch.Generator().manual_seed(0))
        trainers[name] = U.Trainer(eng, lr=5e-7, diff_loss=True)
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
    rec = {"geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0, "storage": "bf16", "diff_loss": True}}
    for name, tr in trainers.items():
        rec[name] = {"step_ms": runs[name], "head_passes": tr.engine.head_passes, "loss": float(tr.engine.loss_out[0])}
    rec["spread"] = {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}
    rec["generic_over_head1x1"] = min(runs["generic"]) / min(runs["head1x1"])
    print("whole_step", json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "diffunet.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    if a.samples < 50 or a.warmup < 10:
        print("note: fewer than 50 samples or 10 warm-ups - not the record's conditions", file=sys.stderr)
    res = {"samples": a.samples, "warmup": a.warmup, "reps_per_sample": REPS, "device": torch.cuda.get_device_name(0),
           "arch": torch.cuda.get_device_properties(0).gcnArchName,
           "geometry": {"H": H, "W": W, "batch": B, "number_filters_0": F0, "storage": "bf16"},
           "note": "bytes = the algorithm's, not measured traffic; the buffers (47 MB at C = 32) fit the Infinity Cache, for every variant and "
                   "for the copy alike",
           "head": {f"C{c}": head(c, a.samples, a.warmup) for c in (32, 64)}}
    res["whole_step"] = whole_step(a.samples, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
