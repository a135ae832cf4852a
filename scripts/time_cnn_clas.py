"""Time the room classifier deep_CNN (dl_models/cnn_clas.py; csrc/cnn_clas.hip) at 144 x 160 x 2, five classes, batch 32, fp32
(informational; README.md and DESIGN.md quote the record).  No threshold: the record is the deliverable.

    python scripts/time_cnn_clas.py [--samples 50] [--warmup 10] [--parts step,layers,pool] [--out profiles/cnn_clas.json]

Every comparison ALTERNATES its variants in one process, twice each (a, b, a, b): a run is the median over --samples samples, after
--warmup warm-ups, of the device time between two HIP events; `spread` is the relative distance between the two medians of one
variant.  An existing --out file is updated part by part.

  step    `Trainer.step` of DeepCNNEngine (Adam, Dropout on; also with valid_kernels_only=True) against the same model as torch expressions on the device - F.conv2d,
          F.avg_pool2d, F.batch_norm, F.cross_entropy, autograd, torch.optim.Adam, NCHW tensors: median device time per step, host
          time to enqueue a step, device kernels per step (torch.profiler).
  layers  every pass of every 'valid' convolution against the existing 'same' entry point on the same input (for the weight
          gradient: unetrir_conv2d_wgrad_f32 + unetrir_colsum_f32, which together give what the one call gives, without the ReLU
          mask): the cost of the twin before any crop - and `same_composed`, the twin with the glue that makes it the same
          function (cnn_clas.twin_forward: crop + ReLU; cnn_clas.twin_dgrad: ReLU mask + zero-ringed copy), which is what the
          engine runs where it wins (DeepCNNEngine.TWIN_*_MIN_CIN).  REPS calls per sample.
  pool    AveragePooling2D behind BatchNormalization on the first block's tensor (32 x 142 x 158 x 16, 46 MB): the forward kernel
          with the affine folded in against affine-then-pool (unetrir_bn_act_add_f32 + plain pooling); the backward composition
          the engine runs (pooling adjoint + unetrir_bn_bwd_f32) and its two parts; and a device-to-device copy of the same tensor
          in the same process.  `share_of_copy_rate` = the bytes the ALGORITHM has to move over the time, over the copy's
          bytes / time.  The buffers are reused call after call and fit the 256 MB Infinity Cache: cache-warm numbers, not HBM rates."""
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
from unet_rir_amd.cnn_clas import twin_dgrad, twin_forward

DEV = "cuda:0"
H, W, B, CLASSES = 144, 160, 32, 5
REPS = 5
LAYERS = (("Conv0_A", 144, 160, 4, 16), ("Conv1_A", 71, 79, 16, 32), ("Conv0_C", 34, 38, 32, 64))


def event_us(fn, samples, warmup, reps=REPS):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(us)


def alternate(variants, samples, warmup):
    """name -> [median us, median us] with the variants alternating, plus the spread of each."""
    runs = {k: [] for k in variants}
    for _ in range(2):
        for k, fn in variants.items():
            runs[k].append(event_us(fn, samples, warmup))
    return {"us": runs, "spread": {k: abs(v[0] - v[1]) / min(v) for k, v in runs.items()}}


def versus(rec, new, old):
    """old / new of the faster medians, and whether `new` is slower than `old` by more than the spread."""
    us, sp = rec["us"], max(rec["spread"].values())
    rec[f"{old}_over_{new}"] = min(us[old]) / min(us[new])
    rec[f"{new}_slower_beyond_spread"] = min(us[new]) > max(us[old]) * (1.0 + sp)
    return rec


def layers(samples, warmup):
    ops, out = U.ops, {}
    for name, h, w, ci, co in LAYERS:
        gen = torch.Generator(device=DEV); gen.manual_seed(h * 1000 + ci)
        rnd = lambda *sh: (torch.rand(sh, device=DEV, generator=gen) - 0.5) * 2
        g = ops.geom(B, h, w, ci, co, 3, 1)
        x, dx = ops.Act(rnd(B, h, w, ci)), ops.Act(rnd(B, h, w, ci))
        yv, dyv = ops.Act(rnd(B, h - 2, w - 2, co)), ops.Act(rnd(B, h - 2, w - 2, co))
        ys, dys = ops.Act(rnd(B, h, w, co)), ops.Act(rnd(B, h, w, co))
        wk, bias = rnd(co, 3, 3, ci) * 0.1, rnd(co)
        wt = torch.empty(ci * 9 * co, device=DEV)
        ops.transpose_weight(wk, wt, co, 9, ci)
        dw, db, ws = torch.empty_like(wk), torch.empty(co, device=DEV), ops.Workspace(DEV)
        ops.conv3x3_valid_fwd(g, x, wk, bias, yv, True)           # yv holds a ReLU output: the masks of the backward kernels are real

        def twin_wgrad():
            ops.conv2d_wgrad(g, x, dys, dw, ws)
            ops.colsum(dys, db, ws)
        yc, gm, dyz = ops.Act(rnd(B, h - 2, w - 2, co)), ops.Act(rnd(B, h - 2, w - 2, co)), ops.Act(torch.zeros((B, h, w, co), device=DEV))
        y2 = ops.Act(torch.empty_like(yv.base))
        rec = {"input": [B, h, w, ci], "output_valid": [B, h - 2, w - 2, co], "output_same": [B, h, w, co],
               "forward": versus(versus(alternate({"valid": lambda: ops.conv3x3_valid_fwd(g, x, wk, bias, y2, True),
                                                   "same": lambda: ops.conv2d_fwd(g, x, wk, bias, ys),
                                                   "same_composed": lambda: twin_forward(g, x, wk, bias, ys, yc, y2, True)}, samples, warmup),
                                        "valid", "same"), "valid", "same_composed"),
               "weight_gradient": versus(alternate({"valid": lambda: ops.conv3x3_valid_wgrad(g, x, dyv, yv, dw, db, ws, True),
                                                    "same": twin_wgrad}, samples, warmup), "valid", "same")}
        if ci != 4:                # the first layer needs no data gradient
            rec["data_gradient"] = versus(versus(alternate({"valid": lambda: ops.conv3x3_valid_dgrad(g, dyv, yv, wt, dx, True),
                                                            "same": lambda: ops.conv2d_dgrad(g, dys, wt, dx),
                                                            "same_composed": lambda: twin_dgrad(g, dyv, yv, wt, dx, gm, dyz, True)},
                                                           samples, warmup), "valid", "same"), "valid", "same_composed")
        rec["engine_runs_composed"] = {"forward": ci >= U.DeepCNNEngine.TWIN_FWD_MIN_CIN, "data_gradient": ci >= U.DeepCNNEngine.TWIN_DGRAD_MIN_CIN}
        print(name, json.dumps(rec))
        out[name] = rec
    return out


def pool(samples, warmup):
    ops = U.ops
    h, w, c = 142, 158, 16
    gen = torch.Generator(device=DEV); gen.manual_seed(7)
    rnd = lambda *sh: torch.rand(sh, device=DEV, generator=gen)
    x, t, da, dx = (ops.Act(rnd(B, h, w, c)) for _ in range(4))
    y, dy = ops.Act(rnd(B, h // 2, w // 2, c)), ops.Act(rnd(B, h // 2, w // 2, c) - 0.5)
    gamma, beta = rnd(c) + 0.5, rnd(c) - 0.5
    aff, saved, dg, db, ws = torch.empty(2 * c, device=DEV), torch.empty(2 * c, device=DEV), torch.empty(c, device=DEV), torch.empty(c, device=DEV), ops.Workspace(DEV)
    ops.bn_stats(x, gamma, beta, aff, saved, ws)
    full, quarter = x.base.numel() * 4, y.base.numel() * 4

    def unfused_fwd():
        ops.bn_act_add(x, aff, t, 0, None)
        ops.avgpool2_fwd(t, None, y)

    def shipped_bwd():
        ops.avgpool2_bwd(dy, da)
        ops.bn_bwd(da, x, None, aff, saved, dx, dg, db, ws, relu=0)
    fwd = versus(alternate({"folded": lambda: ops.avgpool2_fwd(x, aff, y), "affine_then_pool": unfused_fwd}, samples, warmup),
                 "folded", "affine_then_pool")
    bwd = alternate({"pool_adjoint_then_bn_bwd": shipped_bwd, "pool_adjoint": lambda: ops.avgpool2_bwd(dy, da),
                     "bn_bwd": lambda: ops.bn_bwd(da, x, None, aff, saved, dx, dg, db, ws, relu=0),
                     "copy": lambda: t.base.copy_(x.base)}, samples, warmup)
    copy_rate = 2 * full / (min(bwd["us"]["copy"]) * 1e-6)
    share = lambda nbytes, us: nbytes / (min(us) * 1e-6) / copy_rate
    rec = {"tensor": [B, h, w, c], "bytes": full, "cache_warm": True, "copy_bytes_per_s": copy_rate, "forward": fwd, "backward": bwd,
           "fused_backward": "not built: the engine composes the pooling adjoint with unetrir_bn_bwd_f32",
           "algorithm_bytes": {"forward_folded": full + quarter, "backward": quarter + 2 * full},
           "share_of_copy_rate": {"forward_folded": share(full + quarter, fwd["us"]["folded"]),
                                  "forward_affine_then_pool": share(full + quarter, fwd["us"]["affine_then_pool"]),
                                  "backward_shipped": share(quarter + 2 * full, bwd["us"]["pool_adjoint_then_bn_bwd"])}}
    print("pool", json.dumps(rec))
    return rec


class TorchBaseline:
    """The same model as torch expressions with autograd and torch.optim.Adam (NCHW, fp32)."""

    def __init__(self, eng):
        k = {n: v.to(DEV) for n, v in eng.export_keras_params().items()}
        p = lambda t: t.clone().requires_grad_(True)
        self.conv = [(p(k[n + ".kernel"].permute(3, 2, 0, 1).contiguous()), p(k[n + ".bias"])) for n in ("Conv0_A", "Conv1_A", "Conv0_C")]
        self.bn = [(p(k[f"bn{i}.gamma"]), p(k[f"bn{i}.beta"]), torch.zeros_like(k[f"bn{i}.gamma"]), torch.ones_like(k[f"bn{i}.gamma"])) for i in range(4)]
        self.fc = [(p(k[n + ".kernel"].t().contiguous()), p(k[n + ".bias"])) for n in ("dense", "dense_1")]
        leaves = [t for pair in self.conv + self.fc for t in pair] + [t for b in self.bn for t in b[:2]]
        self.opt = torch.optim.Adam(leaves, lr=1e-3, eps=1e-7)

    def bnorm(self, h, i):
        g, b, rm, rv = self.bn[i]
        return F.batch_norm(h, rm, rv, g, b, training=True, momentum=0.01, eps=1e-3)

    def step(self, x, y):
        h = x
        for i, (w, b) in enumerate(self.conv):
            h = self.bnorm(F.relu(F.conv2d(h, w, b)), i)
            h = F.avg_pool2d(h, 2) if i < 2 else h.mean((2, 3))
        h = self.bnorm(F.relu(F.linear(h, *self.fc[0])), 3)
        loss = F.cross_entropy(F.linear(F.dropout(h, 0.5, training=True), *self.fc[1]), y)
        self.opt.zero_grad(set_to_none=True)
        loss.backward()
        self.opt.step()
        return loss


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


def whole_step(samples, warmup):
    gen = torch.Generator(); gen.manual_seed(1)
    x = torch.rand((B, 2, H, W), generator=gen).to(DEV)
    y = torch.zeros((B, CLASSES))
    y[torch.arange(B), torch.randint(0, CLASSES, (B,), generator=gen)] = 1.0
    y = y.to(DEV)
    eng = U.DeepCNNEngine(H, W, B, classes=CLASSES, device=DEV)
    eng.reset_parameters(torch.Generator().manual_seed(0))
    eng_v = U.DeepCNNEngine(H, W, B, classes=CLASSES, device=DEV, valid_kernels_only=True)
    eng_v.reset_parameters(torch.Generator().manual_seed(0))
    tr, tr_v, base = U.Trainer(eng, lr=1e-3), U.Trainer(eng_v, lr=1e-3), TorchBaseline(eng)
    steps = {"hip": lambda: tr.step(x, None, y), "hip_valid_kernels_only": lambda: tr_v.step(x, None, y), "torch": lambda: base.step(x, y)}
    runs = {k: {"ms": [], "host_us": []} for k in steps}
    for _ in range(2):
        for name, fn in steps.items():
            for _ in range(warmup):
                fn()
            torch.cuda.synchronize()
            dev_ms, host_us = [], []
            for _ in range(samples):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                fn()
                host_us.append((time.perf_counter() - t0) * 1e6)
                e1.record()
                torch.cuda.synchronize()
                dev_ms.append(e0.elapsed_time(e1))
            runs[name]["ms"].append(statistics.median(dev_ms))
            runs[name]["host_us"].append(statistics.median(host_us))
    rec = {"geometry": {"H": H, "W": W, "depth": 2, "classes": CLASSES, "batch": B, "storage": "f32", "optimizer": "adam", "dropout": True}}
    for name, fn in steps.items():
        ms = runs[name]["ms"]
        rec[name] = {"step_ms": ms, "spread": abs(ms[0] - ms[1]) / min(ms), "host_enqueue_us": runs[name]["host_us"],
                     "launches_per_step": count_launches(fn, 4)}
    rec["hip"]["loss"] = float(eng.loss_out[0])
    rec["hip"]["composed_passes"] = {k: list(v) for k, v in eng.twin_passes.items()}
    rec["torch_over_hip"] = min(rec["torch"]["step_ms"]) / min(rec["hip"]["step_ms"])
    print("whole_step", json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--parts", default="step,layers,pool")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "cnn_clas.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    if a.samples < 50 or a.warmup < 10:
        print("note: fewer than 50 samples or 10 warm-ups - not the record's conditions", file=sys.stderr)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update({"samples": a.samples, "warmup": a.warmup, "reps_per_sample": REPS, "device": torch.cuda.get_device_name(0),
                "arch": torch.cuda.get_device_properties(0).gcnArchName,
                "geometry": {"H": H, "W": W, "depth": 2, "classes": CLASSES, "batch": B, "storage": "f32"}})
    parts = a.parts.split(",")
    if "layers" in parts:
        res["layers"] = layers(a.samples, a.warmup)
    if "pool" in parts:
        res["pool"] = pool(a.samples, a.warmup)
    if "step" in parts:
        res["whole_step"] = whole_step(a.samples, a.warmup)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
