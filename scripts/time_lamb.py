"""Time the LAMB step (csrc/lamb.hip; tfa.optimizers.LAMB, trainer.py:37-38) against the Adam step on the same buffers
(informational; README.md and DESIGN.md quote the record).  No threshold: the record is the deliverable.

    python scripts/time_lamb.py [--samples 50] [--warmup 10] [--out profiles/lamb.json]

Buffers: theta / grad / m / v of the default U-Net (BASELINE.json configs[1]: 256 x 256, F0 = 64, depth 4), 68.6 M elements each, 1.1 GB
together - far more than the 32 MiB of L2 and four times the 256 MiB Infinity Cache, so this is NOT a cache-warm figure (part of a buffer can still
be served from the Infinity Cache between two calls; the same holds for both variants).
Kernel level: one full-buffer `ops.lamb` (3 launches: moments + partial norms, ratios, step) against one `ops.adam` (1 launch), the two
ALTERNATING sample by sample in one process after --warmup warm-ups of each; a sample is the device time between two HIP events
around REPS back-to-back calls, divided by REPS; median, min and max over --samples samples.  `bytes` is what the algorithm has to
move (Adam: read theta, g, m, v, write theta, m, v = 7 passes of 4 n bytes; LAMB: pass 1 reads theta, g, m, v and writes m, v, pass 2
reads theta, m, v and writes theta = 10 passes, plus 16 bytes per 4096-element chunk), `copy_share` that over the time as a share of
the rate a device-to-device copy of one buffer reaches in the same process (8 n bytes over its median time) - the algorithm's bytes
over the time, not measured HBM traffic.
Whole step: `Trainer.step` at configs[1] (batch 32, bf16, side-stream schedule: the optimizer runs bucket by bucket on its own stream
while the backward pass continues) with Adam and with LAMB, two engines alternating in one process: median device time per step; what
LAMB adds to the step is what is NOT hidden behind the backward pass (`exposed_ms`), next to what it adds stand-alone."""
import argparse
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U

DEV = "cuda:0"
H = W = 256
F0, DEPTH, BATCH = 64, 4, 32
REPS = 3


def event_ms(fns, samples, warmup, reps=REPS):
    """Per function of `fns` (alternating sample by sample) the list of per-call device times in ms."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1) / reps)
    return out


def stat(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "samples": len(ms)}


def engine(dtype="bf16"):
    eng = U.UNetEngine(H, W, BATCH, F0=F0, k=3, depth=DEPTH, device=DEV, dtype=dtype, overlap_wgrad=True)
    g = torch.Generator(); g.manual_seed(0)
    eng.reset_parameters(g)
    eng.dropout_seed = 1234
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step-samples", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lamb.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lamb.py measures on the GPU; there is none here")
    ops = U.ops
    e_adam, e_lamb = engine(), engine()
    opt = U.LAMB(learning_rate=5e-7)
    t_adam = U.Trainer(e_adam, lr=5e-7)
    t_lamb = U.Trainer(e_lamb, lr=5e-7, optimizer=opt)
    n = e_adam.theta.numel()

    # ---- kernel level: the optimizer alone, on the LAMB engine's buffers with a random gradient
    eng = e_lamb
    gen = torch.Generator(); gen.manual_seed(1)
    eng.grad.copy_((torch.randn(n, generator=gen) * 1e-3).to(DEV))
    table = eng._lamb_table()
    b1, b2 = 0.9, 0.999
    lr_t = 5e-7 * math.sqrt(1 - b2 ** 10) / (1 - b1 ** 10)
    scratch = torch.empty_like(eng.theta)
    fns = {
        "adam": lambda: ops.adam(eng.theta, eng.grad, eng.adam_m, eng.adam_v, lr_t, b1, b2, 1e-7),
        "lamb": lambda: ops.lamb(table, eng.theta, eng.grad, eng.adam_m, eng.adam_v, 0, table.end, 5e-7, b1, b2, 1e-6, 0.0,
                                 1 - b1 ** 10, 1 - b2 ** 10),
        "copy": lambda: scratch.copy_(eng.theta),
    }
    ms = event_ms(fns, a.samples, a.warmup)
    copy_rate = 8.0 * n / (statistics.median(ms["copy"]) * 1e-3)
    passes = {"adam": 7, "lamb": 10}
    kern = {}
    for k in ("adam", "lamb"):
        byts = passes[k] * 4 * n + (16 * table.n_chunks + 4 * table.n_seg if k == "lamb" else 0)
        st = stat(ms[k])
        st.update(launches=1 if k == "adam" else 3, passes=passes[k], bytes=byts,
                  bytes_per_s=byts / (st["median_ms"] * 1e-3), copy_share=byts / (st["median_ms"] * 1e-3) / copy_rate)
        kern[k] = st
    kern["copy"] = dict(stat(ms["copy"]), bytes=8 * n, bytes_per_s=copy_rate)
    ratio = kern["lamb"]["median_ms"] / kern["adam"]["median_ms"]

    # ---- whole step at configs[1]: the bucket-wise optimizer stream, Adam against LAMB
    for e in (e_adam, e_lamb):
        e.reset_parameters(torch.Generator().manual_seed(0))
    g2 = torch.Generator(); g2.manual_seed(2)
    spec_in, spec_out = (torch.rand((BATCH, 2, H, W), generator=g2).to(DEV) for _ in range(2))
    emb = torch.randint(26, 1282, (BATCH, 2, 16), generator=g2).to(DEV)
    sms = event_ms({"adam": lambda: t_adam.step(spec_in, emb, spec_out), "lamb": lambda: t_lamb.step(spec_in, emb, spec_out)},
                   a.step_samples, 5, reps=1)
    step = {k: stat(v) for k, v in sms.items()}
    exposed = step["lamb"]["median_ms"] - step["adam"]["median_ms"]
    rec = {
        "what": "tfa.optimizers.LAMB (trainer.py:37-38) against Adam on the parameter buffers of BASELINE.json configs[1]",
        "device": torch.cuda.get_device_name(0), "n_elements": n, "n_variables": table.n_seg, "n_chunks": table.n_chunks,
        "buffers_bytes": 16 * n,
        "note": f"four buffers of 4 n bytes ({16 * n / 1e9:.2f} GB together): not an L2-warm figure; several times the Infinity Cache, which can "
                "still serve part of a buffer between two calls, for both variants alike.  bytes = the algorithm's, not measured traffic.",
        "kernel": kern, "lamb_over_adam": ratio, "expected_from_bytes": 10 / 7,
        "step": {"config": f"UNetEngine {H}x{W} F0={F0} depth={DEPTH} batch={BATCH} bf16, side-stream schedule, bucket-wise optimizer",
                 "adam": step["adam"], "lamb": step["lamb"], "exposed_ms": exposed,
                 "standalone_extra_ms": kern["lamb"]["median_ms"] - kern["adam"]["median_ms"],
                 "buckets": len(t_lamb.bucketer.bounds)},
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({"lamb_over_adam": ratio, "adam_ms": kern["adam"]["median_ms"], "lamb_ms": kern["lamb"]["median_ms"],
                      "copy_TBps": copy_rate / 1e12, "step_adam_ms": step["adam"]["median_ms"], "step_lamb_ms": step["lamb"]["median_ms"],
                      "exposed_ms": exposed}))


if __name__ == "__main__":
    main()
