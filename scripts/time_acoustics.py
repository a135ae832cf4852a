"""The cost of the room-acoustic figures of a test batch of 32 waveforms (T = 9600), measured two ways in one process:

  (a) the figures of (pred, true) and their per-room fold
        kernels  `ops.acoustic_figures` + `ops.acoustic_accumulate`: two launches per batch;
        torch    the same definitions as batched torch expressions in fp64 on the device (flip / cumsum for the Schroeder
                 integral, masked sums for the windows, log10 and masked sums for the regression, index_add_ for the rooms), with
                 no read-back either - what a user has to write without the kernels.  It is the yardstick of this script, not code
                 under test.
  (b) `Evaluator.update` per batch with `acoustics` off and on, behind a stub model that returns a prepared prediction (so a
      batch is reconstruction + scoring; a real network only adds the same inference time to both).

Every variant is warmed up first.  A sample is a window of `--batches` batches bracketed by device events and ended by a
synchronise; the variants of (a), then of (b), alternate sample by sample; the median and the spread of `--samples` (>= 50)
samples are reported, in microseconds per batch.  Host time is the wall time of enqueueing the window (before the synchronise)
per batch.  Launches per batch come from torch.profiler over a few batches outside the timed windows (null when this torch
build gives no device events).

    python scripts/time_acoustics.py [--samples 60] [--batches 200] [--out profiles/acoustics.json]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U

B, T, G, FS = 32, 9600, 5, 48000.0
N_PRE, N_DIR, N_EARLY = 120, 120, 2400


def make_waves(dev, seed, stretch):
    """Impulse responses: silence, a direct sound, an exponentially decaying noise tail (peak and decay vary over the batch)."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    n = torch.arange(T, device=dev, dtype=torch.float32)[None]
    peak = torch.randint(50, 3000, (B, 1), device=dev, generator=g).float()
    tau = stretch * (800.0 + 3000.0 * torch.rand((B, 1), device=dev, generator=g))
    tail = 0.3 * torch.randn((B, T), device=dev, generator=g) * torch.exp(-(n - peak) / tau)
    w = torch.where(n > peak, tail, torch.zeros_like(tail))
    w[torch.arange(B, device=dev), peak[:, 0].long()] = 1.0
    return (w * 0.05).contiguous()


def torch_figures(w):
    """fig [B, 10] of `evaluate.ACOUSTIC_FIGURES` as torch expressions, fp64 from the fp32 samples."""
    e = w.double() ** 2
    n = torch.arange(T, device=w.device)[None]
    n0 = w.abs().argmax(1, keepdim=True)
    s = (n0 - N_PRE).clamp_min(0)
    S = e.flip(1).cumsum(1).flip(1)
    after = n >= s
    e_tot = S.gather(1, s)
    e_dir = (e * (after & (n <= n0 + N_DIR))).sum(1, keepdim=True)
    e_early = (e * (after & (n < s + N_EARLY))).sum(1, keepdim=True)
    k = (n - s).double()
    m1 = (k * e * after).sum(1, keepdim=True)
    fit = after & (10.0 * S >= e_tot)
    N = fit.sum(1, keepdim=True).double()
    L = torch.where(fit, 10.0 * torch.log10(S / e_tot), torch.zeros_like(S))
    sl, skl = L.sum(1, keepdim=True), (k * L).sum(1, keepdim=True)
    sk, sk2 = N * (N - 1.0) / 2.0, (N - 1.0) * N * (2.0 * N - 1.0) / 6.0
    slope = (N * skl - sk * sl) / (N * sk2 - sk * sk) * FS
    return torch.cat([n0.double(), e_tot, e_dir, e_early, m1, N, 10.0 * torch.log10(e_dir / (e_tot - e_dir)),
                      10.0 * torch.log10(e_early / (e_tot - e_early)), m1 / e_tot / FS * 1e3, -60.0 / slope], 1)


def torch_fold(fp, ft, room, acc):
    """The errors of `evaluate.ACOUSTIC_ERRORS` folded into acc [(G + 1), 20] on the device."""
    p = torch.cat([fp[:, :1] / FS * 1e3, fp[:, 6:]], 1)
    t = torch.cat([ft[:, :1] / FS * 1e3, ft[:, 6:]], 1)
    err = (p - t).abs()
    err[:, 4] = 100.0 * err[:, 4] / t[:, 4]
    ok = torch.isfinite(p) & torch.isfinite(t)
    ok[:, 4] &= (p[:, 4] > 0) & (t[:, 4] > 0)
    zero = torch.zeros_like(p)
    cols = torch.stack([torch.where(ok, err, zero), torch.where(ok, p, zero), torch.where(ok, t, zero), ok.double()], 2).reshape(B, 20)
    acc[0] += cols.sum(0)
    acc.index_add_(0, room.long() + 1, cols)


def timed_window(step, n):
    """(device microseconds per batch, host microseconds per batch) of n batches."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(n):
        step()
    e1.record()
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n, host * 1e6 / n


def count_launches(step, n):
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                step()
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        return round(len(kernels) / n, 2) if kernels else None
    except Exception as exc:                                    # the measurement is optional; say why it is missing
        print("launch count not available:", exc, file=sys.stderr)
        return None


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "p10": float(np.percentile(v, 10)),
            "p90": float(np.percentile(v, 90)), "samples": len(v)}


def alternate(steps, samples, batches):
    """{name: {"device_us_per_batch": spread, "host_us_per_batch": spread}} with the variants alternating sample by sample."""
    for step in steps.values():
        timed_window(step, batches)
        timed_window(step, batches)
    dev_t, host_t = {k: [] for k in steps}, {k: [] for k in steps}
    for _ in range(samples):
        for k, step in steps.items():
            d, h = timed_window(step, batches)
            dev_t[k].append(d)
            host_t[k].append(h)
    return {k: {"device_us_per_batch": spread(dev_t[k]), "host_us_per_batch": spread(host_t[k])} for k in steps}


class Stub:
    def __init__(self, pred):
        self.pred = pred

    def model(self, inputs, training=False):
        return self.pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.samples < 50:
        raise SystemExit("--samples: the record wants the median of at least 50")
    if not torch.cuda.is_available():
        raise SystemExit("time_acoustics.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    wt, wp = make_waves(dev, 1234, 1.0), make_waves(dev, 1234, 1.15)
    room = torch.randint(0, G, (B,), device=dev, dtype=torch.int32)

    # ---- (a) figures + fold: kernels against torch expressions
    fig = torch.empty((B, 2, 10), dtype=torch.float64, device=dev)
    acc_k = torch.zeros((G + 1, 20), dtype=torch.float64, device=dev)
    acc_t = torch.zeros((G + 1, 20), dtype=torch.float64, device=dev)

    def step_kernels():
        U.ops.acoustic_figures(wp, wt, fig, N_PRE, N_DIR, N_EARLY, FS)
        U.ops.acoustic_accumulate(fig, room, acc_k, FS)

    def step_torch():
        torch_fold(torch_figures(wp), torch_figures(wt), room, acc_t)

    step_kernels()
    step_torch()
    torch.cuda.synchronize()
    fk, ft = fig.cpu().numpy(), torch.stack([torch_figures(wp), torch_figures(wt)], 1).cpu().numpy()
    assert np.isfinite(fk).all() and np.array_equal(fk[..., [0, 5]], ft[..., [0, 5]]), "the two paths must see the same rows"
    assert np.allclose(fk, ft, rtol=1e-8, atol=1e-8), np.abs(fk - ft).max()
    assert np.allclose(acc_k.cpu().numpy(), acc_t.cpu().numpy(), rtol=1e-8, atol=1e-8)
    part_a = alternate({"kernels": step_kernels, "torch": step_torch}, a.samples, a.batches)
    part_a["kernels"]["launches_per_batch"] = count_launches(step_kernels, 8)
    part_a["torch"]["launches_per_batch"] = count_launches(step_torch, 8)
    part_a["ratio_of_median_device_time_torch_over_kernels"] = (part_a["torch"]["device_us_per_batch"]["median"] /
                                                               part_a["kernels"]["device_us_per_batch"]["median"])

    # ---- (b) Evaluator.update with and without the figures
    pre = U.features.PreProcess()
    spec_out = pre(wt)
    pred = pre(wp).permute(0, 2, 3, 1).contiguous()
    emb = torch.zeros((B, 2, 16), dtype=torch.int32, device=dev)
    evs = {"acoustics_off": U.Evaluator(Stub(pred)), "acoustics_on": U.Evaluator(Stub(pred), acoustics=True)}
    steps = {k: (lambda ev=ev: ev.update(spec_out, emb, spec_out, wt, room)) for k, ev in evs.items()}
    part_b = alternate(steps, a.samples, a.batches)
    for k in steps:
        part_b[k]["launches_per_batch"] = count_launches(steps[k], 8)
    part_b["added_device_us_per_batch_on_minus_off"] = (part_b["acoustics_on"]["device_us_per_batch"]["median"] -
                                                        part_b["acoustics_off"]["device_us_per_batch"]["median"])
    res = evs["acoustics_on"].result()

    out = {
        "what": "room-acoustic figures of a test batch: (a) figures of (pred, true) + per-room fold, kernels against torch "
                "expressions; (b) Evaluator.update behind a stub model (reconstruction + scoring) without and with the figures",
        "shape": {"batch": B, "T": T, "n_pre": N_PRE, "n_dir": N_DIR, "n_early": N_EARLY, "fs": FS, "rooms": G},
        "device": torch.cuda.get_device_name(0),
        "method": f"a sample is a window of {a.batches} batches between device events, ended by a synchronise; variants alternate "
                  f"sample by sample in one process after a warm-up of each; {a.samples} samples per variant; microseconds per "
                  "batch; host time is the wall time of enqueueing the window",
        "figures_and_fold": part_a,
        "evaluator_update": part_b,
        "evaluator_global_errors": {k: v["err"][0] for k, v in res["acoustics"].items()},
    }
    line = json.dumps(out, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
