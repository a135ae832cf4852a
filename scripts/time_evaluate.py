"""Scoring a test batch of 32 (144 x 160 features, T = 9600 waveforms) two ways, in one process, alternating:

  new    `Evaluator.update_scored`: one scoring launch + one accumulation launch per batch, running sums on the device, one
         read-back (`result()`) at the end of the window;
  torch  the same seven figures as batched torch expressions with one read-back per figure and per-room sums on the host -
         what a user has to write without the scoring kernels.

Every shape is warmed up first; a window is as many batches as take about `--window-s` seconds (calibrated per path, at least
200), bracketed by device events, and ends in a synchronise; windows alternate new / torch; medians and spread over the
windows.  Launches per batch come from torch.profiler over a few batches outside the timed windows, host synchronisations per
batch from torch's sync debug mode; either is reported as null when this torch build cannot provide it.

    python scripts/time_evaluate.py [--windows 7] [--window-s 0.3] [--out profiles/eval_metrics_ab.json]
"""
import argparse
import json
import math
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U

B, H, W, T, N50, G = 32, 144, 160, 9600, 2400, 5


def make_batch(dev):
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    r0, c0 = math.ceil(0.896 * H), math.ceil(0.944 * W)
    pred, spec_in, target = (torch.rand((B, 2, H, W), device=dev, generator=g) for _ in range(3))
    target[:, :, r0:, :] = 0.0
    target[:, :, :, c0:] = 0.0
    wp, wt = ((torch.rand((B, T), device=dev, generator=g) - 0.5) * 2e-2 for _ in range(2))
    room = torch.randint(0, G, (B,), device=dev, generator=g, dtype=torch.int32)
    return pred, spec_in, target, wp, wt, room


class TorchScorer:
    """The figures of `evaluate.METRICS` as torch expressions over a batch, read back one figure at a time."""

    def __init__(self, room_host):
        self.room = np.asarray(room_host)
        self.sums = np.zeros((G + 1, 8))

    def update(self, pred, spec_in, target, wp, wt):
        d = target - pred
        d2 = d * d
        t0 = target[:, 0].reshape(B, -1)
        dw = wt - wp
        dw2 = dw * dw
        figs = (
            d2.reshape(B, -1).mean(1),
            d2[:, 0].reshape(B, -1).mean(1),
            (1 - torch.cos(2 * math.pi * (target[:, 1] - pred[:, 1]))).reshape(B, -1).mean(1),
            20 * torch.log10(torch.linalg.vector_norm(d[:, 0].reshape(B, -1), dim=1) / torch.linalg.vector_norm(t0, dim=1)),
            dw2.mean(1),
            dw2[:, :N50].mean(1),
            20 * torch.log10(torch.linalg.vector_norm(dw, dim=1) / torch.linalg.vector_norm(wt, dim=1)),
        )
        for k, f in enumerate(figs):
            v = f.cpu().numpy().astype(np.float64)             # one read-back per figure
            self.sums[0, k] += v.sum()
            np.add.at(self.sums[1:, k], self.room, v)
        self.sums[0, 7] += B
        np.add.at(self.sums[1:, 7], self.room, 1)

    def means(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return self.sums[:, :7] / self.sums[:, 7:8]


def run_new(batch, n):
    pred, spec_in, target, wp, wt, room = batch
    ev = U.Evaluator(None)
    for _ in range(n):
        ev.update_scored(pred, spec_in, target, wp, wt, room)
    return ev.result()


def run_torch(batch, n, room_host):
    pred, spec_in, target, wp, wt, _ = batch
    sc = TorchScorer(room_host)
    for _ in range(n):
        sc.update(pred, spec_in, target, wp, wt)
    return sc.means()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3, out


def count_launches(fn, n):
    """Device kernels per batch seen by torch.profiler over n batches (None when the profiler gives no device events)."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn(n)
            torch.cuda.synchronize()
        kernels = [e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower()]
        return round(len(kernels) / n, 2) if kernels else None
    except Exception as exc:                                    # the measurement is optional; say why it is missing
        print("launch count not available:", exc, file=sys.stderr)
        return None


def count_syncs(fn, n):
    """Host synchronisations per batch flagged by torch's sync debug mode over n batches."""
    old = torch.cuda.get_sync_debug_mode()
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            fn(n)
        return round(sum("called a synchronizing" in str(w.message).lower() for w in caught) / n, 2)
    finally:
        torch.cuda.set_sync_debug_mode(old)


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "windows": [float(x) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--window-s", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_evaluate.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    batch = make_batch(dev)
    room_host = batch[5].cpu().numpy()

    # warm-up of every shape, and the two paths must agree (torch sums in fp32: 1e-4 relative, 1e-3 dB)
    res = run_new(batch, 20)
    ref = run_torch(batch, 20, room_host)
    new = np.array([res[m] for m in U.evaluate.METRICS]).T
    for c, m in enumerate(U.evaluate.METRICS):
        tol = 1e-3 if m.startswith("mis") else 1e-4 * np.abs(ref[:, c])
        assert np.all(np.abs(new[:, c] - ref[:, c]) <= tol), (m, new[:, c], ref[:, c])
    torch.cuda.synchronize()

    per_new = timed(lambda: run_new(batch, 100))[0] / 100
    per_torch = timed(lambda: run_torch(batch, 100, room_host))[0] / 100
    n_new = min(4000, max(200, math.ceil(a.window_s / per_new)))
    n_torch = min(4000, max(200, math.ceil(a.window_s / per_torch)))
    t_new, t_torch = [], []
    for _ in range(a.windows):                                  # alternating
        t_new.append(timed(lambda: run_new(batch, n_new))[0] / n_new * 1e6)
        t_torch.append(timed(lambda: run_torch(batch, n_torch, room_host))[0] / n_torch * 1e6)

    ev = U.Evaluator(None)
    sc = TorchScorer(room_host)
    step_new = lambda n: [ev.update_scored(*batch) for _ in range(n)]
    step_torch = lambda n: [sc.update(*batch[:5]) for _ in range(n)]
    step_new(2)
    torch.cuda.synchronize()
    out = {
        "what": "scoring one test batch: seven figures per sample + per-room running sums",
        "shape": {"batch": B, "H": H, "W": W, "T": T, "n50": N50, "rooms": G},
        "device": torch.cuda.get_device_name(0),
        "method": "device events around a window of batches that ends in a synchronise (the new path's window includes its one "
                  "read-back); windows alternate new / torch in one process after a warm-up of both; microseconds per batch",
        "windows": a.windows,
        "new": {"batches_per_window": n_new, "us_per_batch": spread(t_new), "launches_per_batch": None, "host_syncs_per_batch": None},
        "torch": {"batches_per_window": n_torch, "us_per_batch": spread(t_torch), "launches_per_batch": None,
                  "host_syncs_per_batch": None},
    }
    out["ratio_of_medians_torch_over_new"] = out["torch"]["us_per_batch"]["median"] / out["new"]["us_per_batch"]["median"]

    def emit():
        line = json.dumps(out, indent=1)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return line

    emit()                                                      # the timings are on disk before the optional counts are taken
    for key, step in (("new", step_new), ("torch", step_torch)):
        out[key]["host_syncs_per_batch"] = count_syncs(step, 8)
        emit()
    for key, step in (("new", step_new), ("torch", step_torch)):
        out[key]["launches_per_batch"] = count_launches(step, 8)
        emit()
    print(emit())


if __name__ == "__main__":
    main()
