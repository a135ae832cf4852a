"""Time the vector-quantiser layer (csrc/vq.hip) against the same layer written as fp32 torch expressions, and the whole VQ-VAE
train step, in one process (informational; DESIGN.md quotes the record).  No threshold: the record is the deliverable.

    python scripts/time_vqvae.py [--samples 50] [--warmup 10] [--out profiles/vqvae.json]

Layer, forward + backward, at two sizes: the reference's own (dl_models/vqvae.py:522-531 at batch 32: 32 x 10 x 9 pixels of 256
channels = 46 080 vectors of D = 16, K = 256) and K = 512, D = 64 (the same pixels with 512 channels: 23 040 vectors).
  kernels  ops.vq_fwd + ops.vq_bwd: 1 + 2 launches
  torch    VectorQuantizer.call + get_code_indices (:61-98) literally - one_hot, two matmuls, `detach` for stop_gradient - and
           autograd of <dy, y> + the add_loss term for the gradients of x and of the codebook
Per variant: device kernels per forward + backward as torch.profiler sees them, and the device time between two HIP events around
REPS back-to-back forward + backward passes, divided by REPS - the median over --samples samples after --warmup warm-ups.
Whole step: `Trainer.step` of VQVAEEngine at the reference's size (160 x 144, batch 32), fp32 and bf16 storage, with the engine's
own dropout masks: median step time between two HIP events, host time to enqueue a step, device kernels per step.
"""
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
H, W, B = 160, 144, 32
BETA = 0.25
REPS = 10
SIZES = {"reference_K256_D16": dict(rows=B * 10 * 9, C=256, D=16, K=256), "K512_D64": dict(rows=B * 10 * 9, C=512, D=64, K=512)}


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


def event_us(fn, samples, warmup, reps):
    """Median / min / max over `samples` of the device time of `reps` back-to-back calls, per call, in microseconds."""
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
    return {"us_median": statistics.median(us), "us_min": min(us), "us_max": max(us)}


def torch_layer(x, E, dy):
    """dl_models/vqvae.py:61-98 as written, fp32; returns (y, term, dx, dE)."""
    x = x.detach().requires_grad_(True)
    E = E.detach().requires_grad_(True)
    flattened = x.reshape(-1, E.shape[0])
    similarity = flattened @ E
    distances = (flattened ** 2).sum(dim=1, keepdim=True) + (E ** 2).sum(dim=0) - 2 * similarity
    encoding_indices = torch.argmin(distances, dim=1)
    encodings = F.one_hot(encoding_indices, E.shape[1]).to(x.dtype)
    quantized = (encodings @ E.t()).reshape(x.shape)
    commitment_loss = ((quantized.detach() - x) ** 2).mean()
    codebook_loss = ((quantized - x.detach()) ** 2).mean()
    term = BETA * commitment_loss + codebook_loss
    y = x + (quantized - x).detach()
    dx, dE = torch.autograd.grad((y * dy).sum() + term, (x, E))
    return y, term, dx, dE


def layer(name, rows, C, D, K, samples, warmup):
    ops = U.ops
    g = torch.Generator(); g.manual_seed(rows + K)
    x = (torch.rand((1, 1, rows, C), generator=g) * 0.4 - 0.2).to(DEV)
    E = (torch.rand((D, K), generator=g) * 0.1 - 0.05).to(DEV)
    dy = (torch.randn((1, 1, rows, C), generator=g) * 0.1).to(DEV)
    a_x, a_dy = ops.Act(x), ops.Act(dy)
    a_y, a_dx = ops.Act(torch.empty_like(x)), ops.Act(torch.empty_like(x))
    idx = torch.zeros(rows * C // D, dtype=torch.int32, device=DEV)
    out, dE, ws = torch.zeros(4, device=DEV), torch.empty_like(E), ops.vq_workspace(DEV)

    def hip():
        ops.vq_fwd(a_x, D, E, BETA, 1.0, idx, a_y, out, ws)
        ops.vq_bwd(a_x, D, idx, E, a_dy, BETA, 1.0, a_dx, dE)

    def hip_fwd():
        ops.vq_fwd(a_x, D, E, BETA, 1.0, idx, a_y, out, ws)

    def ref():
        return torch_layer(x, E, dy)

    hip()
    y_t, term_t, dx_t, dE_t = ref()
    torch.cuda.synchronize()
    agree = {"indices_equal_share": float((torch.argmin(((x.reshape(-1, D) ** 2).sum(1, keepdim=True) + (E ** 2).sum(0)
                                                          - 2 * x.reshape(-1, D) @ E), dim=1).int() == idx).float().mean()),
             "term_kernels": float(out[0]), "term_torch": float(term_t),
             "max_abs_dx_difference": float((a_dx.base - dx_t).abs().max()), "max_abs_dE_difference": float((dE - dE_t).abs().max())}
    rec = {"vectors": rows * C // D, "K": K, "D": D, "codebook_bytes_in_lds": K * (D + 1) * 4 + 2048,
           "kernels": {"launches": count_launches(hip, 4), **event_us(hip, samples, warmup, REPS)},
           "kernels_forward_only": event_us(hip_fwd, samples, warmup, REPS),
           "torch_expressions": {"launches": count_launches(ref, 4), **event_us(ref, samples, warmup, REPS),
                                 "one_hot_and_distance_bytes": 2 * (rows * C // D) * K * 4},
           "agreement": agree}
    rec["torch_over_kernels"] = rec["torch_expressions"]["us_median"] / rec["kernels"]["us_median"]
    print(name, json.dumps(rec))
    return rec


def whole_step(dtype, samples, warmup, data):
    eng = U.VQVAEEngine(H, W, B, device=DEV, dtype=dtype)
    g = torch.Generator(); g.manual_seed(0)
    eng.reset_parameters(g)
    tr = U.Trainer(eng, lr=5e-7)
    step = lambda: tr.step(*data)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    dev_ms, host_us = [], []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        step()
        host_us.append((time.perf_counter() - t0) * 1e6)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    return {"step_ms_median": statistics.median(dev_ms), "step_ms_min": min(dev_ms), "step_ms_max": max(dev_ms),
            "host_enqueue_us_median": statistics.median(host_us), "launches_per_step": count_launches(step, 4),
            "params": eng.n_params(), "loss": float(eng.loss_out[0]), "vq_term": float(eng.vq_out[0]),
            "codes_used": int(torch.unique(eng.vq_indices).numel())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vqvae.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    if a.samples < 50 or a.warmup < 10:
        print("note: fewer than 50 samples or 10 warm-ups - not the record's conditions", file=sys.stderr)
    res = {"samples": a.samples, "warmup": a.warmup, "reps_per_sample": REPS, "device": torch.cuda.get_device_name(0),
           "layer_forward_backward": {n: layer(n, samples=a.samples, warmup=a.warmup, **kw) for n, kw in SIZES.items()}}
    gen = torch.Generator(); gen.manual_seed(1)
    data = (torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
            torch.rand((B, 2, H, W), generator=gen).to(DEV))
    res["whole_step"] = {"geometry": {"H": H, "W": W, "batch": B, "model": "VQVAEEngine.DEFAULTS"}}
    for dtype in ("f32", "bf16"):
        res["whole_step"][dtype] = whole_step(dtype, a.samples, a.warmup, data)
        print(dtype, json.dumps(res["whole_step"][dtype]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
