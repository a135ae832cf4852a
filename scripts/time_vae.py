"""Time the VAE train step against the Autoencoder's at the same geometry, in one process (informational; DESIGN.md quotes it).

    python scripts/time_vae.py [--steps 50] [--warmup 10] [--out profiles/vae_step.json]

Both models in the main_training.py configuration (filters 64..512, kernels 3, strides 2, latent 64, n_neurons 2048) at 144 x 160,
batch 32, fp32 and bf16 storage, `Trainer.step` with the engine's own dropout masks (and, VAE, its own eps).  Per model and storage
type: the median over --steps steps (after --warmup) of the step time between two HIP events, the median host time to enqueue a
step, and the device kernels per step torch.profiler sees.  The VAE - Autoencoder difference is what the second Dense head, the
normal draw, the fused sampling + KL kernels and the loss addition cost (the VAE also has one Dropout fewer and no l2 terms).
"""
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
H, W, B = 144, 160, 32
CFG = dict(conv_filters=(64, 128, 256, 512), conv_kernels=(3, 3, 3, 3), conv_strides=(2, 2, 2, 2), latent_space_dim=64, n_neurons=2048)


def count_launches(fn, n):
    """Device kernels per step seen by torch.profiler over n steps (None when the profiler gives no device events)."""
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


def measure(cls, dtype, steps, warmup, data):
    eng = cls(H, W, B, device=DEV, dtype=dtype, **CFG)
    g = torch.Generator(); g.manual_seed(0)
    eng.reset_parameters(g)
    tr = U.Trainer(eng, lr=5e-7)
    step = lambda: tr.step(*data)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    dev_ms, host_us = [], []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        step()
        host_us.append((time.perf_counter() - t0) * 1e6)
        e1.record()
        torch.cuda.synchronize()
        dev_ms.append(e0.elapsed_time(e1))
    out = {"step_ms_median": statistics.median(dev_ms), "step_ms_min": min(dev_ms), "step_ms_max": max(dev_ms),
           "host_enqueue_us_median": statistics.median(host_us), "launches_per_step": count_launches(step, 4),
           "params": eng.n_params(), "loss": float(eng.loss_out[0])}
    if hasattr(eng, "kl_out"):
        out["kl"] = float(eng.kl_out[0])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vae_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    data = (torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
            torch.rand((B, 2, H, W), generator=gen).to(DEV))
    res = {"geometry": {"H": H, "W": W, "batch": B, **{k: list(v) if isinstance(v, tuple) else v for k, v in CFG.items()}},
           "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for dtype in ("f32", "bf16"):
        ae = measure(U.AutoencoderEngine, dtype, a.steps, a.warmup, data)
        vae = measure(U.VAEEngine, dtype, a.steps, a.warmup, data)
        res[dtype] = {"autoencoder": ae, "vae": vae, "vae_minus_autoencoder_ms": vae["step_ms_median"] - ae["step_ms_median"]}
        print(dtype, json.dumps(res[dtype]))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
