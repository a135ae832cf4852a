"""Time the two forms of the multi-resolution STFT loss against each other: ops.spectral_loss (csrc/spectralloss.hip, fp64 DFTs on the
matrix cores) and ops.spectral_loss_fft (csrc/spectralloss_fft.hip, fp32 FFTs in LDS), the same definition written as torch.stft
expressions in fp32 / complex64 kept on the device under autograd (an independent implementation, not the code under test), and the
bf16 train step of the default U-Net with a WaveLoss alone against the same step with the spectral term of each method on top
(informational; README.md and DESIGN.md quote the file this writes).

    python scripts/time_spectral_loss_fft.py [--calls 50] [--warmup 10] [--out profiles/spectral_loss_fft.json]

Workload and protocol of scripts/time_spectral_loss.py: batch 32, T = 9600, the default resolutions, floor 60 dB; all forms alternate
call by call inside one timed loop of one process; per form the median, minimum, maximum and the 10th / 90th percentile of the device
time between two HIP events, the median host time to enqueue one call and the device kernels per call torch.profiler sees.  The
yardstick is the DFT form in the same process.  After the timed loop, in a pass of its own, torch.profiler gives the mean device time
of each kernel of both forms (the profiler slows the host, not the kernels).  The two forms' results are compared with the fp64 torch
twin (sanity figures, not a parity test - that is tests/test_spectral_loss_fft_gpu.py)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U
from unet_rir_amd import features as F
from unet_rir_amd.spectralloss import RESOLUTIONS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_spectral_loss import B, DEV, FLOOR_DB, H, T, W, WEIGHT, torch_spectral, windows  # noqa: E402
from time_wave_loss import count_launches, summary  # noqa: E402


def kernel_times(fn, n):
    """{kernel name: mean device microseconds per call} over n calls seen by torch.profiler (None when it gives no device events)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower():
                out[e.name] = out.get(e.name, 0.0) + (e.device_time if hasattr(e, "device_time") else e.cuda_time) / n
        return out or None
    except Exception as exc:                                    # the measurement is optional; say why it is missing
        print("kernel times not available:", exc, file=sys.stderr)
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spectral_loss_fft.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator(); gen.manual_seed(1)
    t = torch.arange(T, dtype=torch.float32)
    wav_true = (torch.randn((B, T), generator=gen) * torch.exp(-t / 700.0)[None, :]).to(DEV)
    pred = F.PreProcess()((torch.randn((B, T), generator=gen) * torch.exp(-t / 900.0)[None, :]).to(DEV))      # a plausible prediction
    wav_pred = F.PostProcess().post_process(pred, nhwc=False).clone()
    bytes_dft, bytes_fft = U.ops.spectral_loss_ws_bytes(B, T, RESOLUTIONS), U.ops.spectral_loss_fft_ws_bytes(B, T, RESOLUTIONS)
    ws_dft, ws_fft = U.ops.Workspace(DEV, bytes_dft), U.ops.Workspace(DEV, bytes_fft)
    out_dft, out_fft = (torch.zeros(3, dtype=torch.float64, device=DEV) for _ in range(2))
    dw_dft, dw_fft = torch.empty_like(wav_pred), torch.empty_like(wav_pred)
    wav_leaf = wav_pred.clone().requires_grad_(True)
    w64, w32 = windows(torch.float64), windows(torch.float32)

    def torch_pair(wins):
        wav_leaf.grad = None
        torch_spectral(wav_leaf, wav_true, wins).backward()

    def torch_forward(wins):
        with torch.no_grad():
            return torch_spectral(wav_pred, wav_true, wins)

    dft = lambda dw: U.ops.spectral_loss(wav_pred, wav_true, out_dft, ws_dft, RESOLUTIONS, floor_db=FLOOR_DB, weight=WEIGHT, dwav=dw)
    fft = lambda dw: U.ops.spectral_loss_fft(wav_pred, wav_true, out_fft, ws_fft, RESOLUTIONS, floor_db=FLOOR_DB, weight=WEIGHT, dwav=dw)
    # the whole train step, bf16 storage, the default U-Net (bench.py's flagship geometry), in this process
    spec_in, emb, spec_out = next(iter(U.synthetic_batches(1, B, H, W, DEV)))
    steps = {}
    for name, kw in (("step_bf16_wave", {}),
                     ("step_bf16_wave_spectral_dft", dict(spectral_loss=U.SpectralLoss(weight=WEIGHT, floor_db=FLOOR_DB, method="dft"))),
                     ("step_bf16_wave_spectral_fft", dict(spectral_loss=U.SpectralLoss(weight=WEIGHT, floor_db=FLOOR_DB, method="fft")))):
        eng = U.UNetEngine(H, W, B, device=DEV, dtype="bf16")
        tr = U.Trainer(eng, wave_loss=U.WaveLoss(weight=0.5, norm="energy"), **kw)
        steps[name] = (lambda tr=tr: tr.step(spec_in, emb, spec_out, wav_true=wav_true))
    forms = {"dft_pair": lambda: dft(dw_dft), "dft_forward": lambda: dft(None), "fft_pair": lambda: fft(dw_fft),
             "fft_forward": lambda: fft(None), "torch_c64_pair": lambda: torch_pair(w32), "torch_c64_forward": lambda: torch_forward(w32),
             **steps}
    for _ in range(a.warmup):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    dev_ms, host_us = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.calls):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            fn()
            host_us[name].append((time.perf_counter() - t0) * 1e6)
            e1.record()
            torch.cuda.synchronize()
            dev_ms[name].append(e0.elapsed_time(e1))
    dft(dw_dft)
    fft(dw_fft)
    torch_pair(w64)
    g64 = wav_leaf.grad.clone()
    torch_pair(w32)
    g32 = wav_leaf.grad.clone()
    torch.cuda.synchronize()
    peak = g64.abs().max()
    res = {"workload": {"batch": B, "samples": T, "resolutions": [list(r) for r in RESOLUTIONS], "floor_db": FLOOR_DB, "weight": WEIGHT},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "workspace_bytes": {"dft": bytes_dft, "fft": bytes_fft},
           "dwav_max_abs_difference_over_peak_f64": {"dft": float((dw_dft - g64).abs().max() / peak), "fft": float((dw_fft - g64).abs().max() / peak),
                                                     "torch_c64": float((g32 - g64).abs().max() / peak)},
           "loss": {"dft": float(WEIGHT / B * (out_dft[0] + out_dft[1])), "fft": float(WEIGHT / B * (out_fft[0] + out_fft[1])),
                    "torch_f64": float(torch_forward(w64)), "torch_c64": float(torch_forward(w32))}}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        print(name, json.dumps(res[name]))
    for k in ("dft_pair", "fft_pair"):
        res[k]["launches_per_call_by_construction"] = 4
    for k in ("dft_forward", "fft_forward"):
        res[k]["launches_per_call_by_construction"] = 2
    res["kernel_us_mean"] = {"dft": kernel_times(forms["dft_pair"], 20), "fft": kernel_times(forms["fft_pair"], 20)}
    m = lambda k: res[k]["device_ms_median"]
    res["dft_pair_over_fft_pair"] = m("dft_pair") / m("fft_pair")
    res["dft_forward_over_fft_forward"] = m("dft_forward") / m("fft_forward")
    res["torch_c64_pair_over_fft_pair"] = m("torch_c64_pair") / m("fft_pair")
    res["step_added_ms"] = {"dft": m("step_bf16_wave_spectral_dft") - m("step_bf16_wave"),
                            "fft": m("step_bf16_wave_spectral_fft") - m("step_bf16_wave")}
    res["step_added_share_of_the_step"] = {k: v / m("step_bf16_wave") for k, v in res["step_added_ms"].items()}
    res["step_spread_ms_p10_p90"] = {k: [res[k]["device_ms_p10"], res[k]["device_ms_p90"]] for k in steps}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
