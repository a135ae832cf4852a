"""Time the decay loss (ops.decay_loss: csrc/decayloss.hip) and the vector-Jacobian product of PostProcess (ops.istft_features_bwd:
csrc/istft_bwd.hip), both fp64 inside, against the same two written as torch expressions kept on the device under autograd (cumsum
for the loss in fp64, torch.istft in fp32 / complex64 for the product: independent implementations, not the code under test), and
the bf16 train step of the default U-Net with a WaveLoss alone against the same step with a WaveLoss and a DecayLoss - what the
second adjoint pass costs (informational; README.md and DESIGN.md quote the file this writes).

    python scripts/time_decay_loss.py [--calls 50] [--warmup 10] [--out profiles/decay_loss.json]

Workload: batch 32, 129 x 151 bins x frames inside 144 x 160 planes (dataset.py:62-70), n_fft 256, win 128, hop 64, T = 9600, floor
60 dB.  All forms alternate call by call inside one timed loop of one process, the device-to-device copy the decay kernel's rate is
set against among them; per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP
events, the median host time to enqueue one call, and the device kernels per call torch.profiler sees.  The kernels' results are also
compared with the torch twins' (sanity figures, not a parity test - that is tests/test_decay_loss_gpu.py)."""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import unet_rir_amd as U
from unet_rir_amd import features as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from time_wave_loss import count_launches, summary  # noqa: E402

DEV = "cuda:0"
B, H, W = 32, 144, 160
NB, NF = F.STFT_SHAPE
N_FFT, WIN, HOP = F.N_FFT, F.WIN_LENGTH, F.HOP_LENGTH
T = HOP * (NF - 1)
WEIGHT, FLOOR_DB = 0.01, 60.0


def torch_decay(wav_pred, wav_true):
    """weight / B * sum_b Q_b in torch expressions, fp64"""
    p, t = wav_pred.double(), wav_true.double()
    delta = 10.0 ** (-FLOOR_DB / 10.0)
    e0 = (t * t).sum(dim=1, keepdim=True)
    curve = lambda x: 10.0 * torch.log10(torch.flip(torch.cumsum(torch.flip(x * x, dims=(1,)), dim=1), dims=(1,)) / e0 + delta)
    d = curve(p) - curve(t)
    return WEIGHT / B * (d * d).mean(dim=1).sum()


def torch_waveform(pred, window):
    amp = (10.0 ** ((pred[:, 0, :NB, :NF] * 100.0 - 100.0) / 20.0) - 1e-5) * 128.0
    ph = torch.remainder(pred[:, 1, :NB, :NF] * (2.0 * math.pi), 2.0 * math.pi) - math.pi
    return torch.istft(torch.polar(amp, ph), N_FFT, HOP, WIN, window, center=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "decay_loss.json"))
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
    window = torch.hann_window(WIN, periodic=True, device=DEV)
    ws = U.ops.Workspace(DEV, U.ops.decay_loss_ws_bytes(B, T))
    decay_out = torch.zeros(2, dtype=torch.float64, device=DEV)
    dwav, dpred, copy_dst = torch.empty_like(wav_pred), torch.empty_like(pred), torch.empty_like(wav_pred)
    wav_leaf = wav_pred.clone().requires_grad_(True)
    pred_leaf = pred.clone().requires_grad_(True)

    def torch_decay_pair():
        wav_leaf.grad = None
        torch_decay(wav_leaf, wav_true).backward()

    def torch_vjp():                                 # forward and backward: autograd has no way to the product without the forward
        pred_leaf.grad = None
        torch_waveform(pred_leaf, window).backward(dwav)

    decay = lambda dw: U.ops.decay_loss(wav_pred, wav_true, decay_out, ws, floor_db=FLOOR_DB, weight=WEIGHT, dwav=dw)
    vjp = lambda acc: U.ops.istft_features_bwd(pred, dwav, dpred, NB, NF, N_FFT, WIN, HOP, accumulate=acc)
    # the whole train step, bf16 storage, the default U-Net (bench.py's flagship geometry): the parent commit's step with a WaveLoss
    # against the same step with the decay term on top, in this process
    spec_in, emb, spec_out = next(iter(U.synthetic_batches(1, B, H, W, DEV)))
    steps = {}
    for name, dl in (("step_bf16_wave", None), ("step_bf16_wave_decay", U.DecayLoss(weight=WEIGHT, floor_db=FLOOR_DB))):
        eng = U.UNetEngine(H, W, B, device=DEV, dtype="bf16")
        tr = U.Trainer(eng, wave_loss=U.WaveLoss(weight=0.5, norm="energy"), decay_loss=dl)
        steps[name] = (lambda tr=tr: tr.step(spec_in, emb, spec_out, wav_true=wav_true))
    decay(dwav)
    forms = {"decay_pair": lambda: decay(dwav), "decay_forward": lambda: decay(None), "vjp_write": lambda: vjp(False),
             "vjp_accumulate": lambda: vjp(True), "torch_decay_pair": torch_decay_pair, "torch_vjp": torch_vjp,
             "copy_d2d": lambda: copy_dst.copy_(wav_pred), **steps}
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
    decay(dwav)
    vjp(False)
    torch_decay_pair()
    torch_vjp()
    torch.cuda.synchronize()
    res = {"workload": {"batch": B, "planes": [H, W], "n_bins": NB, "n_frames": NF, "n_fft": N_FFT, "win_length": WIN, "hop_length": HOP,
                        "samples": T, "floor_db": FLOOR_DB, "weight": WEIGHT},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "workspace_bytes": U.ops.decay_loss_ws_bytes(B, T),
           "dwav_max_abs_difference_over_peak": float((dwav - wav_leaf.grad).abs().max() / wav_leaf.grad.abs().max()),
           "vjp_max_abs_difference_over_peak": float((dpred - pred_leaf.grad).abs().max() / pred_leaf.grad.abs().max()),
           "loss_kernels": float(WEIGHT / B * decay_out[0]), "loss_torch": float(torch_decay(wav_pred, wav_true))}
    for name, fn in forms.items():
        res[name] = summary(dev_ms[name], host_us[name])
        res[name]["launches_per_call"] = count_launches(fn, 4)
        print(name, json.dumps(res[name]))
    res["decay_pair"]["launches_per_call_by_construction"] = 2
    res["decay_forward"]["launches_per_call_by_construction"] = 2
    res["vjp_write"]["launches_per_call_by_construction"] = 1
    res["vjp_accumulate"]["launches_per_call_by_construction"] = 1
    m = lambda k: res[k]["device_ms_median"]
    # the decay kernel moves two reads and one write of [B, T] fp32 where the copy moves one read and one write
    moved, copied = 3 * B * T * 4, 2 * B * T * 4
    res["copy_d2d"]["bytes"] = copied
    res["copy_d2d"]["gb_per_s"] = copied / (m("copy_d2d") * 1e-3) / 1e9
    res["decay_pair"]["bytes"] = moved
    res["decay_pair"]["gb_per_s"] = moved / (m("decay_pair") * 1e-3) / 1e9
    res["decay_pair_share_of_copy_rate"] = res["decay_pair"]["gb_per_s"] / res["copy_d2d"]["gb_per_s"]
    res["torch_decay_pair_over_decay_pair"] = m("torch_decay_pair") / m("decay_pair")
    res["torch_vjp_over_vjp_write"] = m("torch_vjp") / m("vjp_write")
    res["step_added_ms"] = m("step_bf16_wave_decay") - m("step_bf16_wave")
    res["step_spread_ms_p10_p90"] = {k: [res[k]["device_ms_p10"], res[k]["device_ms_p90"]] for k in ("step_bf16_wave", "step_bf16_wave_decay")}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
