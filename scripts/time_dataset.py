"""What a batch out of the device-resident data set costs (csrc/dataset.hip, unet_rir_amd.DataGenerator), beside the same batch
as torch expressions and beside a plain device copy of as many bytes; and the reference-geometry U-Net step fed three ways.

    python scripts/time_dataset.py [--out profiles/dataset_gather.json] [--no-step] [--no-abl]

Part 1, at 144 x 160 on a synthetic bank of N = 4096 rows (755 MB), B = 32 and B = 256, HIP events, median of 60 after 12
warm-ups, the variants interleaved in one loop in rotating order and every iteration on another set of random rows (so the bank is read from HBM,
as a training step reads it):
    gather        ops.gather_batch: one launch, non-temporal loads
    gather_plain  the same kernel with default-policy loads (the ablation build; skipped with --no-abl), called through ctypes
                  without the wrapper's argument checks - scripts/time_gather_policy.py is the like-for-like A/B of the two policies
    torch         two index_select on the bank, two on the information vectors, one stack
    copy          Tensor.copy_ of 2 B contiguous bank rows: the yardstick
Launch counts come from torch.profiler.
Part 2: ms per step of the U-Net at the reference geometry (144 x 160, batch 32, F0 = 32, bf16, side-stream schedule) fed (a) by
DeviceBatchPipeline from host arrays, (b) by DataGenerator, (c) with one resident batch; (b) and (c) alternate twice.
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import unet_rir_amd as U
from unet_rir_amd import ops

DEV = torch.device("cuda:0")
H, W, N = 144, 160, 4096
WARM, ITERS, SETS = 12, 60, 24


def abl_gather():
    """unetrir_gather_batch_f32 of the ablation build with its loads switched to the default policy; None when not asked for."""
    if "--no-abl" in sys.argv:
        return None
    lib = U.build.ABL_LIB
    src = [os.path.join(U.build.CSRC, f) for f in os.listdir(U.build.CSRC)]
    if not os.path.exists(lib) or any(os.path.getmtime(s) > os.path.getmtime(lib) for s in src):
        U.build.build_ablations()
    L = C.CDLL(lib)
    L.unetrir_abl_set(16384)
    return U._lib.bind(L, "unetrir_gather_batch_f32")


def count_launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn(); torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
        return {"kernels": len([n for n in names if "emcpy" not in n and "emset" not in n]), "names": sorted(set(names))}
    except Exception as e:          # a profiler that does not start is reported, not hidden
        return {"kernels": None, "error": repr(e)}


def part1(B, plain):
    g = torch.Generator(device=DEV).manual_seed(B)
    bank = torch.rand((N, 2, H, W), device=DEV, generator=g)
    emb_bank = torch.randint(26, 1282, (N, 16), device=DEV, generator=g, dtype=torch.int32)
    idx = torch.randint(0, N, (SETS, 2, B), device=DEV, generator=g, dtype=torch.int32)
    assert int(idx.min()) >= 0 and int(idx.max()) < N
    spec_in, spec_out = (torch.empty((B, 2, H, W), device=DEV) for _ in range(2))
    emb = torch.empty((B, 2, 16), dtype=torch.int32, device=DEV)
    flat = torch.empty((2 * B, 2, H, W), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {}

    def gather(k):
        ops.gather_batch(bank, emb_bank, idx[k, 0], idx[k, 1], spec_in, spec_out, emb)

    def gather_plain(k):
        err = plain(p(bank), N, 2 * H * W, p(emb_bank), 16, None, 0, None, p(idx[k, 0]), p(idx[k, 1]), B, p(spec_in), p(spec_out), p(emb),
                    None, None, stream())
        assert err == 0

    def torch_expr(k):
        a = bank.index_select(0, idx[k, 0])
        b = bank.index_select(0, idx[k, 1])
        e = torch.stack((emb_bank.index_select(0, idx[k, 0]), emb_bank.index_select(0, idx[k, 1])), dim=1)
        out["torch"] = (a, e, b)

    def copy(k):
        r0 = (k * 2 * B) % (N - 2 * B)
        flat.copy_(bank[r0:r0 + 2 * B])

    variants = {"gather": gather, "torch": torch_expr, "copy": copy}
    if plain is not None:
        variants["gather_plain"] = gather_plain
    # the gather computes what the torch expressions compute
    gather(3); torch_expr(3); torch.cuda.synchronize()
    assert torch.equal(spec_in, out["torch"][0]) and torch.equal(emb, out["torch"][1]) and torch.equal(spec_out, out["torch"][2])
    if plain is not None:
        spec_in.zero_(); gather_plain(3); torch.cuda.synchronize()
        assert torch.equal(spec_in, out["torch"][0])
    times = {n: [] for n in variants}
    evs = []
    for it in range(WARM + ITERS):
        k = it % SETS
        order = list(variants.items())
        order = order[it % len(order):] + order[:it % len(order)]          # rotated: no variant always runs behind the same other one
        for n, fn in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(k); e1.record()
            if it >= WARM:
                evs.append((n, e0, e1))
    torch.cuda.synchronize()
    for n, e0, e1 in evs:
        times[n].append(e0.elapsed_time(e1))
    nbytes = 2 * B * 2 * H * W * 4
    res = {"B": B, "bytes_moved_each_way": nbytes}
    for n, v in times.items():
        med = statistics.median(v)
        res[n] = {"median_ms": round(med, 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5), "n": len(v),
                  "read_plus_write_GBps": round(2 * nbytes / med / 1e6, 1)}
    res["gather"]["launches"] = count_launches(lambda: gather(5))
    res["torch"]["launches"] = count_launches(lambda: torch_expr(5))
    res["copy"]["launches"] = count_launches(lambda: copy(5))
    return res


class SyntheticSet:
    """What DataGenerator needs of a Dataset, over random banks: 2048 rows, every row its own pair."""

    def __init__(self, n):
        g = torch.Generator(device=DEV).manual_seed(7)
        self.device, self.seed = DEV, 500
        self.bank = torch.rand((n, 2, H, W), device=DEV, generator=g)
        self.emb_bank = torch.randint(26, 1282, (n, 16), device=DEV, generator=g, dtype=torch.int32)
        self.room_bank = self.wav_bank = None
        self.index_in = list(range(n))
        self.index_out = list(range(n))
        np.random.RandomState(1).shuffle(self.index_out)

    def __len__(self):
        return self.bank.shape[0]

    def return_characteristics(self):
        return None


def part2():
    B, F0, steps, warm = 32, 32, 60, 12
    eng = U.UNetEngine(H, W, B, F0=F0, k=3, device=DEV, dtype="bf16", overlap_wgrad=True)
    g = torch.Generator(); g.manual_seed(0)
    eng.reset_parameters(g)
    tr = U.Trainer(eng, lr=5e-7)
    gen = U.DataGenerator(SyntheticSet(2048), batch_size=B, partition="train")
    assert len(gen) >= 40
    rng = np.random.default_rng(0)
    host = [(rng.random((B, H, W, 2), dtype=np.float32), rng.integers(26, 1282, (B, 2, 16)).astype(np.int32),
             rng.random((B, H, W, 2), dtype=np.float32)) for _ in range(3)]

    def timed(batches):
        t0 = None
        n = 0
        for i, (a, e, b) in enumerate(batches):
            if i == warm:
                torch.cuda.synchronize(); t0 = time.perf_counter()
            tr.step(a, e, b)
            n = i + 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / (n - warm) * 1e3

    def from_generator():
        for i in range(steps + warm):
            yield gen[i % len(gen)]

    def resident():
        batch = tuple(t.clone() for t in gen[0])
        for _ in range(steps + warm):
            yield batch

    def from_host():
        return U.DeviceBatchPipeline((host[i % 3] for i in range(steps + warm)), DEV, nhwc=True)

    res = {"geometry": f"{H}x{W} B={B} F0={F0} bf16 side-stream schedule, {steps} steps after {warm}", "pipeline_ms": [], "generator_ms": [],
           "resident_ms": []}
    for _ in range(2):
        res["generator_ms"].append(round(timed(from_generator()), 4))
        res["resident_ms"].append(round(timed(resident()), 4))
        res["pipeline_ms"].append(round(timed(from_host()), 4))
    return res


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    plain = abl_gather()
    rec = {"what": "scripts/time_dataset.py", "device": torch.cuda.get_device_name(0), "bank": f"N={N} rows of 2x{H}x{W} fp32",
           "notes": ["times are HIP events around one variant on an otherwise idle stream: a variant of several launches includes the "
                     "host's enqueue gaps between them",
                     "launches.kernels counts profiler device events whose name holds neither 'emcpy' nor 'emset': the copy variant is "
                     "a device-to-device memcpy when the runtime serves it so, and then counts 0 kernels",
                     "step.pipeline_ms: the DeviceBatchPipeline (producer thread, pinned staging) is started inside the timed "
                     "generator; only the first 12 steps are excluded, as for the other two feeds"],
           "gather": [part1(B, plain) for B in (32, 256)]}
    torch.cuda.empty_cache()
    if "--no-step" not in sys.argv:
        rec["step"] = part2()
    text = json.dumps(rec, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
