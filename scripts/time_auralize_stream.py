"""Time `AuralizeStream` (csrc/auralize_fft.hip: the FFT form block by block) against what a user could do without it (README.md and
DESIGN.md quote the file this writes).

    python scripts/time_auralize_stream.py [--calls 50] [--warmup 10] [--out profiles/auralize_stream.json]

Workload: responses of K = 9600 taps (the reference's 0.2 s at 48 kHz) for B = 1, 8 and 32 rows, pushes of 1, 4 and 8 blocks of 2048
samples, the dry signal shared by the rows or one per row.  The forms alternate call by call inside one timed loop:

    push         ops.auralize_stream_push_f32(state, dry, out): the three launches, a caller's buffers, max_blocks = 8
    push_graph   the same push captured once in a HIP graph and replayed
    push_fade    the same push with an update pending (ops.auralize_stream_update before the timed region): its first block is rendered
                 through two responses and blended
    before       what could be done before: y = auralize(rir, chunk, method="fft", length="full"), the K - 1 samples carried from
                 the chunks before added to its head, its own tail carried on (two torch kernels around the two launches)
    floor        the one-shot auralize(rir, x, method="fft", length="same") over 256 blocks; reported per push (time x blocks / 256)

per form: the median, minimum, maximum and the 10th / 90th percentile of the device time between two HIP events, the median host time
to enqueue one call, and the device kernels per call torch.profiler sees.  `before_over_push` and `push_over_floor` are ratios of the
medians; `push_beats_before_beyond_spread` says whether push's 90th percentile is below before's 10th.  `real_time_factor` is the audio
a push renders (blocks x 2048 / 48 kHz) over the device time of a push; `sustained_real_time_factor` the same over wall-clock time per push
in a run of 200 pushes enqueued back to back with one synchronisation at the end."""
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
K, P, MAXB, SR = 9600, 2048, 8, 48000
BS = (1, 8, 32)
BLOCKS = (1, 4, 8)
FLOOR_BLOCKS = 256


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


def summary(dev_ms, host_us):
    q = statistics.quantiles(dev_ms, n=10)
    return {"calls": len(dev_ms), "device_ms_median": statistics.median(dev_ms), "device_ms_min": min(dev_ms), "device_ms_max": max(dev_ms),
            "device_ms_p10": q[0], "device_ms_p90": q[-1], "host_enqueue_us_median": statistics.median(host_us)}


def timed(pre, fn):
    if pre is not None:
        pre()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e6
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), host


def alternate(forms, a):
    """forms: {name: (pre or None, fn)}; every form called in turn: a.warmup rounds untimed, then a.calls timed rounds -> {name: summary}"""
    for _ in range(a.warmup):
        for pre, fn in forms.values():
            if pre is not None:
                pre()
            fn()
    torch.cuda.synchronize()
    dev_ms, host_us = {k: [] for k in forms}, {k: [] for k in forms}
    for _ in range(a.calls):
        for name, (pre, fn) in forms.items():
            ms, host = timed(pre, fn)
            dev_ms[name].append(ms)
            host_us[name].append(host)
    return {name: summary(dev_ms[name], host_us[name]) for name in forms}


def measure(B, blocks, rows, a, gen):
    n = blocks * P
    xr = B if rows else 1
    t = torch.arange(K, dtype=torch.float32)
    h = (torch.randn((B, K), generator=gen) * torch.exp(-t / 1500.0)[None, :]).to(DEV)         # decaying noise: plausible responses
    h1 = (torch.randn((B, K), generator=gen) * torch.exp(-t / 1500.0)[None, :]).to(DEV)
    x = torch.randn((xr, n) if rows else (n,), generator=gen).mul_(0.1).to(DEV)
    xl = torch.randn((xr, FLOOR_BLOCKS * P) if rows else (FLOOR_BLOCKS * P,), generator=gen).mul_(0.1).to(DEV)
    outs = {k: torch.empty((B, n), dtype=torch.float32, device=DEV) for k in ("push", "graph", "fade")}
    states = {k: U.ops.AuralizeStreamState(h.device, B, K, xr, MAXB) for k in outs}
    for st in states.values():
        U.ops.auralize_stream_init(st, h)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        U.ops.auralize_stream_push_f32(states["graph"], x, outs["graph"])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            U.ops.auralize_stream_push_f32(states["graph"], x, outs["graph"])
    torch.cuda.current_stream().wait_stream(side)
    carry = torch.zeros((B, K - 1), dtype=torch.float32, device=DEV)

    def before():
        y = U.auralize(h, x, method="fft")
        y[:, :K - 1] += carry
        carry.copy_(y[:, n:])
        return y[:, :n]

    out_floor = torch.empty((B, FLOOR_BLOCKS * P), dtype=torch.float32, device=DEV)
    flip = [h1, h]

    def pend():
        flip.reverse()
        U.ops.auralize_stream_update(states["fade"], flip[0])

    forms = {"push": (None, lambda: U.ops.auralize_stream_push_f32(states["push"], x, outs["push"])),
             "push_graph": (None, graph.replay),
             "push_fade": (pend, lambda: U.ops.auralize_stream_push_f32(states["fade"], x, outs["fade"])),
             "before": (None, before),
             "floor": (None, lambda: U.auralize(h, xl, length="same", out=out_floor, method="fft"))}
    r = alternate(forms, a)
    for name, (pre, fn) in forms.items():
        r[name]["launches_per_call"] = count_launches(fn, 4)
    r["push"]["launches_per_call_by_construction"] = r["push_fade"]["launches_per_call_by_construction"] = 3
    r["push"]["state_bytes"] = states["push"].need
    m = lambda k: r[k]["device_ms_median"]
    r["floor_ms_per_push"] = m("floor") * blocks / FLOOR_BLOCKS
    r["before_over_push"] = m("before") / m("push")
    r["before_over_push_graph"] = m("before") / m("push_graph")
    r["push_over_floor"] = m("push") / r["floor_ms_per_push"]
    r["fade_over_push"] = m("push_fade") / m("push")
    r["push_beats_before_beyond_spread"] = bool(r["push"]["device_ms_p90"] < r["before"]["device_ms_p10"])
    audio_ms = 1e3 * n / SR
    r["audio_ms_per_push"] = audio_ms
    r["real_time_factor"] = audio_ms / m("push")
    r["real_time_factor_graph"] = audio_ms / m("push_graph")
    runs = 200
    for name in ("push", "push_graph"):
        fn = forms[name][1]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(runs):
            fn()
        torch.cuda.synchronize()
        r["sustained_real_time_factor" + name[4:]] = audio_ms / ((time.perf_counter() - t0) * 1e3 / runs)
    for name in list(forms) + ["floor_ms_per_push", "before_over_push", "before_over_push_graph", "push_over_floor", "fade_over_push",
                               "push_beats_before_beyond_spread", "real_time_factor", "real_time_factor_graph",
                               "sustained_real_time_factor", "sustained_real_time_factor_graph"]:
        print(B, blocks, "rows" if rows else "shared", name, json.dumps(r[name]), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "auralize_stream.json"))
    a = ap.parse_args()
    if a.calls < 50 or a.warmup < 10:
        raise SystemExit("at least 50 timed calls after at least 10 warm-ups")
    if not torch.cuda.is_available():
        raise SystemExit("the measurement runs on the GPU; there is none here")
    gen = torch.Generator()
    gen.manual_seed(1)
    res = {"workload": {"taps": K, "block": P, "max_blocks": MAXB, "batches": list(BS), "blocks_per_push": list(BLOCKS),
                        "dry": ["shared", "rows"], "floor_blocks": FLOOR_BLOCKS, "sample_rate": SR},
           "calls": a.calls, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for B in BS:
        for blocks in BLOCKS:
            for rows in (False, True):
                res[f"B={B} blocks={blocks} {'rows' if rows else 'shared'}"] = measure(B, blocks, rows, a, gen)
                with open(a.out, "w") as f:                       # after every point: a later failure keeps the earlier figures
                    json.dump(res, f, indent=1)
                    f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
