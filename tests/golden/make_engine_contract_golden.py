"""Generates tests/golden/engine_contract.json: what the host side of every engine must keep when it is rearranged - the flat
parameter layout and the launch order of one train step.

Each of the six engines (UNetEngine, UNetGraphEngine mode 0 and mode 3, ResAEEngine, AutoencoderEngine, VAEEngine) is built on the
simulated runtime (tests/sim_runtime.py) with the CPU operators (tests/cpu_ops.py, tests/vae_cpu_ops.py) at the sizes of
tests/test_schedule_sim.py and tests/test_vae_sim.py, with overlap_wgrad off and on.  Recorded per engine:
    params   [name, offset, shape, kind] of every parameter, in the order of the flat buffers (the same with overlap off and on)
    plain / overlap   the launches of one Trainer.step: one "<stream name>:<what>" string per SimRuntime.touch, in order
The recording is made before a rearrangement and must come out byte for byte the same after it:

    python tests/golden/make_engine_contract_golden.py            (writes the file)
    python tests/golden/make_engine_contract_golden.py --check    (compares; prints the first differing line of every entry)
"""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p_ in (ROOT, os.path.join(ROOT, "tests")):          # run as a script (under pytest, tests/conftest.py has put ROOT there)
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import unet_rir_amd as U  # noqa: E402
from sim_runtime import SimRuntime  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "engine_contract.json")
H = W = 16
B = 2
AE_ARGS = ((4, 8, 8, 8), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)        # filters, kernels, strides, latent, n_neurons
KINDS = ("unet", "graph0", "graph3", "resae", "ae", "vae")
TAKES_DPRED = ("unet", "graph0", "graph3")          # engines the module's autograd bridge drives: backward(dpred=...)


class TracingRuntime(SimRuntime):
    """SimRuntime that also keeps the list of launches: "<stream name>:<what>" per touch."""

    def __init__(self):
        super().__init__()
        self.trace = []

    def touch(self, reads=(), writes=(), what="", stream=None):
        s = stream if stream is not None else self.current_stream()
        self.trace.append(f"{s.name}:{what}")
        super().touch(reads, writes, what, stream)


def make_engine(kind, rt, overlap):
    kw = dict(device="cpu", runtime=rt, overlap_wgrad=overlap)
    if kind == "unet":
        eng = U.UNetEngine(H, W, B, F0=4, k=3, **kw)
    elif kind in ("graph0", "graph3"):
        eng = U.UNetGraphEngine(H, W, B, F0=4, k=3, mode=int(kind[-1]), **kw)
    else:
        cls = {"resae": U.ResAEEngine, "ae": U.AutoencoderEngine, "vae": U.VAEEngine}[kind]
        eng = cls(H, W, B, *AE_ARGS, **kw)
    eng.reset_parameters(torch.Generator().manual_seed(0))
    return eng


def batch():
    from oracle import torch_ref as R
    return tuple(torch.tensor(a) for a in R.synthetic_batch(R.Config(H, W), B))


def installed(kind, overlap):
    """(monkeypatch, runtime, engine) with the CPU operators in place; the caller undoes the monkeypatch."""
    import cpu_ops
    import vae_cpu_ops
    mp = pytest.MonkeyPatch()
    rt = TracingRuntime()
    (vae_cpu_ops if kind == "vae" else cpu_ops).install(mp, rt)
    try:
        return mp, rt, make_engine(kind, rt, overlap)
    except Exception:
        mp.undo()
        raise


def record_one(kind, overlap):
    mp, rt, eng = installed(kind, overlap)
    try:
        tr = U.Trainer(eng, lr=1e-3, dropout=False, bucket_bytes=8192)
        del rt.trace[:]
        tr.step(*batch())
        params = [[n, s_.offset, list(s_.shape), s_.kind] for n, s_ in eng.specs.items()]
        return params, list(rt.trace)
    finally:
        mp.undo()


def record():
    doc = {}
    for kind in KINDS:
        params, plain = record_one(kind, False)
        params_ov, overlap = record_one(kind, True)
        if params != params_ov:
            raise AssertionError(f"{kind}: the parameter table depends on overlap_wgrad")
        doc[kind] = {"params": params, "plain": plain, "overlap": overlap}
    return doc


def dumps(doc):
    return json.dumps(doc, separators=(",", ":")) + "\n"


def first_difference(want, got):
    """One line per entry that differs: the first index at which the two lists part."""
    out = []
    for kind in KINDS:
        for key in ("params", "plain", "overlap"):
            a, b = want[kind][key], got[kind][key]
            if a != b:
                i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                out.append(f"{kind}/{key}: lengths {len(a)} / {len(b)}, first difference at {i}: "
                           f"{a[i] if i < len(a) else None!r} / {b[i] if i < len(b) else None!r}")
    return out


if __name__ == "__main__":
    doc = record()
    for kind in KINDS:
        print(f"{kind}: {len(doc[kind]['plain'])} / {len(doc[kind]['overlap'])} launches, {len(doc[kind]['params'])} parameters", file=sys.stderr)
    if "--check" in sys.argv[1:]:
        with open(OUT) as f:
            text = f.read()
        diff = first_difference(json.loads(text), doc)
        print("\n".join(diff) if diff else "identical", file=sys.stderr)
        sys.exit(0 if text == dumps(doc) else 1)
    with open(OUT, "w") as f:
        f.write(dumps(doc))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes", file=sys.stderr)
