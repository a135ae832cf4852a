"""What the host side of the engines owes everything below and above it, on CPU (simulated runtime, CPU operators):

  * the flat parameter layout (name, offset, shape, kind - checkpoints, gradient buckets and the Keras converters depend on it) and
    the launch order of one Trainer.step, stream by stream, of all six engines with overlap_wgrad off and on, equal the recording
    tests/golden/engine_contract.json (tests/golden/make_engine_contract_golden.py): rearranging the host code moves no launch;
  * the input gate: every tensor a caller hands to forward / loss_from_logits / backward reaches a kernel as a raw pointer, so a
    wrong shape, dtype, layout or device is refused with ValueError BEFORE the first launch of the call (the launch trace does not
    grow).  "Another device" is a meta tensor here; on the GPU it would be a host tensor, and the refused call a memory fault.
"""
import importlib.util
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_engine_contract_golden", os.path.join(GOLDEN, "make_engine_contract_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


REC = _recorder()


@pytest.fixture(scope="module")
def recording():
    with open(REC.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize("kind", REC.KINDS)
def test_parameter_layout_and_launch_order_equal_the_recording(recording, kind):
    params, plain = REC.record_one(kind, False)
    params_ov, overlap = REC.record_one(kind, True)
    assert params_ov == params
    got = {**recording, kind: {"params": params, "plain": plain, "overlap": overlap}}
    assert got[kind] == recording[kind], REC.first_difference(recording, got)


def test_the_recorder_reproduces_the_file_byte_for_byte():
    with open(REC.OUT) as f:
        text = f.read()
    assert REC.dumps(json.loads(text)) == text          # the serialisation is canonical: equal contents <=> equal bytes


def _bad_batches(good):
    """The four ways an NCHW batch can be wrong, as (label, tensor)."""
    B, C, H, W = good.shape
    return [("shape", torch.zeros(B, C, H, W + 1)),
            ("dtype", good.double()),
            ("non-contiguous", torch.zeros(B, C, W, H).transpose(2, 3)),
            ("device", torch.empty(B, C, H, W, device="meta"))]


@pytest.mark.parametrize("kind", REC.KINDS)
def test_the_gate_refuses_bad_tensors_before_any_launch(kind):
    mp, rt, eng = REC.installed(kind, False)
    try:
        spec, emb, target = REC.batch()
        assert not _bad_batches(spec)[2][1].is_contiguous() and _bad_batches(spec)[2][1].shape == spec.shape

        def refused(what, label, call):
            n = len(rt.trace)
            with pytest.raises(ValueError, match=what):
                call()
            assert len(rt.trace) == n, (what, label, rt.trace[n:])

        for label, bad in _bad_batches(spec):
            refused("spec", label, lambda: eng.forward(bad, emb))
            refused("spec", label, lambda: eng.forward(bad, emb, target=target))
            refused("target", label, lambda: eng.forward(spec, emb, target=bad))
            if hasattr(eng, "encode"):
                refused("spec", label, lambda: eng.encode(bad, emb))
        refused("emb", "shape", lambda: eng.forward(spec, emb.reshape(emb.shape[0], -1)))
        refused("emb", "shape", lambda: eng.forward(spec, emb[:1], target=target))
        eng.forward(spec, emb)                      # a good pass: there are logits and a prediction now
        n_good = len(rt.trace)
        assert n_good > 0
        if kind != "vae":                           # the VAE forms its loss in the forward pass only
            for label, bad in _bad_batches(target):
                refused("target", label, lambda: eng.loss_from_logits(bad))
        if kind in REC.TAKES_DPRED:
            for label, bad in _bad_batches(spec):
                refused("dpred", label, lambda: eng.backward(dpred=bad))
            eng.backward(dpred=torch.ones_like(spec))
            assert len(rt.trace) > n_good
    finally:
        mp.undo()
