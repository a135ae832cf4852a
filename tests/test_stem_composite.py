"""The algebra of the stem's composite gradient (csrc/stem_composite.hip, tests/stem_composite_ref.py) against autograd of the
two-layer stack Conv2D(3x3, bias) -> Conv2D(3x3) on the oracle's own convolution, in fp64: the 5x5 correlation, the border terms
for the zero padding of the tensor between the layers, and the contraction.  The 3x3 image makes every pixel a border pixel with
all four corners adjacent - where a wrong predicate shows first.  A second part runs the product's step schedule with the op
modelled on the simulated operators: same results as the oracle's step, and no unordered cross-stream access.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stem_composite_ref as SC  # noqa: E402


def _autograd(x, g, w0, b0, w1):
    from oracle import torch_ref as R
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    w0t, b0t = t(w0).requires_grad_(True), t(b0).requires_grad_(True)
    d = R.conv2d_same(t(x).permute(0, 3, 1, 2), w0t.permute(1, 2, 3, 0), b0t, 1)            # [Cout][k][k][Cin] -> HWIO
    y = R.conv2d_same(d, t(w1).permute(1, 2, 3, 0), None, 1)
    gw, gb = torch.autograd.grad(y, (w0t, b0t), t(g).permute(0, 3, 1, 2))
    return gw.numpy(), gb.numpy()


@pytest.mark.parametrize("H,W", [(5, 7), (8, 8), (3, 3)])
def test_composite_formulas_equal_autograd_of_the_two_layer_stack(H, W):
    rng = np.random.default_rng(100 * H + W)
    B, Ci, C0, C1 = 2, 2, 4, 3
    x, g = rng.standard_normal((B, H, W, Ci)), rng.standard_normal((B, H, W, C1))
    w0, b0, w1 = rng.standard_normal((C0, 3, 3, Ci)), rng.standard_normal(C0), rng.standard_normal((C1, 3, 3, C0))
    want_w, want_b = _autograd(x, g, w0, b0, w1)
    got_w, got_b = SC.stem_composite(x, g, w1)
    assert np.abs(got_w - want_w).max() <= 1e-10 * np.abs(want_w).max()
    assert np.abs(got_b - want_b).max() <= 1e-10 * np.abs(want_b).max()
    # the border terms are not optional: without them the result is wrong by far more than the tolerance
    S, T, E, F = SC.terms(x, g)
    no_w, no_b = SC.contract(S, T, np.zeros_like(E), np.zeros_like(F), w1)
    assert np.abs(no_w - want_w).max() > 1e-3 * np.abs(want_w).max()
    assert np.abs(no_b - want_b).max() > 1e-3 * np.abs(want_b).max()
    # the weight-decay term is added on the result
    reg_w, _ = SC.stem_composite(x, g, w1, 0.25, w0)
    assert np.abs(reg_w - (want_w + 0.25 * w0)).max() <= 1e-10 * np.abs(want_w).max()


def test_chain_equals_autograd_of_the_two_layer_stack():
    """SC.chain, the reference of the exact device tests, is the oracle's two layers under autograd - on integers, so with ==."""
    rng = np.random.default_rng(7)
    B, H, W, Ci, C0, C1 = 2, 4, 6, 2, 5, 3
    x, g = rng.integers(-1, 4, (B, H, W, Ci)), rng.integers(-1, 4, (B, H, W, C1))
    w0, b0, w1 = rng.integers(-1, 3, (C0, 3, 3, Ci)), rng.integers(-3, 4, C0), rng.integers(-1, 3, (C1, 3, 3, C0))
    want_w, want_b = _autograd(x, g, w0, b0, w1)
    got_w, got_b = SC.chain(x, g, w1)
    assert np.array_equal(got_w, want_w) and np.array_equal(got_b, want_b)
    reg_w, reg_b = SC.chain(x, g, w1, 0.5, w0)
    assert np.array_equal(reg_w, want_w + 0.5 * w0) and np.array_equal(reg_b, want_b)


@pytest.mark.parametrize("B,H,W", SC.EXACT_SHAPES)
def test_exact_data_chain_equals_formulas_and_stays_exact_in_fp32(B, H, W):
    """What tests/test_stem_composite_exact_gpu.py rests on, from the reference's side only (no kernel output is looked at): on the
    integer data of each of its shapes the two-layer chain and the S, T, E, F formulas agree in every element; the inputs are
    integers that bfloat16 holds; every fp32 partial sum of the device (products of magnitude <= 9 over at most P = B H W pixels)
    stays below 2^24 in any order; and so does the result - below 2^23 where it is used with reg = 0.5, so that result + 0.5 * w0
    is exact in fp32, fused or not."""
    import exact_data as X
    c = SC.exact_case(B, H, W)
    t = torch.tensor
    X.check_exactness_conditions({"x": (t(c["x"]), True), "g": (t(c["g"]), True), "w1": (t(c["w1"]), True), "w0": (t(c["w0"]), False)},
                                 9 * B * H * W, what=f"stem composite {B}x{H}x{W}")
    assert max(map(abs, X.ACT)) ** 2 == 9 and 9 * B * H * W < 2 ** 24
    assert c["x"].shape == (B, H, W, 2) and c["g"].shape == (B, H, W, 64) and c["dw0"].shape == (64, 3, 3, 2) and c["db0"].shape == (64,)
    got_w, got_b = SC.stem_composite(c["x"], c["g"], c["w1"])
    assert np.array_equal(c["dw0"], got_w) and np.array_equal(c["db0"], got_b)
    big = max(np.abs(c["dw0"]).max(), np.abs(c["db0"]).max())
    assert big < 2 ** 24
    assert np.array_equal(c["dw0"], np.round(c["dw0"])) and np.array_equal(c["db0"], np.round(c["db0"]))
    assert (c["w0"][..., 2:] != 0).all()
    if (B, H, W) in SC.REG_SHAPES:
        reg_w, reg_b = SC.chain(c["x"], c["g"], c["w1"], X.REG, c["w0"][..., :2])
        assert np.array_equal(reg_w, c["dw0"] + X.REG * c["w0"][..., :2]) and np.array_equal(reg_b, c["db0"])
        assert np.abs(reg_w).max() < 2 ** 23 and big < 2 ** 23
    print(f"stem composite exact data {B}x{H}x{W}: P {B * H * W}, largest |dW0| {np.abs(c['dw0']).max():.4g}, |db0| {np.abs(c['db0']).max():.4g}")


def _model_stem_composite(rt):
    """The op on the simulated operators: reads g_y[1], the input and the transposed enc1.cb1 kernel, writes the two gradient ranges."""
    def stem_composite(g, x, w1t, dw0, db0, ws, reg=0.0, w0=None):
        rt.touch([g, x, w1t, w0 if reg else None], [dw0, db0, ws], "stem_composite")
        C0, C1 = dw0.shape[0], g.C
        w1 = w1t.reshape(C0, 3, 3, C1).to(torch.float64).permute(3, 1, 2, 0).numpy()          # [Cin][T][Cout] -> [Cout][k][k][Cin]
        gw, gb = SC.stem_composite(x.base[..., :2].to(torch.float64).numpy(), g.base[..., g.c0:g.c0 + g.C].to(torch.float64).numpy(), w1)
        out = torch.zeros(dw0.shape, dtype=torch.float64)
        out[..., :2] = torch.tensor(gw)
        if reg:
            out = out + reg * w0.reshape(dw0.shape).to(torch.float64)
        dw0.copy_(out.to(dw0.dtype))
        db0[:C0] = torch.tensor(gb).to(db0.dtype)
    return stem_composite


@pytest.mark.parametrize("overlap", [False, True])
def test_step_schedule_with_the_composite_op_matches_oracle(monkeypatch, overlap):
    import cpu_ops
    import test_schedule_sim as TS
    import unet_rir_amd as U
    from sim_runtime import SimRuntime
    from oracle import torch_ref as R
    rt = SimRuntime()
    cpu_ops.install(monkeypatch, rt)
    monkeypatch.setattr(U.ops, "stem_composite", _model_stem_composite(rt))
    B = 2
    cfg, eng, tr = TS._build(rt, B, overlap, bucket_bytes=8192)
    assert eng.stem_composite is False                 # a simulated device has no such kernel: off unless a test models the op
    eng.stem_composite_supported = eng.stem_composite = True
    launched = []
    touch = rt.touch
    monkeypatch.setattr(rt, "touch", lambda r=(), w=(), what="", **k: (launched.append(what), touch(r, w, what, **k))[1])
    spec_in, emb, spec_out = R.synthetic_batch(cfg, B)
    t = torch.tensor
    want_p, want_g, want_l = TS._oracle_steps(1, B, 2, 1e-3)
    loss = tr.step(t(spec_in), t(emb), t(spec_out), return_loss=True)
    assert abs(loss - want_l[0]) <= 1e-5 * abs(want_l[0])
    got_g = eng.export_keras_grads()
    floor = 1e-6 * max(float(g.abs().max()) for g in want_g.values())
    for n, g in want_g.items():
        e = float((got_g[n].double() - g).abs().max())
        assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
    loss2 = tr.step(t(spec_in), t(emb), t(spec_out), return_loss=True)
    assert abs(loss2 - want_l[1]) <= 1e-5 * abs(want_l[1])
    TS._check_params(eng, want_p)
    # the op replaced the full-resolution data gradient and the stem's weight gradient: per step one data gradient fewer than
    # encoder levels, one composite launch
    assert launched.count("stem_composite") == 2
    n_dgrad_enc = 2 * (eng.L - 1)                      # enc_l.cb1 (l >= 2) and enc_l.down (l >= 2); enc1.cb1's is gone
    n_dgrad_dec = 2 * eng.depth + 1                    # dec_l.cb1b, dec_l.cb1a; the head's
    n_dgrad_vec = 1                                    # vec.conv
    assert launched.count("conv2d_dgrad") == 2 * (n_dgrad_enc + n_dgrad_dec + n_dgrad_vec)
    if not overlap:
        assert rt.n_cross_stream == 0
