"""The fp64 references of the waveform-domain loss (tests/wave_loss_ref.py) hold together before any kernel is compared with them:
the torch restatement reproduces the oracle's waveform, the closed-form gradient equals autograd's, the adjoint identity holds,
finite differences agree, a waveform's own features give a vanishing loss, the D_b = 0 rule holds and the fused spectrogram term is
the gradient of the reference's compute_loss expression."""
import itertools
import math

import numpy as np
import pytest
import torch

import features_cases as FC
import wave_loss_ref as WR
from oracle import features as FO
from oracle import torch_ref

SWITCHES = list(itertools.product(("mse", "energy"), (False, True), (False, True), (False, True)))     # norm, time_weight, phase_ref, fused


def _geo(inp):
    return inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"]


@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_torch_waveform_equals_the_oracle(name, tight):
    inp = WR.inputs(name, tight)
    des, n_fft, win, hop = _geo(inp)
    yh = WR.t_waveform(torch.from_numpy(np.array(inp["pred"])).double(), des, n_fft, win, hop).numpy()
    for b in range(inp["B"]):
        want = FO.feature_to_wav(inp["pred"][b], des, n_fft, win, hop)
        assert np.abs(yh[b] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_closed_form_equals_autograd(name, tight):
    inp = WR.inputs(name, tight)
    for norm, tw, ref, fused in SWITCHES:
        kw = WR.options(inp, norm, tw, ref, fused)
        val, g = WR.autograd(inp["pred"], inp["wav_true"], *_geo(inp), **kw)
        cf = WR.closed_form(inp["pred"], inp["wav_true"], *_geo(inp), **kw)
        for plane in (0, 1):
            gap = np.abs(cf["grad"][:, plane] - g[:, plane]).max()
            assert gap <= 1e-10 * np.abs(g[:, plane]).max(), (norm, tw, ref, fused, plane, gap)
        if not fused:
            nb, nf = inp["des_shape"]
            assert abs(cf["loss"] - val) <= 1e-12 * abs(val)
            assert not cf["grad"][:, :, nb:, :].any() and not cf["grad"][:, :, :, nf:].any()       # padding: exact zeros
        assert (cf["abs"] >= np.abs(cf["grad"]) * (1 - 1e-12)).all()


@pytest.mark.parametrize("name", ["rir", "oddwin", "hop_eq_win", "gaps", "edge"])
def test_adjoint_identity(name):
    inp = WR.inputs(name, True)
    des, n_fft, win, hop = _geo(inp)
    rng = np.random.default_rng(5)
    S = rng.standard_normal(des) + 1j * rng.standard_normal(des)
    g = rng.standard_normal(inp["T"])
    adj = WR.adjoint(g, des, n_fft, win, hop)
    lhs = float(np.dot(FO.istft(S, n_fft, win, hop), g))
    rhs = float((S.real * adj.real + S.imag * adj.imag).sum())
    scale = float(np.abs(S.real * adj.real).sum() + np.abs(S.imag * adj.imag).sum())
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("name", ["oddwin", "hop_eq_win", "edge"])
def test_central_differences_agree_with_autograd(name):
    """20 seeded elements per plane, step h = 1e-6.  Allowance: truncation h^2 / 6 f''' with |f'''| <= (5 ln 10)^3 = 1526 (amplitude
    plane) or (2 pi)^3 = 248 (phase plane) times the plane's largest gradient -> below 1e-6 of it; rounding 4 ulp of the loss over h.
    Without phase_ref: the fp32 sum pred + phase_ref is a staircase of 2^-24 steps under a perturbation of 1e-6."""
    inp = WR.inputs(name, True)
    des, n_fft, win, hop = _geo(inp)
    kw = WR.options(inp, "energy", True, False, True)
    val, g = WR.autograd(inp["pred"], inp["wav_true"], des, n_fft, win, hop, **kw)
    t = lambda v: None if v is None else torch.from_numpy(np.array(v))
    tk = {k: (t(v).double() if k == "spec_target" else t(v)) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    base = torch.from_numpy(np.array(inp["pred"])).double()
    rng = np.random.default_rng(11)
    h = 1e-6
    nb, nf = des
    for plane in (0, 1):
        gmax = np.abs(g[:, plane]).max()
        for _ in range(20):
            b, k, f = int(rng.integers(inp["B"])), int(rng.integers(nb)), int(rng.integers(nf))
            vals = []
            for sgn in (1.0, -1.0):
                q = base.clone()
                q[b, plane, k, f] += sgn * h
                vals.append(float(WR.loss(q, t(inp["wav_true"]), des, n_fft, win, hop, **tk)))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[b, plane, k, f]) <= 1e-6 * gmax + 4 * 2.0 ** -53 * abs(val) / h, (plane, b, k, f)


@pytest.mark.parametrize("name", ["rir", "oddwin"])
def test_a_waveforms_own_features_give_no_loss(name):
    B, T0, n_fft, win, hop = FC.GEOMETRIES[name]
    des, T = FC.dims(name), FC.t_out(name)
    x = FC.waves(name, "noise").astype(np.float64)
    feat = np.stack([FO.wav_to_feature(x[b], des, n_fft, win, hop, remove_mean=False) for b in range(B)])
    _, E, _, _ = WR.wave_terms(torch.as_tensor(feat), torch.as_tensor(x[:, :T]), des, n_fft, win, hop)
    assert (E.numpy() <= 1e-10 * (x[:, :T] ** 2).sum(axis=1)).all()


def test_a_silent_target_counts_nothing_under_the_energy_norm():
    inp = WR.inputs("oddwin", False)
    y = np.array(inp["wav_true"])
    y[1] = 0.0
    kw = WR.options(inp, "energy", False, False, False)
    val, g = WR.autograd(inp["pred"], y, *_geo(inp), **kw)
    cf = WR.closed_form(inp["pred"], y, *_geo(inp), **kw)
    assert cf["D"][1] == 0.0 and cf["E"][1] > 0.0 and cf["wave_out"][1] == cf["E"].sum()
    assert not g[1].any() and not cf["grad"][1].any() and g[0].any()
    one = WR.closed_form(inp["pred"][:1], y[:1], *_geo(inp), **dict(kw, global_batch=2))
    assert cf["loss"] == one["loss"] and abs(val - one["loss"]) <= 1e-12 * abs(val)
    # "mse" divides by T: the silent sample counts
    assert WR.closed_form(inp["pred"], y, *_geo(inp), **dict(kw, norm="mse"))["grad"][1].any()


@pytest.mark.parametrize("ref,pw", [(False, False), (True, False), (False, True), (True, True)])
def test_fused_term_is_the_gradient_of_compute_loss(ref, pw):
    inp = WR.inputs("oddwin", False)
    kw = WR.options(inp, "mse", False, ref, True, weight=0.0)
    if not pw:
        kw["phase_weight"] = None
    cf = WR.closed_form(inp["pred"], inp["wav_true"], *_geo(inp), **kw)
    p = torch.from_numpy(np.array(inp["pred"])).double().requires_grad_(True)
    tgt = torch.from_numpy(np.array(inp["spec_target"])).double()
    x_in = torch.from_numpy(np.array(inp["phase_ref"])).double() if ref else None
    wgt = torch.from_numpy(np.array(inp["phase_weight"])) if pw else None
    # the trainer's normalisation 1 / (2 H W global_batch) is data_loss's own; alpha as the C ABI passes it
    dl = torch_ref.data_loss(tgt, p, WR.f32(WR.ALPHA), inp["B"], x_in, wgt)
    dl.backward()
    g = p.grad.numpy()
    # inv_norm travels as fp32 (2^-24 relative); with phase_ref the kernel's fp32 t1 - ref moves ph by at most 2^-24 * 2 pi * |t1|
    slack = 2.0 ** -23 + (2.0 ** -22 * math.pi * 2.0 if ref else 0.0)
    for plane in (0, 1):
        assert np.abs(cf["grad"][:, plane] - g[:, plane]).max() <= slack * np.abs(g[:, plane]).max()
