"""The two references of tests/spectral_loss_ref.py against each other and against finite differences, on the CPU: the closed form the
GPU tests hold the kernels to is the gradient of the loss written out literally on torch.stft, and its bound says something."""
import functools

import numpy as np
import pytest
import torch

import spectral_loss_ref as SR

CASES = [(c[0], (tuple(c[1:]),)) for c in SR.SINGLE] + list(SR.MULTI)
IDS = ["-".join(map(str, (T,) + tuple(v for r in res for v in r))) for T, res in CASES]
KW = dict(sc_weight=0.8, log_weight=1.3, weight=0.7, global_batch=4)


@functools.lru_cache(maxsize=None)
def case(T, res, floor_db):
    yp, yt = SR.inputs(T)
    return yp, yt, SR.closed_form(yp, yt, res, floor_db, **KW)


@pytest.mark.parametrize("floor_db", SR.FLOORS)
@pytest.mark.parametrize("T,res", CASES, ids=IDS)
def test_closed_form_is_autograd_of_the_literal_loss(T, res, floor_db):
    yp, yt, cf = case(T, res, floor_db)
    val, grad = SR.autograd(yp, yt, res, floor_db, **KW)
    sc, lm, ok = SR.terms(torch.from_numpy(np.array(yp)).double(), torch.from_numpy(np.array(yt)).double(), res, floor_db)
    assert abs(cf["loss"] - val) <= 1e-9 * abs(val) and cf["loss"] > 0
    assert np.allclose(cf["SC"], sc.numpy(), rtol=1e-9, atol=0) and np.allclose(cf["LM"], lm.numpy(), rtol=1e-9, atol=0)
    scale = np.abs(grad).max(axis=1, keepdims=True)
    assert (scale > 0).all() and (np.abs(cf["dwav"] - grad) <= 1e-9 * scale).all()
    assert cf["spectral_out"][2] == yp.shape[0] and bool(ok.all())
    # the difference of the two fp64 references lies inside the allowance the device gets, less its fp32 rounding
    assert (np.abs(cf["dwav"] - grad) <= cf["n_terms"] * SR.U53 * cf["abs"]).all()


@pytest.mark.parametrize("T,res", CASES[:3] + [SR.MULTI[1]], ids=IDS[:3] + ["two"])
def test_closed_form_agrees_with_central_differences(T, res):
    yp, yt = SR.inputs(T, 2)
    cf = SR.closed_form(yp, yt, res, 60.0, **KW)
    p, t = torch.from_numpy(np.array(yp)).double(), torch.from_numpy(np.array(yt)).double()
    for b, s in ((0, 0), (0, 1), (1, T // 2), (1, T - 1), (0, T - 2), (1, 5)):
        h = 1e-6 * float(np.abs(yp[b]).max())            # the rows decay fast: a step that is small against the signal
        hi, lo = p.clone(), p.clone()
        hi[b, s] += h
        lo[b, s] -= h
        fd = float(SR.loss(hi, t, res, 60.0, **KW) - SR.loss(lo, t, res, 60.0, **KW)) / (2.0 * h)
        assert abs(fd - cf["dwav"][b, s]) <= 1e-6 * np.abs(cf["dwav"][b]).max(), (b, s)


def test_a_silent_target_counts_nothing():
    res = ((64, 64, 16), (16, 7, 3))
    yp, yt = SR.inputs(257)
    yt = np.array(yt)
    yt[1] = 0.0
    cf = SR.closed_form(yp, yt, res, 60.0)
    val, grad = SR.autograd(yp, yt, res, 60.0)
    assert list(cf["counted"]) == [True, False, True] and cf["spectral_out"][2] == 2 and not cf["SC"][1].any() and not cf["LM"][1].any()
    assert not cf["dwav"][1].any() and cf["dwav"][0].any() and not grad[1].any()
    assert abs(cf["loss"] - val) <= 1e-12 * val
    # the other rows are what they are without it
    alone = SR.closed_form(yp[[0, 2]], yt[[0, 2]], res, 60.0, global_batch=3)
    assert np.array_equal(alone["dwav"][0], cf["dwav"][0]) and np.array_equal(alone["dwav"][1], cf["dwav"][2])
    # a silent prediction counts, with a gradient of exact zeros and an allowance of zero
    yp = np.array(yp)
    yp[2] = 0.0
    cf = SR.closed_form(yp, yt, res, 60.0)
    assert cf["counted"][2] and cf["SC"][2].all() and not cf["dwav"][2].any() and not cf["abs"][2].any()


def test_the_gradient_of_several_resolutions_is_the_mean_of_the_single_ones():
    T, res = SR.MULTI[1]
    yp, yt = SR.inputs(T)
    both = SR.closed_form(yp, yt, res, 60.0, **KW)
    singles = [SR.closed_form(yp, yt, (r,), 60.0, **KW) for r in res]
    mean = sum(s["dwav"] for s in singles) / len(res)
    assert (np.abs(both["dwav"] - mean) <= 1e-14 * np.abs(mean).max()).all()
    assert abs(both["loss"] - sum(s["loss"] for s in singles) / len(res)) <= 1e-14 * both["loss"]
    assert np.allclose(both["SC"], np.concatenate([s["SC"] for s in singles], axis=1), rtol=1e-15)


def test_identical_waveforms_cost_nothing():
    _, yt = SR.inputs(1000, 2)
    same = SR.closed_form(yt, yt, SR.MULTI[1][1], 60.0)
    assert same["loss"] == 0.0 and not same["dwav"].any()


@pytest.mark.parametrize("floor_db", SR.FLOORS)
@pytest.mark.parametrize("T,res", CASES, ids=IDS)
def test_the_bound_is_not_vacuous_on_the_gpu_tests_inputs(T, res, floor_db):
    """the share of dwav elements whose allowance exceeds 2^-20 of their row's largest reference value stays under 1 %, and
    |dwav| <= abs"""
    yp, yt, cf = case(T, res, floor_db)
    tol = SR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    top = np.abs(cf["dwav"]).max(axis=1, keepdims=True)
    assert (top > 0).all() and (np.abs(cf["dwav"]) <= cf["abs"] * (1 + 1e-12)).all()
    share = float((tol > 2.0 ** -20 * top).mean())
    print(f"T {T} {res} floor {floor_db}: share {share:.4f}, largest allowance / row maximum {float((tol / top).max()):.3e}, "
          f"spectral_out {cf['spectral_out']} allowance {cf['spectral_out_tol']}")
    assert share < 0.01
    assert (cf["spectral_out_tol"][:2] <= 1e-6 * cf["spectral_out"][:2]).all()
