"""The two references of tests/decay_loss_ref.py against each other and against finite differences, on the CPU: the closed form the
GPU tests hold the kernels to is the gradient of the loss written out literally, and its bound says something."""
import numpy as np
import pytest

import decay_loss_ref as DR
import wave_loss_ref as WR

SMALL = (1, 2, 63, 65, 257, 1000)


@pytest.mark.parametrize("floor_db", DR.FLOORS)
@pytest.mark.parametrize("T", SMALL)
def test_closed_form_is_autograd_of_the_literal_loss(T, floor_db):
    yp, yt = DR.inputs(T)
    val, grad = DR.autograd(yp, yt, floor_db, weight=0.7, global_batch=4)
    cf = DR.closed_form(yp, yt, floor_db, weight=0.7, global_batch=4)
    assert abs(cf["loss"] - val) <= 1e-9 * abs(val) and cf["loss"] > 0
    scale = np.abs(grad).max(axis=1, keepdims=True)
    assert (np.abs(cf["dwav"] - grad) <= 1e-9 * scale).all()
    assert cf["decay_out"][1] == yp.shape[0]


def test_closed_form_agrees_with_central_differences():
    import torch
    T = 257
    yp, yt = DR.inputs(T, 2)
    cf = DR.closed_form(yp, yt, 60.0, weight=1.0, global_batch=2)
    p, t = torch.from_numpy(np.array(yp)).double(), torch.from_numpy(np.array(yt)).double()
    h = 1e-6
    for b, s in ((0, 0), (0, 5), (1, 100), (1, 256), (0, 200)):
        hi, lo = p.clone(), p.clone()
        hi[b, s] += h
        lo[b, s] -= h
        fd = float(DR.loss(hi, t, 60.0, 1.0, 2) - DR.loss(lo, t, 60.0, 1.0, 2)) / (2.0 * h)
        assert abs(fd - cf["dwav"][b, s]) <= 1e-6 * np.abs(cf["dwav"][b]).max(), (b, s)


def test_a_silent_target_counts_nothing():
    yp, yt = DR.inputs(65)
    yt = np.array(yt)
    yt[1] = 0.0
    cf = DR.closed_form(yp, yt, 60.0)
    val, grad = DR.autograd(yp, yt, 60.0)
    assert list(cf["counted"]) == [True, False, True] and cf["decay_out"][1] == 2 and cf["Q"][1] == 0
    assert not cf["dwav"][1].any() and cf["dwav"][0].any() and not grad[1].any()
    assert abs(cf["loss"] - val) <= 1e-12 * val
    # the other rows are what they are without it
    alone = DR.closed_form(yp[[0, 2]], yt[[0, 2]], 60.0, global_batch=3)
    assert np.array_equal(alone["dwav"][0], cf["dwav"][0]) and np.array_equal(alone["dwav"][1], cf["dwav"][2])


def test_a_scaled_prediction_moves_the_curve_by_the_expected_db():
    """both curves are normalised by the TARGET's energy: y^ = a y puts c_y^[0] at 10 log10(a^2 + delta) - 20 log10(a) dB but for the
    floor's delta = 1e-6 - while c_y[0] stays at 10 log10(1 + delta); a = 1/2 and 2 scale fp32 values exactly"""
    _, yt = DR.inputs(1000, 1)
    for a in (0.5, 2.0):
        cf = DR.closed_form((a * yt.astype(np.float64)).astype(np.float32), yt, 60.0)
        assert abs(cf["c_true"][0, 0] - 10.0 * np.log10(1.0 + 1e-6)) <= 1e-9
        assert abs(cf["c_pred"][0, 0] - 10.0 * np.log10(a * a + 1e-6)) <= 1e-9
        assert abs((cf["c_pred"][0, 0] - cf["c_true"][0, 0]) - 20.0 * np.log10(a)) <= 1e-4
    same = DR.closed_form(yt, yt, 60.0)
    assert same["loss"] == 0.0 and not same["dwav"].any()


@pytest.mark.parametrize("floor_db", DR.FLOORS)
@pytest.mark.parametrize("T", DR.LENGTHS)
def test_the_bound_is_not_vacuous_on_the_gpu_tests_inputs(T, floor_db):
    """the share of dwav elements whose allowance exceeds 2^-20 of their row's largest reference value stays under 1 %, and for the
    long cases both curves do run into the floor inside the row"""
    yp, yt = DR.inputs(T)
    cf = DR.closed_form(yp, yt, floor_db, weight=0.7, global_batch=4)
    tol = DR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    top = np.abs(cf["dwav"]).max(axis=1, keepdims=True)
    assert (top > 0).all()
    share = float((tol > 2.0 ** -20 * top).mean())
    print(f"T {T} floor {floor_db}: share {share:.4f}, largest allowance / row maximum {float((tol / top).max()):.3e}")
    assert share < 0.01
    if T >= 1000:
        assert (cf["c_true"][:, -1] < -floor_db + 0.5).all() and (cf["c_pred"][:, -1] < -floor_db + 0.5).all()
        assert (cf["c_true"][:, T // 8] > -floor_db + 3.0).all()          # ... and not at once: 11 to 14 dB down an eighth into the row


@pytest.mark.parametrize("name,tight", [("oddwin", False), ("gaps", False), ("edge", False)])
@pytest.mark.parametrize("ref", [False, True])
def test_vjp_closed_form_is_autograd_of_the_torch_chain(name, tight, ref):
    inp = WR.inputs(name, tight)
    g = DR.cotangent(name)
    pr = inp["phase_ref"] if ref else None
    geo = (inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"])
    cf = DR.vjp_closed_form(inp["pred"], g, *geo, phase_ref=pr)
    ag = DR.vjp_autograd(inp["pred"], g, *geo, phase_ref=pr)
    nb, nf = inp["des_shape"]
    assert (np.abs(cf["grad"] - ag) <= 1e-9 * np.abs(ag).max()).all() and np.abs(ag).max() > 0
    assert not cf["grad"][:, :, nb:, :].any() and not cf["grad"][:, :, :, nf:].any() and not ag[:, :, nb:, :].any()
    assert (np.abs(cf["grad"]) <= cf["abs"] * (1 + 1e-12)).all()


def test_vjp_closed_form_is_the_linear_part_of_the_wave_loss():
    """with the cotangent the wave loss forms, scale_b w[t] (y^[t] - y[t]), the vector-Jacobian product is that loss's gradient"""
    inp = WR.inputs("oddwin", False)
    geo = (inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"])
    wl = WR.closed_form(inp["pred"], inp["wav_true"], *geo, norm="energy", weight=0.7, global_batch=4, time_weight=inp["time_weight"])
    g = wl["scale"][:, None] * inp["time_weight"].astype(np.float64)[None, :] * (wl["wav"] - inp["wav_true"].astype(np.float64))
    g32 = g.astype(np.float32)
    cf = DR.vjp_closed_form(inp["pred"], g32, *geo)
    assert (np.abs(cf["grad"] - wl["grad"]) <= 2.0 ** -23 * cf["abs"] + 1e-12 * np.abs(wl["grad"]).max()).all()
