"""GPU tests of the waveform-loss kernels (csrc/waveloss.hip) per element against the fp64 closed form of tests/wave_loss_ref.py, on
the geometries of tests/features_cases.py, with the bounds derived there (never measured on a kernel).  Every output is carved out of
a larger buffer with a canary either side and prefilled with NaN, so an element the kernels leave out shows."""
import functools
import itertools

import numpy as np
import pytest
import torch

import wave_loss_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1234.5
GUARD = 1024
WEIGHT, GLOBAL_BATCH, LOSS0 = 0.7, 4, 1.5
SWITCHES = list(itertools.product(("mse", "energy"), (False, True), (False, True), (False, True)))     # norm, time_weight, phase_ref, fused
SWITCH_IDS = ["-".join([n, "tw" if t else "ones", "ref" if r else "noref", "fused" if f else "plain"]) for n, t, r, f in SWITCHES]


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


class Guarded:
    def __init__(self, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.big = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=DEV)
        self.out = self.big[GUARD:GUARD + n].view(shape)
        self.out.fill_(float("nan"))

    def result(self):
        torch.cuda.synchronize()
        assert bool((self.big[:GUARD] == CANARY).all()) and bool((self.big[GUARD + self.out.numel():] == CANARY).all())
        return self.out


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def reference(name, tight, norm, tw, ref, fused):
    inp = WR.inputs(name, tight)
    kw = WR.options(inp, norm, tw, ref, fused, weight=WEIGHT)
    return WR.closed_form(inp["pred"], inp["wav_true"], inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"], global_batch=GLOBAL_BATCH, **kw)


def run(U, inp, norm, tw, ref, fused, rows=None, backward=True, ws=None, wav_true=None):
    """one call of ops.wave_loss on the (rows of the) layout's inputs -> (dpred or None, wav_pred, wave_out, loss_out) on the device"""
    sel = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[list(rows)]))
    B = inp["B"] if rows is None else len(rows)
    nb, nf = inp["des_shape"]
    dp, wv, wo = Guarded((B, 2, inp["H"], inp["W"])), Guarded((B, inp["T"])), Guarded((2,), torch.float64)
    lo = torch.full((4,), LOSS0, dtype=torch.float32, device=DEV)
    kw = WR.options(inp, norm, tw, ref, fused, weight=WEIGHT)
    for k in ("phase_ref", "spec_target"):
        if kw.get(k) is not None:
            kw[k] = dev(sel(kw[k]))
    for k in ("time_weight", "phase_weight"):
        if kw.get(k) is not None:
            kw[k] = dev(kw[k])
    U.ops.wave_loss(dev(sel(inp["pred"])), dev(sel(inp["wav_true"] if wav_true is None else wav_true)), wo.out,
                    ws if ws is not None else U.ops.Workspace(DEV), nb, nf, inp["n_fft"], inp["win"], inp["hop"],
                    global_batch=GLOBAL_BATCH, dpred=dp.out if backward else None, wav_pred=wv.out, loss_out=lo, **kw)
    return (dp.result() if backward else None), wv.result(), wo.result(), lo


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("sw", SWITCHES, ids=SWITCH_IDS)
@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_every_element_against_the_closed_form(U, name, tight, sw):
    norm, tw, ref, fused = sw
    inp = WR.inputs(name, tight)
    cf = reference(name, tight, *sw)
    nb, nf = inp["des_shape"]
    dp, wv, wo, lo = run(U, inp, *sw)
    got = dp.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                                     # a NaN left over: an element not written
    err, tol = np.abs(got - cf["grad"]), WR.bound(cf["grad"], cf["abs"], cf["n_terms"])
    at = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    print(f"{name} {sw}: worst at {tuple(int(i) for i in at)}: err {err[at]:.3e} bound {tol[at]:.3e} value {cf['grad'][at]:.3e}; "
          f"largest err / bound {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    if not fused:
        assert not bool(dp[:, :, nb:, :].any()) and not bool(dp[:, :, :, nf:].any())  # exact zeros in the padding
    # the waveform: the bits of ops.istft_features on the planes the loss reconstructs from
    feat = dev(inp["pred"]).clone()
    if ref:
        feat[:, 1] += dev(inp["phase_ref"])[:, 1]
    want = torch.empty_like(wv)
    U.ops.istft_features(feat, want, nb, nf, inp["n_fft"], inp["win"], inp["hop"], denormalize=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(wv), bits(want))
    # the two sums and the increment of loss_out[0], each within its own summation bound
    w = wo.cpu().numpy()
    print(f"  wave_out {w} reference {cf['wave_out']} allowance {cf['wave_out_tol']}")
    assert (np.abs(w - cf["wave_out"]) <= cf["wave_out_tol"]).all()
    want_lo = LOSS0 + cf["loss"]
    assert abs(float(lo[0]) - want_lo) <= WEIGHT / GLOBAL_BATCH * cf["wave_out_tol"][0] + 2.0 ** -24 * (abs(cf["loss"]) + abs(want_lo))
    assert bool((lo[1:] == LOSS0).all())
    # the loss alone: the same bits, dpred not needed
    _, wv2, wo2, lo2 = run(U, inp, *sw, backward=False)
    assert torch.equal(bits(wo2), bits(wo)) and torch.equal(bits(wv2), bits(wv)) and torch.equal(bits(lo2), bits(lo))
    # a second run: the same bits
    dp3, _, wo3, _ = run(U, inp, *sw)
    assert torch.equal(bits(dp3), bits(dp)) and torch.equal(bits(wo3), bits(wo))


@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_a_rows_bits_depend_neither_on_the_batch_nor_on_its_place(U, name, tight):
    inp = WR.inputs(name, tight)
    sw = ("energy", True, True, True)
    dp, wv, _, _ = run(U, inp, *sw)
    for rows in ((0,), (1,), (1, 0, 1)):
        d, w, _, _ = run(U, inp, *sw, rows=rows)
        for i, r in enumerate(rows):
            assert torch.equal(bits(d[i]), bits(dp[r])) and torch.equal(bits(w[i]), bits(wv[r])), (rows, i)


def test_exact_size_workspace_in_front_of_a_canary(U):
    inp = WR.inputs("oddwin", False)
    need = U.ops.wave_loss_ws_bytes(inp["B"], inp["des_shape"][1], inp["hop"])
    assert need == 8 * (inp["B"] * inp["T"] + 2 * inp["B"] * -(-inp["T"] // 64) + inp["B"])
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = U.ops.Workspace(DEV)
    ws.buf = big[:need]
    sw = ("energy", True, True, True)
    dp, _, wo, _ = run(U, inp, *sw, ws=ws)
    assert ws.buf.data_ptr() == big.data_ptr() and bool((big[need:] == 0xA5).all())
    ref_dp, _, ref_wo, _ = run(U, inp, *sw)
    assert torch.equal(bits(dp), bits(ref_dp)) and torch.equal(bits(wo), bits(ref_wo))


def test_a_silent_target_counts_nothing_under_the_energy_norm(U):
    inp = WR.inputs("oddwin", False)
    y = np.array(inp["wav_true"])
    y[1] = 0.0
    dp, _, wo, lo = run(U, inp, "energy", False, False, False, wav_true=y)
    cf = WR.closed_form(inp["pred"], y, inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"], norm="energy", weight=WEIGHT,
                        global_batch=GLOBAL_BATCH)
    assert not bool(dp[1].any()) and bool(dp[0].any())
    assert (np.abs(wo.cpu().numpy() - cf["wave_out"]) <= cf["wave_out_tol"]).all()
    one, _, wo1, _ = run(U, inp, "energy", False, False, False, rows=(0,), wav_true=y)
    assert torch.equal(bits(one[0]), bits(dp[0])) and float(wo1[0]) == float(wo[0])


def test_wave_loss_object_and_nan_prefill(U):
    """WaveLoss on its own: keeps its buffers, returns dpred, equals the op; forward-only returns None."""
    inp = WR.inputs("edge", False)
    nb, nf = inp["des_shape"]
    wl = U.WaveLoss(weight=WEIGHT, norm="energy", time_weight=inp["time_weight"], des_shape=(nb, nf), n_fft=inp["n_fft"],
                    win_length=inp["win"], hop_length=inp["hop"])
    pred, y = dev(inp["pred"]), dev(inp["wav_true"])
    dp = wl(pred, y, global_batch=GLOBAL_BATCH, want_wav=True)
    again = wl(pred, y, global_batch=GLOBAL_BATCH)
    assert again.data_ptr() == dp.data_ptr() and tuple(wl.wave_out.shape) == (2,) and wl.wave_out.dtype == torch.float64
    want, wv, wo, _ = run(U, inp, "energy", True, False, False)
    torch.cuda.synchronize()
    assert torch.equal(bits(dp), bits(want)) and torch.equal(bits(wl.wav_pred), bits(wv)) and torch.equal(bits(wl.wave_out), bits(wo))
    assert wl(pred, y, global_batch=GLOBAL_BATCH, backward=False) is None
