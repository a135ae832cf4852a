"""GPU tests of the decay-loss kernels (csrc/decayloss.hip) and of the vector-Jacobian product of PostProcess (csrc/istft_bwd.hip), per
element against the fp64 closed forms of tests/decay_loss_ref.py with the bounds derived there (never measured on a kernel).  Every
output is carved out of a larger buffer with a canary either side and prefilled with NaN, so an element the kernels leave out shows."""
import functools

import numpy as np
import pytest
import torch

import decay_loss_ref as DR
import wave_loss_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1234.5
GUARD = 1024
WEIGHT, GLOBAL_BATCH, LOSS0 = 0.7, 4, 1.5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


class Guarded:
    def __init__(self, shape, dtype=torch.float32, fill=float("nan")):
        n = int(np.prod(shape))
        self.big = torch.full((n + 2 * GUARD,), CANARY, dtype=dtype, device=DEV)
        self.out = self.big[GUARD:GUARD + n].view(shape)
        if isinstance(fill, float):
            self.out.fill_(fill)
        else:
            self.out.copy_(fill)

    def result(self):
        torch.cuda.synchronize()
        assert bool((self.big[:GUARD] == CANARY).all()) and bool((self.big[GUARD + self.out.numel():] == CANARY).all())
        return self.out


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ------------------------------------------------------------------------------------------------------ the decay kernel
@functools.lru_cache(maxsize=None)
def decay_case(T, B, floor_db):
    """(wav_pred, wav_true, closed form): the first B rows of the inputs of the reference test"""
    yp, yt = DR.inputs(T)
    yp, yt = np.ascontiguousarray(yp[:B]), np.ascontiguousarray(yt[:B])
    return yp, yt, DR.closed_form(yp, yt, floor_db, weight=WEIGHT, global_batch=GLOBAL_BATCH)


def run_decay(U, yp, yt, floor_db, backward=True, exact_ws=True):
    """one call of ops.decay_loss -> (dwav: the kernel's, or the untouched NaN prefill without backward; decay_out; loss_out), with
    exactly the advertised workspace in front of a canary"""
    B, T = yp.shape
    dw, do = Guarded((B, T)), Guarded((2,), torch.float64)
    lo = torch.full((4,), LOSS0, dtype=torch.float32, device=DEV)
    need = U.ops.decay_loss_ws_bytes(B, T)
    assert need == 16 * B
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = U.ops.Workspace(DEV)
    if exact_ws:
        ws.buf = big[:need]
    U.ops.decay_loss(dev(yp), dev(yt), do.out, ws, floor_db=floor_db, weight=WEIGHT, global_batch=GLOBAL_BATCH,
                     dwav=dw.out if backward else None, loss_out=lo)
    out = dw.result(), do.result(), lo
    if exact_ws:
        assert ws.buf.data_ptr() == big.data_ptr() and bool((big[need:] == 0xA5).all())
    return out


def check_decay(got_dwav, got_out, got_lo, cf, what):
    got = got_dwav.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                                     # a NaN left over: an element not written
    err, tol = np.abs(got - cf["dwav"]), DR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    at = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    print(f"{what}: worst at {tuple(int(i) for i in at)}: err {err[at]:.3e} bound {tol[at]:.3e} value {cf['dwav'][at]:.3e}; "
          f"largest err / bound {float((err / tol).max()):.3f}")
    assert (err <= tol).all()
    o = got_out.cpu().numpy()
    print(f"  decay_out {o} reference {cf['decay_out']} allowance {cf['decay_out_tol']}")
    assert abs(o[0] - cf["decay_out"][0]) <= cf["decay_out_tol"][0] and o[1] == cf["decay_out"][1]
    want_lo = LOSS0 + cf["loss"]
    assert abs(float(got_lo[0]) - want_lo) <= WEIGHT / GLOBAL_BATCH * cf["decay_out_tol"][0] + 2.0 ** -24 * (abs(cf["loss"]) + abs(want_lo))
    assert bool((got_lo[1:] == LOSS0).all())


@pytest.mark.parametrize("floor_db", DR.FLOORS)
@pytest.mark.parametrize("B", DR.BATCHES)
@pytest.mark.parametrize("T", DR.LENGTHS)
def test_decay_every_element_against_the_closed_form(U, T, B, floor_db):
    yp, yt, cf = decay_case(T, B, floor_db)
    dw, do, lo = run_decay(U, yp, yt, floor_db)
    check_decay(dw, do, lo, cf, f"T {T} B {B} floor {floor_db}")
    assert cf["decay_out"][1] == B and cf["decay_out"][0] > 0
    # a second run: the same bits
    dw2, do2, lo2 = run_decay(U, yp, yt, floor_db, exact_ws=False)
    assert torch.equal(bits(dw2), bits(dw)) and torch.equal(bits(do2), bits(do)) and torch.equal(bits(lo2), bits(lo))
    # the loss alone: the same sums, and no dwav written (the NaN prefill stays)
    dw3, do3, lo3 = run_decay(U, yp, yt, floor_db, backward=False)
    assert bool(torch.isnan(dw3).all()) and torch.equal(bits(do3), bits(do)) and torch.equal(bits(lo3), bits(lo))


@pytest.mark.parametrize("T", DR.LENGTHS)
def test_decay_a_rows_bits_depend_neither_on_the_batch_nor_on_its_place(U, T):
    yp, yt, _ = decay_case(T, 3, 60.0)
    dw, _, _ = run_decay(U, yp, yt, 60.0)
    for rows in ((0,), (1,), (2,), (2, 0, 2)):
        sel = list(rows)
        d, do, _ = run_decay(U, np.ascontiguousarray(yp[sel]), np.ascontiguousarray(yt[sel]), 60.0)      # the same inv_global_batch
        for i, r in enumerate(rows):
            assert torch.equal(bits(d[i]), bits(dw[r])), (rows, i)
        assert float(do[1]) == len(rows)


@pytest.mark.parametrize("T", (1, 65, 1000, 9600))
def test_decay_a_zero_target_row_and_a_zero_prediction_row(U, T):
    """a silent target counts nothing - zeros in its row of dwav, nothing in either sum; a silent prediction has the floor for a curve
    and a gradient of exact zeros (dwav carries the factor y^), but counts"""
    yp, yt = (np.array(a) for a in DR.inputs(T))
    yt[1] = 0.0
    yp[2] = 0.0
    cf = DR.closed_form(yp, yt, 60.0, weight=WEIGHT, global_batch=GLOBAL_BATCH)
    assert list(cf["counted"]) == [True, False, True] and cf["Q"][2] > 0
    dw, do, lo = run_decay(U, yp, yt, 60.0)
    check_decay(dw, do, lo, cf, f"T {T} with silent rows")
    assert not bool(dw[1].any()) and not bool(dw[2].any()) and bool(dw[0].any()) and float(do[1]) == 2.0
    one, do1, _ = run_decay(U, yp[:1], yt[:1], 60.0)
    assert torch.equal(bits(one[0]), bits(dw[0]))
    # every target silent: both sums zero, loss_out unchanged
    dwz, doz, loz = run_decay(U, yp, np.zeros_like(yt), 60.0)
    assert not bool(dwz.any()) and not bool(doz.any()) and float(loz[0]) == LOSS0


def test_decay_loss_object(U):
    """DecayLoss on its own: keeps its buffers, returns dwav, equals the op; with pred it returns dpred = the vector-Jacobian product of
    its dwav; backward=False returns None"""
    inp = WR.inputs("edge", False)
    nb, nf = inp["des_shape"]
    geo = dict(des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"])
    dl = U.DecayLoss(weight=WEIGHT, floor_db=30.0, **geo)
    pred, y = dev(inp["pred"]), dev(inp["wav_true"])
    wav = U.features.PostProcess().post_process(pred, des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"],
                                                nhwc=False)
    dwav = dl(wav, y, global_batch=GLOBAL_BATCH)
    again = dl(wav, y, global_batch=GLOBAL_BATCH)
    assert again.data_ptr() == dwav.data_ptr() and tuple(dl.decay_out.shape) == (2,) and dl.decay_out.dtype == torch.float64
    want, do, _ = run_decay(U, wav.cpu().numpy(), inp["wav_true"], 30.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(dwav), bits(want)) and torch.equal(bits(dl.decay_out), bits(do)) and float(do[0]) > 0
    dpred = dl(wav, y, pred=pred, global_batch=GLOBAL_BATCH)
    by_op = torch.full_like(pred, float("nan"))
    U.ops.istft_features_bwd(pred, want, by_op, nb, nf, inp["n_fft"], inp["win"], inp["hop"])
    torch.cuda.synchronize()
    assert torch.equal(bits(dpred), bits(by_op)) and bool(dpred.any())
    base = torch.ones_like(pred)
    assert dl(wav, y, pred=pred, dpred=base, accumulate=True, global_batch=GLOBAL_BATCH) is base
    assert bool((base[:, :, nb:, :] == 1).all()) and bool((base[:, :, :, nf:] == 1).all()) and not torch.equal(base, torch.ones_like(pred))
    assert dl(wav, y, global_batch=GLOBAL_BATCH, backward=False) is None
    with pytest.raises(ValueError):
        dl(wav, y, pred=pred, accumulate=True)


# ------------------------------------------------------------------------------------------- the vector-Jacobian product
@functools.lru_cache(maxsize=None)
def vjp_case(name, tight, ref):
    inp = WR.inputs(name, tight)
    g = DR.cotangent(name)
    cf = DR.vjp_closed_form(inp["pred"], g, inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"], phase_ref=inp["phase_ref"] if ref else None)
    return inp, g, cf


def base_of(inp):
    """what dpred holds before an accumulating call: the layout's "feature" planes, of the size of a loss gradient"""
    return (np.asarray(inp["spec_target"], dtype=np.float32) - np.float32(0.5)) * np.float32(1e-3)


def run_vjp(U, inp, g, ref, accumulate, rows=None):
    sel = (lambda a: a) if rows is None else (lambda a: np.ascontiguousarray(a[list(rows)]))
    B = inp["B"] if rows is None else len(rows)
    nb, nf = inp["des_shape"]
    dp = Guarded((B, 2, inp["H"], inp["W"]), fill=dev(sel(base_of(inp))) if accumulate else float("nan"))
    U.ops.istft_features_bwd(dev(sel(inp["pred"])), dev(sel(g)), dp.out, nb, nf, inp["n_fft"], inp["win"], inp["hop"],
                             phase_ref=dev(sel(inp["phase_ref"])) if ref else None, accumulate=accumulate)
    return dp.result()


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("ref", [False, True], ids=["noref", "ref"])
@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_vjp_every_element_against_the_closed_form(U, name, tight, ref, accumulate):
    inp, g, cf = vjp_case(name, tight, ref)
    nb, nf = inp["des_shape"]
    dp = run_vjp(U, inp, g, ref, accumulate)
    got = dp.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                                     # a NaN left over: an element not written
    if accumulate:
        base = base_of(inp)
        want, tol = base.astype(np.float64) + cf["grad"], DR.bound_accumulated(base, cf["grad"], cf["abs"], cf["n_terms"])
        pad = np.ones(got.shape, dtype=bool)
        pad[:, :, :nb, :nf] = False
        assert np.array_equal(dp.cpu().numpy()[pad], base[pad])                       # the padding: untouched, bit for bit
    else:
        want, tol = cf["grad"], DR.bound(cf["grad"], cf["abs"], cf["n_terms"])
        assert not bool(dp[:, :, nb:, :].any()) and not bool(dp[:, :, :, nf:].any())  # exact zeros in the padding
    err = np.abs(got - want)
    at = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    print(f"{name} ref {ref} accumulate {accumulate}: worst at {tuple(int(i) for i in at)}: err {err[at]:.3e} bound {tol[at]:.3e} value "
          f"{want[at]:.3e}; largest err / bound {float((err / tol).max()):.3f}")
    assert (err <= tol).all() and np.abs(cf["grad"]).max() > 0
    # a second run: the same bits; a row alone or elsewhere in a batch: the same bits
    assert torch.equal(bits(run_vjp(U, inp, g, ref, accumulate)), bits(dp))
    for rows in ((1,), (1, 0, 1)):
        d = run_vjp(U, inp, g, ref, accumulate, rows=rows)
        for i, r in enumerate(rows):
            assert torch.equal(bits(d[i]), bits(dp[r])), (rows, i)


@pytest.mark.parametrize("ref", [False, True], ids=["noref", "ref"])
@pytest.mark.parametrize("name,tight", WR.LAYOUTS, ids=WR.LAYOUT_IDS)
def test_vjp_of_the_wave_loss_cotangent_is_the_wave_loss_gradient(U, name, tight, ref):
    """dwav = the cotangent WaveLoss forms, scale_b w[t] (y^[t] - y[t]), here from the fp64 reference and rounded to fp32: the
    vector-Jacobian product is that loss's gradient.  Allowance: the VJP kernel's bound on its own reference, the wave loss's bound on
    its own, and 2^-24 abs for the one rounding of each dwav element, which the linear map passes on term by term."""
    inp = WR.inputs(name, tight)
    nb, nf = inp["des_shape"]
    geo = (inp["des_shape"], inp["n_fft"], inp["win"], inp["hop"])
    pr = inp["phase_ref"] if ref else None
    wl = WR.closed_form(inp["pred"], inp["wav_true"], *geo, norm="energy", weight=WEIGHT, global_batch=GLOBAL_BATCH,
                        time_weight=inp["time_weight"], phase_ref=pr)
    g32 = (wl["scale"][:, None] * inp["time_weight"].astype(np.float64)[None, :] * (wl["wav"] - inp["wav_true"].astype(np.float64))).astype(np.float32)
    cf = DR.vjp_closed_form(inp["pred"], g32, *geo, phase_ref=pr)
    mine = run_vjp(U, inp, g32, ref, False)
    theirs = torch.full_like(mine, float("nan"))
    U.ops.wave_loss(dev(inp["pred"]), dev(inp["wav_true"]), torch.zeros(2, dtype=torch.float64, device=DEV), U.ops.Workspace(DEV), nb, nf,
                    inp["n_fft"], inp["win"], inp["hop"], norm="energy", weight=WEIGHT, global_batch=GLOBAL_BATCH,
                    time_weight=dev(inp["time_weight"]), phase_ref=dev(pr), dpred=theirs)
    torch.cuda.synchronize()
    tol = DR.bound(cf["grad"], cf["abs"], cf["n_terms"]) + WR.bound(wl["grad"], wl["abs"], wl["n_terms"]) + 2.0 ** -24 * cf["abs"]
    err = np.abs(mine.cpu().numpy().astype(np.float64) - theirs.cpu().numpy().astype(np.float64))
    print(f"{name} ref {ref}: largest err / allowance {float((err / tol).max()):.3f}")
    assert (err <= tol).all() and bool(theirs.any())


@pytest.mark.parametrize("name", ["oddwin", "edge"])
def test_postprocess_differentiable(U, name):
    """torch.autograd.grad of sum(c * wav) through PostProcess.differentiable is the vector-Jacobian product with c, and its forward
    is the inverse-STFT op"""
    inp, g, _ = vjp_case(name, False, True)
    nb, nf = inp["des_shape"]
    kw = dict(des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"])
    for ref in (None, dev(inp["phase_ref"])):
        pred = dev(inp["pred"]).requires_grad_(True)
        wav = U.features.PostProcess.differentiable(pred, phase_ref=ref, **kw)
        feat = dev(inp["pred"]).clone()
        if ref is not None:
            feat[:, 1] += ref[:, 1]
        want_wav = torch.empty_like(wav)
        U.ops.istft_features(feat, want_wav, nb, nf, inp["n_fft"], inp["win"], inp["hop"], denormalize=True)
        c = dev(g)
        grad, = torch.autograd.grad((c * wav).sum(), pred)
        want = run_vjp(U, inp, g, ref is not None, False)
        torch.cuda.synchronize()
        assert torch.equal(bits(wav.detach()), bits(want_wav)) and torch.equal(bits(grad), bits(want)) and bool(grad.any())
    # any torch expression on the waveform: the chain rule goes through
    pred = dev(inp["pred"]).requires_grad_(True)
    wav = U.features.PostProcess.differentiable(pred, **kw)
    (wav ** 2).sum().backward()
    by_op = torch.empty_like(pred)
    U.ops.istft_features_bwd(pred.detach(), (2.0 * wav.detach()).contiguous(), by_op, nb, nf, inp["n_fft"], inp["win"], inp["hop"])
    torch.cuda.synchronize()
    assert torch.equal(bits(pred.grad), bits(by_op))
