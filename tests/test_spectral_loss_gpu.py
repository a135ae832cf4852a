"""GPU tests of the multi-resolution STFT loss kernels (csrc/spectralloss.hip), per element against the fp64 closed form of
tests/spectral_loss_ref.py with the bounds derived there (never measured on a kernel).  Every output is carved out of a larger buffer
with a canary either side and prefilled with NaN, so an element the kernels leave out shows; the workspace is exactly the advertised
size in front of a canary."""
import functools

import numpy as np
import pytest
import torch

import spectral_loss_ref as SR
import wave_loss_ref as WR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1234.5
GUARD = 1024
KW = dict(sc_weight=0.8, log_weight=1.3, weight=0.7, global_batch=4)
LOSS0 = 1.5
CASES = [(c[0], (tuple(c[1:]),)) for c in SR.SINGLE] + list(SR.MULTI)
IDS = ["-".join(map(str, (T,) + tuple(v for r in res for v in r))) for T, res in CASES]


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


@functools.lru_cache(maxsize=None)
def case(T, res, B, floor_db):
    """(wav_pred, wav_true, closed form): the first B rows of the inputs of the reference test"""
    yp, yt = SR.inputs(T)
    yp, yt = np.ascontiguousarray(yp[:B]), np.ascontiguousarray(yt[:B])
    return yp, yt, SR.closed_form(yp, yt, res, floor_db, **KW)


def base_of(yp):
    """what dwav holds before an accumulating call: of the size of another term's cotangent"""
    return (np.asarray(yp, dtype=np.float32) * np.float32(0.25) + np.float32(1e-3)).astype(np.float32)


def run(U, yp, yt, res, floor_db, backward=True, accumulate=False, exact_ws=True):
    """one call of ops.spectral_loss -> (dwav: the kernel's, or the untouched NaN prefill without backward; spectral_out; loss_out),
    with exactly the advertised workspace in front of a canary"""
    B, T = yp.shape
    dw = Guarded((B, T), fill=dev(base_of(yp)) if accumulate else float("nan"))
    so = Guarded((3,), torch.float64)
    lo = torch.full((4,), LOSS0, dtype=torch.float32, device=DEV)
    need = U.ops.spectral_loss_ws_bytes(B, T, res)
    assert need > 0 and need % 8 == 0
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = U.ops.Workspace(DEV)
    if exact_ws:
        ws.buf = big[:need]
    U.ops.spectral_loss(dev(yp), dev(yt), so.out, ws, res, floor_db=floor_db, sc_weight=KW["sc_weight"], log_weight=KW["log_weight"],
                        weight=KW["weight"], global_batch=KW["global_batch"], dwav=dw.out if backward else None, accumulate=accumulate,
                        loss_out=lo)
    out = dw.result(), so.result(), lo
    if exact_ws:
        assert ws.buf.data_ptr() == big.data_ptr() and bool((big[need:] == 0xA5).all())
    return out


def check(got_dwav, got_out, got_lo, cf, what, base=None):
    got = got_dwav.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                                     # a NaN left over: an element not written
    if base is None:
        want, tol = cf["dwav"], SR.bound(cf["dwav"], cf["abs"], cf["n_terms"])
    else:
        want, tol = base.astype(np.float64) + cf["dwav"], SR.bound_accumulated(base, cf["dwav"], cf["abs"], cf["n_terms"])
    err = np.abs(got - want)
    at = np.unravel_index(int(np.argmax(err - tol)), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(tol > 0, err / tol, np.where(err > 0, np.inf, 0.0))))
    print(f"{what}: worst at {tuple(int(i) for i in at)}: err {err[at]:.3e} bound {tol[at]:.3e} value {want[at]:.3e}; "
          f"largest err / bound {ratio:.3f}")
    assert (err <= tol).all()
    o = got_out.cpu().numpy()
    print(f"  spectral_out {o} reference {cf['spectral_out']} allowance {cf['spectral_out_tol']}")
    assert (np.abs(o[:2] - cf["spectral_out"][:2]) <= cf["spectral_out_tol"][:2]).all() and o[2] == cf["spectral_out"][2]
    want_lo = LOSS0 + cf["loss"]
    lo_tol = KW["weight"] / KW["global_batch"] * (KW["sc_weight"] * cf["spectral_out_tol"][0] + KW["log_weight"] * cf["spectral_out_tol"][1])
    assert abs(float(got_lo[0]) - want_lo) <= lo_tol + 2.0 ** -24 * (abs(cf["loss"]) + abs(want_lo))
    assert bool((got_lo[1:] == LOSS0).all())


@pytest.mark.parametrize("B", SR.BATCHES)
@pytest.mark.parametrize("T,res", CASES, ids=IDS)
def test_every_element_against_the_closed_form(U, T, res, B):
    yp, yt, cf = case(T, res, B, 60.0)
    dw, so, lo = run(U, yp, yt, res, 60.0)
    check(dw, so, lo, cf, f"T {T} {res} B {B}")
    assert cf["spectral_out"][2] == B and cf["spectral_out"][0] > 0 and cf["spectral_out"][1] > 0
    # a second run: the same bits
    dw2, so2, lo2 = run(U, yp, yt, res, 60.0, exact_ws=False)
    assert torch.equal(bits(dw2), bits(dw)) and torch.equal(bits(so2), bits(so)) and torch.equal(bits(lo2), bits(lo))
    # the loss alone: the same sums, and no dwav element touched (the NaN prefill stays)
    dw3, so3, lo3 = run(U, yp, yt, res, 60.0, backward=False)
    assert bool(torch.isnan(dw3).all()) and torch.equal(bits(so3), bits(so)) and torch.equal(bits(lo3), bits(lo))
    # accumulate: (float)((double) base + g), the same sums
    dw4, so4, lo4 = run(U, yp, yt, res, 60.0, accumulate=True)
    check(dw4, so4, lo4, cf, f"T {T} {res} B {B} accumulate", base=base_of(yp))
    assert torch.equal(bits(so4), bits(so))


@pytest.mark.parametrize("T,res", [CASES[1], CASES[4], CASES[6], SR.MULTI[1]], ids=[IDS[1], IDS[4], IDS[6], "two"])
def test_floor_30(U, T, res):
    yp, yt, cf = case(T, res, 3, 30.0)
    dw, so, lo = run(U, yp, yt, res, 30.0)
    check(dw, so, lo, cf, f"T {T} {res} floor 30")


@pytest.mark.parametrize("T,res", CASES, ids=IDS)
def test_a_rows_bits_depend_neither_on_the_batch_nor_on_its_place(U, T, res):
    yp, yt, _ = case(T, res, 3, 60.0)
    dw, _, _ = run(U, yp, yt, res, 60.0)
    for rows in ((1,), (2, 0, 2)):
        sel = list(rows)
        d, so, _ = run(U, np.ascontiguousarray(yp[sel]), np.ascontiguousarray(yt[sel]), res, 60.0)      # the same inv_global_batch
        for i, r in enumerate(rows):
            assert torch.equal(bits(d[i]), bits(dw[r])), (rows, i)
        assert float(so[2]) == len(rows)


@pytest.mark.parametrize("T,res", [CASES[1], CASES[3], SR.MULTI[0]], ids=[IDS[1], IDS[3], "default"])
def test_a_zero_target_row_and_a_zero_prediction_row(U, T, res):
    """a silent target counts nothing - zeros in its row of dwav, nothing in any sum; a silent prediction sits on the floor with a
    gradient of exact zeros (dRe, dIm carry the factor X^), but counts"""
    yp, yt = (np.array(a) for a in SR.inputs(T))
    yt[1] = 0.0
    yp[2] = 0.0
    cf = SR.closed_form(yp, yt, res, 60.0, **KW)
    assert list(cf["counted"]) == [True, False, True] and cf["SC"][2].all()
    dw, so, lo = run(U, yp, yt, res, 60.0)
    check(dw, so, lo, cf, f"T {T} with silent rows")
    assert not bool(dw[1].any()) and not bool(dw[2].any()) and bool(dw[0].any()) and float(so[2]) == 2.0
    one, _, _ = run(U, yp[:1], yt[:1], res, 60.0)
    assert torch.equal(bits(one[0]), bits(dw[0]))
    # accumulate leaves the silent rows' base as it is
    acc, _, _ = run(U, yp, yt, res, 60.0, accumulate=True)
    assert torch.equal(bits(acc[1:]), bits(dev(base_of(yp))[1:]))
    # every target silent: all sums zero, loss_out unchanged
    dwz, soz, loz = run(U, yp, np.zeros_like(yt), res, 60.0)
    assert not bool(dwz.any()) and not bool(soz.any()) and float(loz[0]) == LOSS0


def test_spectral_loss_object(U):
    """SpectralLoss on its own: keeps its buffers, returns dwav, equals the op; with pred it returns dpred = the vector-Jacobian
    product of its dwav bit for bit; dwav= adds; backward=False returns None"""
    inp = WR.inputs("oddwin", False)
    nb, nf = inp["des_shape"]
    geo = dict(des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"])
    T = inp["hop"] * (nf - 1)
    res = tuple(r for r in ((16, 16, 4), (64, 48, 12), (128, 64, 32)) if r[0] // 2 + 1 <= T)
    sl = U.SpectralLoss(weight=KW["weight"], resolutions=res, sc_weight=KW["sc_weight"], log_weight=KW["log_weight"], floor_db=30.0, **geo)
    assert sl.T == T and len(res) >= 2
    pred, y = dev(inp["pred"]), dev(inp["wav_true"])
    wav = U.features.PostProcess().post_process(pred, des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"],
                                                nhwc=False)
    gb = KW["global_batch"]
    dwav = sl(wav, y, global_batch=gb)
    again = sl(wav, y, global_batch=gb)
    assert again.data_ptr() == dwav.data_ptr() and tuple(sl.spectral_out.shape) == (3,) and sl.spectral_out.dtype == torch.float64
    want, so, _ = run(U, wav.cpu().numpy(), inp["wav_true"], res, 30.0)
    torch.cuda.synchronize()
    assert torch.equal(bits(dwav), bits(want)) and torch.equal(bits(sl.spectral_out), bits(so)) and float(so[0]) > 0 and bool(want.any())
    dpred = sl(wav, y, pred=pred, global_batch=gb)
    by_op = torch.full_like(pred, float("nan"))
    U.ops.istft_features_bwd(pred, want, by_op, nb, nf, inp["n_fft"], inp["win"], inp["hop"])
    torch.cuda.synchronize()
    assert torch.equal(bits(dpred), bits(by_op)) and bool(dpred.any())
    base = torch.ones_like(pred)
    assert sl(wav, y, pred=pred, dpred=base, accumulate=True, global_batch=gb) is base
    assert bool((base[:, :, nb:, :] == 1).all()) and bool((base[:, :, :, nf:] == 1).all()) and not torch.equal(base, torch.ones_like(pred))
    # dwav=: the cotangent is added to the caller's buffer
    mine = dev(base_of(wav.cpu().numpy()))
    assert sl(wav, y, dwav=mine, global_batch=gb) is mine
    acc, _, _ = run(U, wav.cpu().numpy(), inp["wav_true"], res, 30.0, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(mine), bits(acc))
    assert sl(wav, y, global_batch=gb, backward=False) is None
    with pytest.raises(ValueError):
        sl(wav, y, pred=pred, accumulate=True)
