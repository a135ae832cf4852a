"""GPU tests of the FFT form of the multi-resolution STFT loss (csrc/spectralloss_fft.hip) against the fp64 truth of
tests/spectral_loss_ref.py, with the tolerances of tests/spectral_loss_fft_ref.py: per row e(kernel) <= 4 e(complex64 restatement) +
2^-22 with e(v) = max_t |v - dwav64| / max_t |dwav64|, and the scalars to a relative 64 log2(N_max) 2^-24 - neither measured on a
kernel.  Every output is carved out of a larger buffer with a canary either side and prefilled with NaN, so an element the kernels
leave out shows; the workspace is exactly the advertised size in front of a canary."""
import numpy as np
import pytest
import torch

import spectral_loss_fft_ref as FR
from test_spectral_loss_gpu import CANARY, DEV, LOSS0, Guarded, base_of, bits, dev  # noqa: F401  (the guarded buffers of the DFT form's test)

pytestmark = pytest.mark.gpu
KW = FR.KW


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


def run(U, yp, yt, res, floor_db, backward=True, accumulate=False, exact_ws=True):
    """one call of ops.spectral_loss_fft -> (dwav: the kernel's, or the untouched NaN prefill without backward; spectral_out; loss_out),
    with exactly the advertised workspace in front of a canary"""
    B, T = yp.shape
    dw = Guarded((B, T), fill=dev(base_of(yp)) if accumulate else float("nan"))
    so = Guarded((3,), torch.float64)
    lo = torch.full((4,), LOSS0, dtype=torch.float32, device=DEV)
    need = U.ops.spectral_loss_fft_ws_bytes(B, T, res)
    assert need > 0 and need % 8 == 0
    big = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    ws = U.ops.Workspace(DEV)
    if exact_ws:
        ws.buf = big[:need]
    U.ops.spectral_loss_fft(dev(yp), dev(yt), so.out, ws, res, floor_db=floor_db, sc_weight=KW["sc_weight"], log_weight=KW["log_weight"],
                            weight=KW["weight"], global_batch=KW["global_batch"], dwav=dw.out if backward else None, accumulate=accumulate,
                            loss_out=lo)
    out = dw.result(), so.result(), lo
    if exact_ws:
        assert ws.buf.data_ptr() == big.data_ptr() and bool((big[need:] == 0xA5).all())
    return out


def check(got_dwav, got_out, got_lo, T, res, floor_db, B, what, base=None):
    tr, rs = FR.truth(T, res, floor_db), FR.restated(T, res, floor_db)
    truth = tr["dwav"][:B]
    got = got_dwav.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()                                                     # a NaN left over: an element not written
    peak = np.abs(truth).max(axis=1)
    e_rs = FR.rel_err(rs["dwav"][:B], truth)
    tol = 4.0 * e_rs + 2.0 ** -22
    if base is None:
        e = FR.rel_err(got, truth)
        print(f"{what}: e(kernel) {e} e(restatement) {e_rs} allowed {tol}")
        assert (e <= tol).all()
    else:                                                                             # (float)((double) base + g): one more rounding, of the sum
        want = base.astype(np.float64) + truth
        err = np.abs(got - want)
        allowed = (tol * peak)[:, None] + 2.0 ** -24 * np.abs(want)
        print(f"{what}: largest err / allowance {float((err / allowed).max()):.3f}")
        assert (err <= allowed).all()
    want_out, want_loss = FR.truth_scalars(tr, B)
    o = got_out.cpu().numpy()
    sb = FR.scalar_bound(res)
    print(f"  spectral_out {o} fp64 {want_out} relative {np.abs(o[:2] - want_out[:2]) / want_out[:2]} of {sb:.3e}")
    assert (np.abs(o[:2] - want_out[:2]) <= sb * want_out[:2]).all() and o[2] == want_out[2]
    want_lo = LOSS0 + want_loss                                                       # the fp32 term, then one fp32 addition
    assert abs(float(got_lo[0]) - want_lo) <= sb * want_loss + 2.0 ** -24 * (want_loss + want_lo)
    assert bool((got_lo[1:] == LOSS0).all())


@pytest.mark.parametrize("B", FR.BATCHES)
@pytest.mark.parametrize("T,res", FR.CASES, ids=FR.IDS)
def test_every_element_against_fp64(U, T, res, B):
    yp, yt = (np.ascontiguousarray(a[:B]) for a in FR.inputs(T))
    dw, so, lo = run(U, yp, yt, res, 60.0)
    check(dw, so, lo, T, res, 60.0, B, f"T {T} {res} B {B}")
    # a second run: the same bits
    dw2, so2, lo2 = run(U, yp, yt, res, 60.0, exact_ws=False)
    assert torch.equal(bits(dw2), bits(dw)) and torch.equal(bits(so2), bits(so)) and torch.equal(bits(lo2), bits(lo))
    # the loss alone: the same sums, and no dwav element touched (the NaN prefill stays)
    dw3, so3, lo3 = run(U, yp, yt, res, 60.0, backward=False)
    assert bool(torch.isnan(dw3).all()) and torch.equal(bits(so3), bits(so)) and torch.equal(bits(lo3), bits(lo))
    # accumulate: (float)((double) base + g), the same sums
    dw4, so4, lo4 = run(U, yp, yt, res, 60.0, accumulate=True)
    check(dw4, so4, lo4, T, res, 60.0, B, f"T {T} {res} B {B} accumulate", base=base_of(yp))
    assert torch.equal(bits(so4), bits(so))


@pytest.mark.parametrize("B", FR.BATCHES)
@pytest.mark.parametrize("T,res", FR.CASES, ids=FR.IDS)
def test_floor_30(U, T, res, B):
    yp, yt = (np.ascontiguousarray(a[:B]) for a in FR.inputs(T))
    dw, so, lo = run(U, yp, yt, res, 30.0)
    check(dw, so, lo, T, res, 30.0, B, f"T {T} {res} B {B} floor 30")
    dw4, so4, lo4 = run(U, yp, yt, res, 30.0, accumulate=True)
    check(dw4, so4, lo4, T, res, 30.0, B, f"T {T} {res} B {B} floor 30 accumulate", base=base_of(yp))


@pytest.mark.parametrize("T,res", FR.CASES, ids=FR.IDS)
def test_a_rows_bits_depend_neither_on_the_batch_nor_on_its_place(U, T, res):
    yp, yt = FR.inputs(T)
    dw, _, _ = run(U, yp, yt, res, 60.0)
    for rows in ((1,), (2, 0, 2)):
        sel = list(rows)
        d, so, _ = run(U, np.ascontiguousarray(yp[sel]), np.ascontiguousarray(yt[sel]), res, 60.0)      # the same inv_global_batch
        for i, r in enumerate(rows):
            assert torch.equal(bits(d[i]), bits(dw[r])), (rows, i)
        assert float(so[2]) == len(rows)


@pytest.mark.parametrize("T,res", [FR.CASES[1], FR.CASES[3], FR.MULTI[0]], ids=[FR.IDS[1], FR.IDS[3], "default"])
def test_a_zero_target_row_and_a_zero_prediction_row(U, T, res):
    """a silent target counts nothing - zeros in its row of dwav, nothing in any sum; a silent prediction sits on the floor with a
    gradient of exact zeros (G carries the factor X^), but counts"""
    import spectral_loss_ref as SR
    yp, yt = (np.array(a) for a in FR.inputs(T))
    yt[1] = 0.0
    yp[2] = 0.0
    sc, lm, ok = SR.terms(torch.from_numpy(yp).double(), torch.from_numpy(yt).double(), res, 60.0)
    assert list(ok.numpy()) == [True, False, True]
    dw, so, lo = run(U, yp, yt, res, 60.0)
    want = np.array([float(sc.mean(dim=1).sum()), float(lm.mean(dim=1).sum())])
    o = so.cpu().numpy()
    assert (np.abs(o[:2] - want) <= FR.scalar_bound(res) * want).all() and o[2] == 2.0
    assert not bool(dw[1].any()) and not bool(dw[2].any()) and bool(dw[0].any())
    one, _, _ = run(U, yp[:1], yt[:1], res, 60.0)
    assert torch.equal(bits(one[0]), bits(dw[0]))
    full, _, _ = run(U, *FR.inputs(T), res, 60.0)                                      # row 0 is what it is among audible rows
    assert torch.equal(bits(full[0]), bits(dw[0]))
    # accumulate leaves the silent rows' base as it is
    acc, _, _ = run(U, yp, yt, res, 60.0, accumulate=True)
    assert torch.equal(bits(acc[1:]), bits(dev(base_of(yp))[1:]))
    # every target silent: all sums zero, loss_out unchanged
    dwz, soz, loz = run(U, yp, np.zeros_like(yt), res, 60.0)
    assert not bool(dwz.any()) and not bool(soz.any()) and float(loz[0]) == LOSS0


def test_spectral_loss_object(U):
    """SpectralLoss(method="fft") on its own: keeps its buffers, returns dwav, equals the op; with pred it returns dpred = the
    vector-Jacobian product of its dwav bit for bit; dwav= adds; backward=False returns None; the default method is the DFT form"""
    import wave_loss_ref as WR
    inp = WR.inputs("oddwin", False)
    nb, nf = inp["des_shape"]
    geo = dict(des_shape=(nb, nf), n_fft=inp["n_fft"], win_length=inp["win"], hop_length=inp["hop"])
    T = inp["hop"] * (nf - 1)
    res = tuple(r for r in ((128, 64, 32), (256, 100, 37), (512, 256, 128)) if r[0] // 2 + 1 <= T)
    assert len(res) >= 2                                                              # T = 203, odd: rows off 16 bytes
    kw = dict(weight=KW["weight"], resolutions=res, sc_weight=KW["sc_weight"], log_weight=KW["log_weight"], floor_db=30.0, **geo)
    sl = U.SpectralLoss(method="fft", **kw)
    assert sl.T == T and sl.method == "fft" and U.SpectralLoss(**kw).method == "dft"
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
    # the DFT form on the same data: another kernel, the same quantity
    ref = U.SpectralLoss(**kw)(wav, y, global_batch=gb)
    torch.cuda.synchronize()
    assert not torch.equal(bits(ref), bits(dwav)) and float((ref - dwav).abs().max()) <= 1e-3 * float(ref.abs().max())
    dpred = sl(wav, y, pred=pred, global_batch=gb)
    by_op = torch.full_like(pred, float("nan"))
    U.ops.istft_features_bwd(pred, want, by_op, nb, nf, inp["n_fft"], inp["win"], inp["hop"])
    torch.cuda.synchronize()
    assert torch.equal(bits(dpred), bits(by_op)) and bool(dpred.any())
    mine = dev(base_of(wav.cpu().numpy()))
    assert sl(wav, y, dwav=mine, global_batch=gb) is mine
    acc, _, _ = run(U, wav.cpu().numpy(), inp["wav_true"], res, 30.0, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(mine), bits(acc))
    assert sl(wav, y, global_batch=gb, backward=False) is None
    with pytest.raises(ValueError):
        sl(wav, y, pred=pred, accumulate=True)


@pytest.mark.parametrize("others", [False, True], ids=["spectral-alone", "with-wave-and-decay"])
def test_a_graph_step_equals_an_eager_step(U, others):
    """Trainer(spectral_loss=SpectralLoss(method="fft")): steps replayed as a HIP graph are the steps issued launch by launch, bit for
    bit"""
    from test_decay_loss_step_gpu import _batches, _decay, _wave
    from test_wave_loss_step_gpu import GEO, _engine
    res = ((128, 64, 32), (256, 128, 32))
    data = _batches(2)
    out = []
    for graph in (True, False):
        eng = _engine(U, "unet", "bf16")
        sl = U.SpectralLoss(weight=0.05, resolutions=res, sc_weight=0.8, log_weight=1.3, floor_db=40.0, method="fft", **GEO)
        tr = U.Trainer(eng, lr=1e-3, graph=graph, wave_loss=_wave(U) if others else None, decay_loss=_decay(U) if others else None,
                       spectral_loss=sl)
        if not graph:
            eng.use_device_counters(True)          # the same arithmetic by construction: the step's scalars in device memory for both
        losses = [tr.step(a, e, b, wav_true=wav, return_loss=True) for a, e, b, wav in data]
        torch.cuda.synchronize()
        if graph:
            assert tr.use_graph and set(tr._graphs) == {True}
        out.append((losses, eng.theta.clone(), tr.spectral_loss.spectral_out.clone()))
    g, h = out
    assert g[0] == h[0] and torch.equal(g[1], h[1]) and torch.equal(g[2], h[2]) and float(g[2][0]) > 0 and float(g[2][2]) == 2.0


def test_train_script_with_the_fft_method(U, tmp_path, monkeypatch):
    """scripts/train.py --spectral-loss W --spectral-method fft on the generated tree: fit records the two terms for the training and the
    validation pass; a resolution the FFT form does not take is refused at the command line"""
    import json
    import os
    import dataset_tree as DT
    from test_dataset_gpu import run_script
    root = str(tmp_path / "rir")
    os.makedirs(root)
    DT.make_tree(root)
    out = str(tmp_path / "ckpt")
    common = ["--dataset", root, DT.NAME, "--name", "unet", "--filters", 8, "--rooms", "HemiAnechoicRoom", "SmallMeetingRoom", "--no-debug",
              "--batch", 4, "--lr", 1e-4, "--out", out, "--epochs", 1, "--spectral-loss", 0.01, "--spectral-floor-db", 45,
              "--spectral-method", "fft"]
    run_script(monkeypatch, "train", ["--spectral-resolutions", "128:64:32,512:256:128"] + common)
    hist = json.load(open(os.path.join(out, "history.json")))
    assert [h["epoch"] for h in hist] == [1]
    for h in hist:
        assert all(np.isfinite(h[k]) and h[k] > 0 for k in ("train_loss", "val_loss", "train_sc", "val_sc", "train_logmag", "val_logmag"))
    with pytest.raises(SystemExit, match=r'--spectral-resolutions.*method="dft"'):
        run_script(monkeypatch, "train", ["--spectral-resolutions", "64:64:16"] + common)
