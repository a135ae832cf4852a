"""The room-acoustic figure kernels on the GPU against the NumPy fp64 yardstick (tests/acoustics_ref.py).

Waveforms (acoustics_ref.decay_rows): a spike of 2000 at `peak`, behind it 600 g[n] exp(-(n - peak) / tau), g standard normal,
the row times 2^-15; peaks and tau keep every window edge inside the row.  Every test asserts on the REFERENCE values that they
are finite, that the late-energy share of drr and c50 is >= 1 % and that the regression's condition number is <= 100 (it is <= 8
on these rows), so no comparison is skipped and a thin row fails instead of eating the tolerance.

Tolerances are derived, not measured.

Integer rows (the tail rounded to integers): the samples are exact in fp32 and every energy sum is exact in fp64 in any order,
so the six raw columns must EQUAL the yardstick's.  drr, c50 and ts then differ only by the last bits of log10 and one division:
1e-9 dB absolute on drr / c50, 1e-12 relative on ts.  edt: L[k] is known to a few ulp; the regression is linear in L and its
sums of N <= T terms carry N 2^-53 relative error (9600 2^-53 = 1.1e-12) times the asserted condition number (<= 100): 1e-9
relative.

Uniform rows (the same rows unrounded): n0 and N_fit must be equal - the test asserts on the reference that no 10 S[n] lies
within 1e-9 relative of E_tot, so the count is decided.  Sums of T non-negative terms in any order are within T 2^-53 relative:
1e-11 relative on the energy sums and M1.  The dB figures divide by the late energy, a difference of two such sums that is >= 1 %
of them: 100 x that bound, 1e-8 dB.  edt: 1e-8 relative (L[k] within 1e-10 dB through the same sums, times the condition number).

The accumulate kernel gets the yardstick's own figure rows, so it differs from the yardstick's fold by the rounding of a few
fp64 operations per pair: counts equal, sums 1e-12 relative.
"""
import numpy as np
import pytest
import torch

import acoustics_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FS = 48000.0


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


_ROWS = {}


def rows(T, integer):
    """(waveforms [B, T], reference figures [B, 10]) of a shape, computed once; the reference is checked for the properties the
    tolerances stand on."""
    key = (T, integer)
    if key not in _ROWS:
        B, _, n_pre, n_dir, n_early = next(s for s in A.SHAPES if s[1] == T)
        wav = A.decay_rows("rows", T, A.PEAKS[T][:B], integer)
        figs = []
        for h in wav:
            fig, s, S, L = A.figures(h, n_pre, n_dir, n_early, FS, detail=True)
            assert np.isfinite(fig).all(), "the reference values must be finite: no comparison is skipped"
            assert (fig[1] - fig[2]) >= 0.01 * fig[1] and (fig[1] - fig[3]) >= 0.01 * fig[1], "late-energy share below 1 %"
            assert A.condition(L) <= 100
            assert s + n_early <= T and fig[0] + n_dir < T, "every window edge inside the row"
            if not integer:
                assert np.min(np.abs(10.0 * S[s:] / fig[1] - 1.0)) > 1e-9, "N_fit must be decided"
            figs.append(fig)
        wav.setflags(write=False)
        ref = np.stack(figs)
        ref.setflags(write=False)
        _ROWS[key] = (wav, ref)
    return _ROWS[key]


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).to(DEV)


def check(got, want, what, raw_rel, db_abs, ts_rel, edt_rel):
    got, want = np.asarray(got).reshape(-1, 10), np.asarray(want).reshape(-1, 10)
    assert got.shape == want.shape
    for r in range(len(want)):
        for c, name in enumerate(A.FIGURES):
            g, w = got[r, c], want[r, c]
            err = abs(g - w)
            print(f"{what} row {r} {name}: got {g!r} want {w!r} abs err {err:.3e} rel {err / max(abs(w), 1e-300):.3e}")
            if name in ("n0", "n_fit"):
                assert g == w, (what, r, name)
            elif c < A.RAW:
                assert err <= raw_rel * abs(w), (what, r, name)
            elif name in ("drr", "c50"):
                assert err <= db_abs, (what, r, name)
            else:
                assert err <= (ts_rel if name == "ts" else edt_rel) * abs(w), (what, r, name)


@pytest.mark.parametrize("B,T,n_pre,n_dir,n_early", A.SHAPES)
def test_integer_rows(U, B, T, n_pre, n_dir, n_early):
    wav, ref = rows(T, True)
    got = U.acoustics(dev(wav), None, n_pre, n_dir, n_early, FS)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 1, 10) and got.is_cuda
    check(got.cpu().numpy(), ref, f"integer T={T}", 0.0, 1e-9, 1e-12, 1e-9)
    # the pair in one launch: the same rows, the partner in column 1
    pair = U.acoustics(dev(wav), dev(wav[::-1]), n_pre, n_dir, n_early, FS).cpu()
    assert tuple(pair.shape) == (B, 2, 10)
    assert torch.equal(pair[:, 0], got.cpu()[:, 0]) and torch.equal(pair[:, 1], got.cpu()[:, 0].flip(0))


@pytest.mark.parametrize("B,T,n_pre,n_dir,n_early", A.SHAPES)
def test_uniform_rows(U, B, T, n_pre, n_dir, n_early):
    wav, ref = rows(T, False)
    got = U.acoustics(dev(wav), None, n_pre, n_dir, n_early, FS)
    check(got.cpu().numpy(), ref, f"uniform T={T}", 1e-11, 1e-8, 1e-11, 1e-8)


def test_rows_do_not_depend_on_the_batch_and_repeat_bit_for_bit(U):
    bits = lambda t: t.cpu().view(torch.int64)
    for T_ in (9600, 257):                                              # 257: rows 1 and up start off a 16-byte boundary
        Bk, _, a, b, c = next(s for s in A.SHAPES if s[1] == T_)
        wav = dev(rows(T_, False)[0])
        full = bits(U.acoustics(wav, None, a, b, c, FS))
        assert torch.equal(bits(U.acoustics(wav, None, a, b, c, FS)), full)                                  # twice
        alone = torch.cat([bits(U.acoustics(wav[i:i + 1], None, a, b, c, FS)) for i in range(Bk)])          # one by one
        assert torch.equal(alone, full)
        rev = bits(U.acoustics(wav.flip(0).contiguous(), None, a, b, c, FS))                                # reversed order
        assert torch.equal(rev.flip(0), full)
        pair = bits(U.acoustics(wav, wav.flip(0).contiguous(), a, b, c, FS))                                # as either partner
        assert torch.equal(pair[:, 0], full[:, 0]) and torch.equal(pair[:, 1].flip(0), full[:, 0])
        # the same rows four bytes off a 16-byte boundary: the scalar fetch must give the bits of the 128-bit one
        off = torch.empty((Bk * T_ + 1,), dtype=torch.float32, device=DEV)[1:].view(Bk, T_)
        off.copy_(wav)
        assert off.data_ptr() % 16 == 4 and off.is_contiguous()
        assert torch.equal(bits(U.acoustics(off, None, a, b, c, FS)), full)


def test_degenerate_rows_on_the_device(U):
    """The IEEE results of the definitions (tests/test_acoustics.py asserts their values on the yardstick)."""
    T = 50
    wav = np.zeros((5, T), np.float32)
    wav[1, 0] = 1.0
    wav[2, 49] = -2.0
    wav[3, [20, 40]] = (-0.75, 0.75)
    wav[3, 41:] = 2.0 ** -7
    wav[4] = A.decay_rows("degenerate", T, ((4, 12.0),))[0]
    got = U.acoustics(dev(wav), None, 5, 5, 20, FS).cpu().numpy()[:, 0]
    want = A.batch_figures(wav, n_pre=5, n_dir=5, n_early=20, fs=FS)
    assert np.array_equal(got[:, :A.RAW], want[:, :A.RAW])
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert np.isnan(got[0, 6:]).all() and got[1, 6] == np.inf and np.isnan(got[1, 9]) and got[2, 9] == -np.inf and got[3, 0] == 20
    fin = np.isfinite(want)
    assert np.allclose(got[fin], want[fin], rtol=1e-9, atol=0)
    one = U.acoustics(dev(np.array([[3.0]], np.float32))).cpu().numpy()[0, 0]                               # T = 1
    assert list(one[:6]) == [0, 9, 9, 9, 0, 1] and one[6] == np.inf and one[8] == 0 and np.isnan(one[9])


def test_accumulate_per_room(U):
    """Three successive batches into one acc; rooms include -1 and a stray index, room 2 stays empty; the second batch holds an
    all-zero prediction and a prediction whose peak is the last sample: excluded figure by figure, not pair by pair."""
    T, G, (n_pre, n_dir, n_early) = 257, 4, (5, 8, 40)
    cases = ((3, 60.0), (20, 45.0), (9, 50.0), (14, 70.0), (30, 40.0))
    acc = torch.zeros((G + 1, 20), dtype=torch.float64, device=DEV)
    figs, groups, errs = [], [], []
    for k, B in enumerate((3, 5, 2)):
        true = A.decay_rows(f"acc/true{k}", T, cases[:B])
        pred = A.decay_rows(f"acc/pred{k}", T, [(p + 2 + k, tau * 1.2) for p, tau in cases[:B]])
        if k == 1:
            pred[1] = 0.0
            pred[3] = 0.0
            pred[3, T - 1] = 0.5
        fig = np.stack([A.batch_figures(pred, n_pre=n_pre, n_dir=n_dir, n_early=n_early, fs=FS),
                        A.batch_figures(true, n_pre=n_pre, n_dir=n_dir, n_early=n_early, fs=FS)], axis=1)
        g = np.array([[0, 1, 3], [3, 0, -1, 1, 9], [1, 3]][k], dtype=np.int32)
        err = torch.full((B, 5), -7.0, dtype=torch.float64, device=DEV)
        U.ops.acoustic_accumulate(dev(fig), dev(g), acc, FS, err=err)
        figs.append(fig); groups.append(g); errs.append(err.cpu().numpy())
    fig, g, err = np.concatenate(figs), np.concatenate(groups), np.concatenate(errs)
    want_err, want_acc = A.fold(fig, g, G, FS)
    got_acc = acc.cpu().numpy()
    cnt, want_cnt = got_acc[:, 3::4], want_acc[:, 3::4]
    print("counts\n", cnt, "\nwant\n", want_cnt)
    assert np.array_equal(cnt, want_cnt)
    assert want_cnt[0].tolist() == [10, 8, 8, 9, 8] and (want_cnt[3] == 0).all() and want_cnt[1:].sum(axis=0).tolist() == [8, 6, 6, 7, 6]
    assert np.array_equal(np.isnan(err), np.isnan(want_err)) and np.array_equal(np.isinf(err), np.isinf(want_err))
    fin = np.isfinite(want_err)
    assert np.all(np.abs(err[fin] - want_err[fin]) <= 1e-12 * np.abs(want_err[fin]))
    assert np.isfinite(want_acc).all()
    for r in range(G + 1):
        for c in range(20):
            print(f"acc[{r}][{c}]: got {got_acc[r, c]!r} want {want_acc[r, c]!r}")
            assert abs(got_acc[r, c] - want_acc[r, c]) <= 1e-12 * abs(want_acc[r, c]), (r, c)
    # without err, and with G = 0 (the global row alone)
    only = torch.zeros((1, 20), dtype=torch.float64, device=DEV)
    U.ops.acoustic_accumulate(dev(figs[1]), dev(groups[1]), only, FS)
    assert np.array_equal(only.cpu().numpy()[0, 3::4], A.fold(figs[1], groups[1], 0, FS)[1][0, 3::4])


class _Stub:
    """A 'model' with the reference's call shape that returns prepared predictions, NHWC, batch after batch."""

    def __init__(self, preds):
        self.preds, self.calls = preds, 0

    def model(self, inputs, training=False):
        self.calls += 1
        return self.preds[(self.calls - 1) % len(self.preds)]


def test_evaluator_with_and_without_acoustics(U):
    """Evaluator(acoustics=True) behind a stub model at the real size: the seven existing figures are those of
    Evaluator(acoustics=False) bit for bit, and the "acoustics" block is the yardstick's fold of the figures of the waveforms
    PostProcess produced (read back here) and the true waveforms.  The waveforms are arbitrary fp32, so the tolerances are the
    uniform rows': the yardstick's means are held to 1e-8 dB (drr, c50), 1e-11 relative (ts), 1e-8 relative (edt error, through
    edt on either side; the error is a difference of two such values divided by a third, asserted not to cancel below 1 % of them)."""
    H, W, B, T = 144, 160, 4, 9600
    pre, post = U.features.PreProcess(), U.features.PostProcess()
    cases = A.PEAKS[9600][:B]
    preds, batches = [], []
    for k in range(2):
        wav_true = dev(A.decay_rows(f"ev/true{k}", T, cases, integer=False))
        wav_model = dev(A.decay_rows(f"ev/pred{k}", T, [(p + 5 * (k + 1), tau * (1.1 + 0.1 * k)) for p, tau in cases], integer=False))
        spec_out = pre(wav_true)                                                                 # NCHW
        preds.append(pre(wav_model).permute(0, 2, 3, 1).contiguous())                            # the stub's prediction, NHWC
        emb = torch.zeros((B, 2, 16), dtype=torch.int32, device=DEV)
        room = [["ShoeBoxRoom", "LargeMeetingRoom", "ShoeBoxRoom", "Cellar"], ["SmallMeetingRoom", "ShoeBoxRoom", "LargeMeetingRoom",
                                                                               "LargeMeetingRoom"]][k]
        batches.append((spec_out.clone(), emb, spec_out, wav_true, room))
    res = {}
    for on in (True, False):
        ev = U.Evaluator(_Stub(preds), acoustics=on)
        for b in batches:
            ev.update(*b)
        res[on] = ev.result()
    assert "acoustics" not in res[False] and sorted(res[True]) == sorted(list(res[False]) + ["acoustics"])
    for m in ("rooms", "n") + U.evaluate.METRICS:
        assert repr(res[True][m]) == repr(res[False][m]), m                                     # repr: NaN of the empty rooms included

    figs, groups = [], []
    for k, b in enumerate(batches):
        wav_pred = post.post_process(preds[k]).cpu().numpy()
        pair = []
        for wav in (wav_pred, b[3].cpu().numpy()):
            rows_ = []
            for h in wav:
                f, s, S, L = A.figures(h, fs=FS, detail=True)
                assert np.isfinite(f).all() and f[9] > 0
                assert (f[1] - f[2]) >= 0.01 * f[1] and (f[1] - f[3]) >= 0.01 * f[1], "late-energy share below 1 %"
                assert A.condition(L) <= 100 and np.min(np.abs(10.0 * S[s:] / f[1] - 1.0)) > 1e-9
                rows_.append(f)
            pair.append(np.stack(rows_))
        figs.append(np.stack(pair, axis=1))
        groups += [U.evaluate.ROOMS.index(r) if r in U.evaluate.ROOMS else -1 for r in b[4]]
    fig = np.concatenate(figs)
    edt_p, edt_t = fig[:, 0, 9], fig[:, 1, 9]
    assert np.all(np.abs(edt_p - edt_t) >= 0.01 * edt_t) and np.all(edt_p <= 2 * edt_t), "the edt error must not be a cancellation"
    want = A.result_block(A.fold(fig, groups, len(U.evaluate.ROOMS), FS)[1])
    got = res[True]["acoustics"]
    assert list(got) == list(A.ERRORS)
    assert want["toa_ms"]["n"] == [8, 0, 3, 0, 3, 1]
    # a figure's value v is held to tol(v) as in the uniform rows (n0 equal: toa differs by the rounding of two operations); a mean
    # of values to the mean of their tolerances; an error |p - t| to tol(p) + tol(t).  edt_pct = 100 |p - t| / t with |p - t| >= t /
    # 100 and p <= 2 t asserted above: relative (1e-8 p + 1e-8 t) / |p - t| + 1e-8 <= 3.01e-6.
    tol = {"toa_ms": lambda v: 1e-12 * abs(v), "drr_db": lambda v: 1e-8, "c50_db": lambda v: 1e-8, "ts_ms": lambda v: 1e-11 * abs(v),
           "edt_pct": lambda v: 1e-8 * abs(v)}
    for name in A.ERRORS:
        assert got[name]["n"] == want[name]["n"] and all(isinstance(v, int) for v in got[name]["n"]), name
        for key in ("err", "pred", "true"):
            assert all(isinstance(v, float) for v in got[name][key])
            for r, (g, w) in enumerate(zip(got[name][key], want[name][key])):
                print(f"{name} {key} row {r}: got {g!r} want {w!r}")
                if want[name]["n"][r] == 0:
                    assert np.isnan(g) and np.isnan(w)
                elif key != "err":
                    assert abs(g - w) <= tol[name](w), (name, key, r)
                elif name == "edt_pct":
                    assert abs(g - w) <= 3.1e-6 * abs(w), (name, key, r)
                else:
                    assert abs(g - w) <= tol[name](want[name]["pred"][r]) + tol[name](want[name]["true"][r]), (name, key, r)
    assert res[True]["timing"]["loss_s"] > 0
