"""Scoring of generated impulse responses on the GPU against the NumPy fp64 yardstick (tests/eval_ref.py).

Tolerances are derived, not measured.  Kernel and yardstick start from the same fp32 values and both accumulate in fp64; they
differ in summation order and in the last bits of the cosine.  A sum of n non-negative fp64 terms in any order is within
n * 2^-53 relative of exact; the largest n is 2 * 144 * 160 = 46 080 -> 5.1e-12.  Hence 1e-10 relative on the MSE figures and
the phase figure (20 x that bound, covering the cosine and the final division), 1e-10 absolute on `phase` where it is below
1e-6 (cancellation in 1 - cos), and 1e-8 dB absolute on the misalignments (20 log10 of a ratio known to 1e-10 moves by
8.7e-10 dB)."""
import numpy as np
import pytest
import torch

import eval_ref
from oracle import detrand

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MSE_COLS, PHASE_COL, DB_COLS = (0, 1, 4, 5), 2, (3, 6)


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def make_inputs(name, B, H, W, T):
    """NHWC fp32 features uniform in [0, 1) with the padding rows / columns of the target zero (the STFT core is 129 x 151 of
    144 x 160: the same fractions here), zero-mean waveforms of amplitude 1e-2: no norm in a denominator is near zero."""
    r0, c0 = int(np.ceil(0.896 * H)), int(np.ceil(0.944 * W))
    d = {k: detrand.uniform(f"eval/{name}/{k}", (B, H, W, 2)) for k in ("pred", "target", "spec_in")}
    d["target"][:, r0:, :, :] = 0.0
    d["target"][:, :, c0:, :] = 0.0
    d["wav_pred"] = detrand.uniform(f"eval/{name}/wp", (B, T), -1e-2, 1e-2)
    d["wav_true"] = detrand.uniform(f"eval/{name}/wt", (B, T), -1e-2, 1e-2)
    return d


def dev(a, nchw=False):
    t = torch.tensor(np.ascontiguousarray(a)).to(DEV)
    return t.permute(0, 3, 1, 2).contiguous() if nchw else t


def check_rows(got, want, what=""):
    """got / want [..., 7] fp64: the derived tolerances, every figure printed before it is asserted."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1, 7), np.asarray(want, dtype=np.float64).reshape(-1, 7)
    assert got.shape == want.shape
    assert np.isfinite(want).all(), "the reference values must be finite: no comparison is skipped"
    for r in range(len(want)):
        for c in range(7):
            g, w = got[r, c], want[r, c]
            err = abs(g - w)
            print(f"{what} row {r} {eval_ref.METRICS[c]}: got {g!r} want {w!r} abs err {err:.3e} rel {err / max(abs(w), 1e-300):.3e}")
            if c in DB_COLS:
                assert err <= 1e-8, (what, r, c, g, w)
            elif c == PHASE_COL and abs(w) < 1e-6:
                assert err <= 1e-10, (what, r, c, g, w)
            else:
                assert err <= 1e-10 * abs(w), (what, r, c, g, w)


@pytest.mark.parametrize("H,W,T,n50", [(144, 160, 9600, 2400), (9, 7, 101, 300)])
@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("diff", [False, True])
def test_score_matches_the_yardstick(U, H, W, T, n50, nchw, diff):
    B = 5
    d = make_inputs("score", B, H, W, T)
    want = eval_ref.batch_metrics(d["pred"], d["target"], d["wav_pred"], d["wav_true"], d["spec_in"] if diff else None, n50)
    got = U.score(dev(d["pred"], nchw), dev(d["target"], nchw), dev(d["wav_pred"]), dev(d["wav_true"]),
                  phase_ref=dev(d["spec_in"], nchw) if diff else None, n50=n50)
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 7) and got.is_cuda
    check_rows(got.cpu().numpy(), want, f"{H}x{W} nchw={nchw} diff={diff}")


def test_without_waveforms_the_waveform_figures_are_nan(U):
    d = make_inputs("score", 5, 144, 160, 9600)
    full = U.score(dev(d["pred"]), dev(d["target"]), dev(d["wav_pred"]), dev(d["wav_true"])).cpu()
    bare = U.score(dev(d["pred"]), dev(d["target"])).cpu()
    assert torch.isnan(bare[:, 4:]).all()
    assert torch.equal(bare[:, :4], full[:, :4])                       # bit for bit
    with pytest.raises(ValueError):
        U.score(dev(d["pred"]), dev(d["target"]), wav_pred=dev(d["wav_pred"]))


def test_scoring_is_deterministic_and_batch_independent(U):
    B = 8
    d = make_inputs("det", B, 144, 160, 9600)
    p, t, r = dev(d["pred"], True), dev(d["target"], True), dev(d["spec_in"], True)
    wp, wt = dev(d["wav_pred"]), dev(d["wav_true"])
    a = U.score(p, t, wp, wt, phase_ref=r).cpu()
    b = U.score(p, t, wp, wt, phase_ref=r).cpu()
    assert torch.equal(a, b)
    single = torch.cat([U.score(p[i:i + 1], t[i:i + 1], wp[i:i + 1], wt[i:i + 1], phase_ref=r[i:i + 1]) for i in range(B)]).cpu()
    assert torch.equal(single, a)
    # an odd plane size takes the scalar fetch; a slice of it starts off a 16-byte boundary and must still give the same rows
    d = make_inputs("det-odd", 3, 9, 7, 101)
    p, t, wp, wt = dev(d["pred"], True), dev(d["target"], True), dev(d["wav_pred"]), dev(d["wav_true"])
    a = U.score(p, t, wp, wt, n50=50).cpu()
    single = torch.cat([U.score(p[i:i + 1], t[i:i + 1], wp[i:i + 1], wt[i:i + 1], n50=50) for i in range(3)]).cpu()
    assert torch.equal(single, a)


def test_degenerate_sample_follows_ieee_and_leaves_its_neighbours_alone(U):
    d = make_inputs("degenerate", 3, 9, 7, 101)
    clean = U.score(dev(d["pred"]), dev(d["target"]), dev(d["wav_pred"]), dev(d["wav_true"]), n50=300).cpu()
    d["target"][1] = 0.0                                               # |target0| = 0, |pred0 - target0| > 0 -> +inf dB
    got = U.score(dev(d["pred"]), dev(d["target"]), dev(d["wav_pred"]), dev(d["wav_true"]), n50=300).cpu()
    assert got[1, 3] == float("inf")
    assert torch.isfinite(got[1, [0, 1, 2, 4, 5, 6]]).all()
    assert torch.equal(got[[0, 2]], clean[[0, 2]])
    d["pred"][1, :, :, 0] = 0.0                                        # both zero -> NaN; zero numerator alone -> -inf
    d["pred"][2, :, :, 0] = d["target"][2, :, :, 0]
    got = U.score(dev(d["pred"]), dev(d["target"]), dev(d["wav_pred"]), dev(d["wav_true"]), n50=300).cpu()
    assert torch.isnan(got[1, 3]) and got[2, 3] == float("-inf") and got[2, 1] == 0
    assert torch.equal(got[0], clean[0])


def test_accumulation_per_room(U):
    """Three batches of different sizes, rooms drawn from detrand with one room (2) never drawn, one stray index: result()
    equals the yardstick's group means, counts exact, the stray sample only in Global, the empty room NaN."""
    H, W, T, G = 24, 20, 200, 5
    ev = U.Evaluator(None, n50=120)
    rows, groups = [], []
    for k, B in enumerate((4, 7, 3)):
        d = make_inputs(f"acc{k}", B, H, W, T)
        g = detrand.randint(f"eval/acc{k}/rooms", (B,), 0, G - 1)
        g = np.where(g >= 2, g + 1, g)                                 # rooms 0, 1, 3, 4
        if k == 1:
            g[3] = 11                                                  # matches no room
        rows.append(eval_ref.batch_metrics(d["pred"], d["target"], d["wav_pred"], d["wav_true"], None, 120))
        groups.append(g)
        room = torch.tensor(g).to(DEV) if k != 2 else [U.evaluate.ROOMS[i] for i in g]        # indices or names
        ev.update_scored(dev(d["pred"]), dev(d["spec_in"]), dev(d["target"]), dev(d["wav_pred"]), dev(d["wav_true"]), room)
    rows, groups = np.concatenate(rows), np.concatenate(groups)
    assert np.isfinite(rows).all()
    means, counts = eval_ref.group_means(rows, groups, G)
    res = ev.result()
    assert res["rooms"] == list(U.evaluate.ROOMS)
    assert counts[3] == 0 and all(counts[r] > 0 for r in (1, 2, 4, 5))           # every other room is drawn: no vacuous comparison
    assert res["n"] == counts.tolist() and res["n"][0] == 14 and res["n"][3] == 0 and sum(res["n"][1:]) == 13
    for c, name in enumerate(eval_ref.METRICS):
        got = np.array(res[name])
        assert all(isinstance(v, float) for v in res[name])
        assert np.isnan(got[3]) and np.isnan(means[3, c])
        for r in (0, 1, 2, 4, 5):
            print(f"{name} row {r}: got {got[r]!r} want {means[r, c]!r}")
            assert abs(got[r] - means[r, c]) <= 1e-10 * abs(means[r, c]), (name, r)
    tm = res["timing"]
    assert tm["n_batches"] == 3 and tm["loss_s"] > 0 and np.isnan(tm["inference_s"]) and np.isnan(tm["postprocess_s"])


@pytest.mark.parametrize("diff_gen", [False, True])
def test_end_to_end_generate_reconstruct_score(U, diff_gen):
    """Evaluator.update on a small UNet equals the yardstick applied to model.model(..., training=False) and
    PostProcess.post_process outputs fetched separately; under diff_gen mse_spec comes from the raw prediction, phase and
    waveform from the sum."""
    from oracle import torch_ref as R
    H, W, F0, B, T = 32, 48, 4, 2, 320
    geo = dict(n_fft=32, win_length=16, hop_length=8, des_shape=(17, 41))
    cfg = R.Config(H, W, F0, 3)
    m = U.UNet((H, W, 2), (2, 16), number_filters_0=F0, kernels=3, batch_size=B, device=DEV, dropout=False)
    m.engine.load_keras_params(R.init_params(cfg, randomize_all=True, dtype=np.float64))
    ev = U.Evaluator(m, diff_gen=diff_gen, n50=80, **geo)
    post = U.features.PostProcess()
    rooms = (["ShoeBoxRoom", "LargeMeetingRoom"], ["ShoeBoxRoom", "SmallMeetingRoom"])
    rows, groups = [], []
    for k in range(2):
        spec_in, emb, spec_out = R.synthetic_batch(cfg, B, seed_name=f"eval-e2e/{k}")           # NCHW
        wav_true = detrand.uniform(f"eval-e2e/{k}/wt", (B, T), -1e-2, 1e-2)
        x, e, y = torch.tensor(spec_in).to(DEV), torch.tensor(emb).to(DEV), torch.tensor(spec_out).to(DEV)
        x_nhwc = x.permute(0, 2, 3, 1).contiguous()
        ev.update(x_nhwc if k == 0 else x, e, y.permute(0, 2, 3, 1) if k == 0 else y, torch.tensor(wav_true).to(DEV), rooms[k])
        with torch.no_grad():
            pred = m.model([x_nhwc, e], training=False).clone()                                  # NHWC
        feat = pred.clone()
        if diff_gen:
            feat[..., 1] = pred[..., 1] + x_nhwc[..., 1]
        wav_pred = post.post_process(feat, **geo).cpu().numpy()
        pred_np, in_np = pred.cpu().numpy(), x_nhwc.cpu().numpy()
        if diff_gen:
            assert np.array_equal(feat[..., 1].cpu().numpy(), np.stack([eval_ref.scored_phase(pred_np[j], in_np[j]) for j in range(B)]))
        rows.append(eval_ref.batch_metrics(pred_np, np.transpose(spec_out, (0, 2, 3, 1)), wav_pred, wav_true,
                                           in_np if diff_gen else None, 80))
        groups += [U.evaluate.ROOMS.index(r) for r in rooms[k]]
    rows = np.concatenate(rows)
    assert np.isfinite(rows).all()
    means, counts = eval_ref.group_means(rows, groups, 5)
    res = ev.result()
    assert res["n"] == counts.tolist() == [4, 0, 1, 0, 2, 1]
    filled = [0, 2, 4, 5]
    check_rows(np.array([[res[n][r] for n in eval_ref.METRICS] for r in filled]), means[filled], f"e2e diff_gen={diff_gen}")
    for n in eval_ref.METRICS:
        assert np.isnan(res[n][1]) and np.isnan(res[n][3])
    tm = res["timing"]
    assert tm["n_batches"] == 2 and tm["batch_size"] == B
    assert tm["inference_s"] > 0 and tm["postprocess_s"] > 0 and tm["loss_s"] > 0 and tm["total_s"] > 0


def test_update_scored_does_not_synchronise_with_the_host(U):
    """From the second call on, update_scored on preallocated inputs runs under torch's sync debug mode "error"."""
    B, H, W, T = 4, 144, 160, 9600
    d = make_inputs("nosync", B, H, W, T)
    p, x, t = dev(d["pred"], True), dev(d["spec_in"], True), dev(d["target"], True)
    wp, wt = dev(d["wav_pred"]), dev(d["wav_true"])
    room = torch.tensor([0, 1, 4, 9], dtype=torch.int32).to(DEV)
    ev = U.Evaluator(None, diff_gen=True)
    ev.update_scored(p, x, t, wp, wt, room)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):
            ev.update_scored(p, x, t, wp, wt, room)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    res = ev.result()
    assert res["n"] == [16, 4, 4, 0, 0, 4]
    want = eval_ref.batch_metrics(d["pred"], d["target"], d["wav_pred"], d["wav_true"], d["spec_in"], 2400)
    check_rows(np.array([[res[n][0] for n in eval_ref.METRICS]]), want.mean(axis=0)[None], "running mean")
