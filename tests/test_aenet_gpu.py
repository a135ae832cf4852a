"""unet_rir_amd.AENetEngine / AENet (dl_models/ae_net.py) on the GPU at 32 x 48, batch 2, against tests/aenet_ref.py; the three
clipped-ReLU kernels against fp64 element by element; the step machinery; one forward + backward of the default model."""
import math

import numpy as np
import pytest
import torch

import aenet_ref as A
import streaming_check as S
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D64 = torch.float64
H, W, B = 32, 48, 2


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _case(F0, mode, batchnorm=True):
    cfg = A.config(H, W, F0, mode, batchnorm)
    params = A.init_params(cfg, f"aenet{F0}m{mode}")
    batch = R.synthetic_batch(cfg, B, f"aenet-d{F0}")
    h5, w5 = H // 16, W // 16
    g = torch.Generator().manual_seed(11)
    masks = tuple(((torch.rand((B, n), generator=g) >= 0.5).double() / 0.5).numpy() for n in (A.VEC_UNITS, h5 * w5 * 2))
    return cfg, params, batch, masks


def _run(eng, params, batch, masks):
    eng.load_keras_params(params)
    t = lambda a: torch.tensor(np.asarray(a)).to(DEV)
    eng.forward(t(batch[0]).float(), t(batch[1]), dropout_mask=tuple(t(m).float().view(B, 1, 1, -1) for m in masks), target=t(batch[2]).float())
    eng.reg_loss()
    eng.backward()
    torch.cuda.synchronize()
    return (eng.pred.double().cpu().clone(), float(eng.loss_out[0]), float(eng.reg_out[0]),
            {k: v.double().cpu() for k, v in eng.export_keras_grads().items()})


@pytest.mark.parametrize("mode,batchnorm", [(0, True), (3, True), (0, False)])
def test_fp32_engine_against_the_restatement(U, mode, batchnorm):
    """Forward, loss and every gradient in fp32 storage (all layers on the generic kernels) at smoke()'s fp32 bounds."""
    cfg, params, batch, masks = _case(4, mode, batchnorm)
    loss, data, pred, z, grads = A.loss_and_grads(params, *batch, cfg, masks)
    assert float(((z > 0) & (z < 1)).double().mean()) > 0.05 and float((z <= 0).double().mean()) > 0.01       # the clip is exercised
    eng = U.AENetEngine(H, W, B, F0=4, mode=mode, batchnorm=batchnorm, device=DEV)
    assert eng.c22_passes == {n[:-len('.kernel')]: 0 for n in A.l2_regularized(cfg)[1:]} and eng.dropout_p == 0.5 and eng.n_dropout_draws == 2
    assert sorted(eng.specs) == sorted(A.param_shapes(cfg)) and eng.l2_names and set(eng.l2_names) == set(A.l2_regularized(cfg))
    pred_h, data_h, reg_h, g_h = _run(eng, params, batch, masks)
    near = ((z.abs() < 2e-5) | ((z - 1).abs() < 2e-5))                  # a logit within fp32 error of a clip edge (a fifth of the bound on the prediction) may land on the other side: the inputs keep clear of that
    assert float((pred_h - pred).abs().max()) <= 1e-4
    assert abs(data_h - data) <= 1e-5 * abs(data) and abs(data_h + reg_h - loss) <= 1e-5 * abs(loss)
    assert int(near.sum()) == 0
    for n, gx in grads.items():
        e = float((g_h[n] - gx).abs().max())
        assert e <= 1e-3 * float(gx.abs().max()) + 1e-9, (n, e)


def test_bf16_engine_runs_the_conv2x2_kernels_and_is_as_close_as_the_storage_model(U):
    """number_filters_0 = 16: every 2x2 stride-2 layer has at least its weight gradient on csrc/conv2x2.hip, forward and data gradient
    where K <= 256 - read from the engine's node list.  Accuracy by the criterion of the other bf16 engines: the restatement with
    bf16 roundings where the product stores bf16 IS the storage model; the HIP path is as close to the exact result as it is."""
    ops = U.ops
    cfg, params, batch, masks = _case(16, 0)
    eng = U.AENetEngine(H, W, B, F0=16, device=DEV, dtype="bf16")
    ch = cfg.enc_channels()
    want = {}
    for l in range(2, 6):
        ci, co = ch[l - 2], ch[l - 1]
        want[f"enc{l}.down"] = ops.C22_WGRAD | (ops.C22_FWD if 4 * ci <= 256 else 0) | (ops.C22_DGRAD if co <= 256 else 0)
        want[f"dec{l - 1}.up"] = ops.C22_WGRAD | (ops.C22_FWD if co <= 256 else 0) | (ops.C22_DGRAD if 4 * ci <= 256 else 0)
    assert eng.c22_passes == want and all(m & ops.C22_WGRAD for m in want.values()) and any(m == 7 for m in want.values())
    generic = U.AENetEngine(H, W, B, F0=16, device=DEV, dtype="bf16", generic_conv2x2=True)
    assert set(generic.c22_passes.values()) == {0}
    pred_h, data_h, _, g_h = _run(eng, params, batch, masks)
    pred_g, data_g, _, g_g = _run(generic, params, batch, masks)
    _, data_q, pred_q, _, g_q = A.loss_and_grads(params, *batch, cfg, masks, storage="bf16")
    _, data_x, pred_x, _, g_x = A.loss_and_grads(params, *batch, cfg, masks)
    nx = float(pred_x.norm())
    for what, pred, data, g in (("conv2x2", pred_h, data_h, g_h), ("generic", pred_g, data_g, g_g)):
        e_h, e_q = float((pred - pred_x).norm()) / nx, float((pred_q - pred_x).norm()) / nx
        print(f"aenet bf16 {what}: pred rel L2 error hip {e_h:.2e} model {e_q:.2e}; loss hip {data:.6f} model {data_q:.6f} exact {data_x:.6f}")
        assert e_h <= 2.0 * e_q + 0.01, (what, e_h, e_q)
        assert abs(data - data_x) <= 2.0 * abs(data_q - data_x) + 1e-2 * abs(data_x), (what, data, data_q, data_x)
        gmax = max(float(v.abs().max()) for v in g_x.values())
        checked = 0
        for n, gx in g_x.items():
            if float(gx.abs().max()) < 1e-6 * gmax:
                continue                               # analytically zero (biases in front of a BatchNorm)
            nrm = float(gx.norm()) + 1e-30
            assert float((g[n] - gx).norm()) / nrm <= 2.0 * float((g_q[n] - gx).norm()) / nrm + 0.03, (what, n)
            checked += 1
        assert checked > 20


TWO_PI_F = float(torch.tensor(6.283185307179586, dtype=torch.float32))
PI_F = float(torch.tensor(3.141592653589793, dtype=torch.float32))


def relu1_loss_ref(z, target, alpha, inv_norm, phase_ref=None, phase_w=None):
    """fp64 reference and per-element bounds of the loss kernel with the clipped ReLU, for logits z [B, H, W, 2] (fp32 values) and
    target [B, 2, H, W]: tests/test_streaming_gpu.py's loss_ref with the other activation.
      pred     p = fminf(fmaxf(z, 0), 1): a selection among exact fp32 numbers - DETERMINED, d = 0
      dlogits  g where 0 < z < 1 (a comparison of exact numbers: determined), else exactly 0, with the roundings of g alone:
               g0 = -2.f da alpha inv, da = t0 - p0: one rounding in da, the product with 2 exact, two more products -> 2;
               g1 = -(1.f - alpha) inv 2pi sinf(ph) w: four products -> 4, sinf within 1 ulp (2 * 2^-24), the phase argument's error
               as there (every fp32 operation 2^-24 of its result, the wrap's |2pi_f - 2pi|), without an error of p1
      sums     fp64 accumulation in a fixed order of fp32 addends, the final conversions: as there."""
    a32 = float(torch.tensor(alpha, dtype=torch.float32)); inv32 = float(torch.tensor(inv_norm, dtype=torch.float32))
    oma32 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(alpha, dtype=torch.float32))
    W_ = target.shape[3]
    zz = z.double()
    p0, p1 = zz[..., 0].clamp(0.0, 1.0), zz[..., 1].clamp(0.0, 1.0)
    in0, in1 = (zz[..., 0] > 0) & (zz[..., 0] < 1), (zz[..., 1] > 0) & (zz[..., 1] < 1)
    t0, t1 = target[:, 0].double(), target[:, 1].double()
    e_t1 = torch.zeros_like(t1)
    if phase_ref is not None:
        t1 = t1 - phase_ref[:, 1].double(); e_t1 = S.U32 * t1.abs()
    w = torch.ones_like(t1) if phase_w is None else phase_w.double().view(1, 1, W_).expand_as(t1)
    da = t0 - p0
    e_da = S.U32 * da.abs()
    e_sq = 2 * da.abs() * e_da + S.U32 * da * da
    a1, a2 = t1 * TWO_PI_F, p1 * TWO_PI_F
    yt, yp = a1 - PI_F, a2 - PI_F
    d1 = yt - yp
    dd = d1 + PI_F
    e_ph = (S.U32 * (a1.abs() + yt.abs() + a2.abs() + yp.abs() + d1.abs() + dd.abs() + TWO_PI_F + PI_F) + TWO_PI_F * e_t1
            + abs(TWO_PI_F - 2 * math.pi))
    ph = torch.remainder(dd, TWO_PI_F) - PI_F
    eph = 1 - torch.cos(ph)
    e_eph = e_ph + 2 * S.U32 * torch.cos(ph).abs() + S.U32 * eph.abs()
    e_ephw = w * e_eph + S.U32 * (eph * w).abs()
    N = da.numel()
    sa, sp, spw = (da * da).sum(), eph.sum(), (eph * w).sum()
    d_sa = S.U32 * sa + e_sq.sum() + N * S.U64 * sa
    d_sp = S.U32 * sp + e_eph.sum() + N * S.U64 * sp
    e_spw = e_ephw.sum() + N * S.U64 * spw
    out0 = (a32 * sa + (1 - a32) * spw) * inv32
    d_out0 = S.U32 * abs(out0) + inv32 * (a32 * (e_sq.sum() + N * S.U64 * sa) + (1 - a32) * e_spw)
    c0 = -2 * a32 * inv32
    g0 = c0 * da
    d_g0 = abs(c0) * e_da + 2 * S.U32 * g0.abs()
    c1 = -oma32 * inv32 * TWO_PI_F
    sn = torch.sin(ph)
    g1 = c1 * sn * w
    d_g1 = abs(c1) * w * (e_ph + 2 * S.U32 * sn.abs()) + 4 * S.U32 * g1.abs()
    zero = torch.zeros_like(g0)
    return dict(p0=p0, p1=p1, v0=torch.where(in0, g0, zero), d_v0=torch.where(in0, d_g0, zero), v1=torch.where(in1, g1, zero),
                d_v1=torch.where(in1, d_g1, zero), sums=torch.stack([out0, sa, sp]), d_sums=torch.stack([d_out0, d_sa, d_sp]))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["plain", "phase_ref", "phase_weight", "both"])
@pytest.mark.parametrize("Bq,Hq,Wq,ldl", [(1, 1, 1, 4), (1, 33, 17, 8), (2, 144, 160, 4)])
def test_relu1_kernels_element_by_element(U, Bq, Hq, Wq, ldl, mode, dt):
    """unetrir_relu1_loss_ex_*, unetrir_relu1_nchw_f32, unetrir_relu1_bwd_* by the criterion of tests/streaming_check.py: every
    element against the fp64 reference with a bound of its own.  Logits straddle 0 and 1 and sit exactly on them (and one ulp to
    either side); phase_ref / phase_weight on and off."""
    ops = U.ops
    g = torch.Generator(device=DEV); g.manual_seed(Bq * Hq + Wq + len(mode))
    ur = lambda shape, lo, hi: torch.rand(shape, device=DEV, generator=g) * (hi - lo) + lo
    alpha, inv_norm = 0.9, 1.0 / (2 * Hq * Wq * Bq)
    z = ur((Bq, Hq, Wq, 2), -0.5, 1.5)
    one = torch.tensor(1.0)
    edges = torch.tensor([0.0, -0.0, 1.0, float(torch.nextafter(one, one * 2)), float(torch.nextafter(one, one * 0)), 1e-45, -1e-45, 5.0], device=DEV)
    pick = torch.randint(0, 64, (Bq, Hq, Wq, 2), device=DEV, generator=g)
    z = torch.where(pick < 8, edges[pick % 8], z)
    target = ur((Bq, 2, Hq, Wq), 0, 1)
    pref = ur((Bq, 2, Hq, Wq), 0, 1) if mode in ("phase_ref", "both") else None
    pw = ur((Wq,), 0, 1) if mode in ("phase_weight", "both") else None
    logits = ops.Act(torch.full((Bq, Hq, Wq, ldl), 777.0, device=DEV), 0, ldl)
    logits.base[..., :2] = z
    ldd = 4 if dt == torch.float32 else 8
    dl = ops.Act(torch.full((Bq, Hq, Wq, ldd), 9.0, dtype=dt, device=DEV))
    pr = torch.full((Bq, 2, Hq, Wq), -1.0, device=DEV)
    out = torch.full((4,), -1.0, device=DEV)
    ws = ops.Workspace(DEV)
    ops.relu1_loss(logits, target, alpha, inv_norm, pr, dl, out, ws, phase_ref=pref, phase_weight=pw)
    torch.cuda.synchronize()
    r = relu1_loss_ref(z, target, alpha, inv_norm, pref, pw)
    tag = f"{(Bq, Hq, Wq)} {mode}"
    S.check(pr[:, 0], r["p0"], 0.0, f"pred 0 {tag}", "relu1_loss pred")
    S.check(pr[:, 1], r["p1"], 0.0, f"pred 1 {tag}", "relu1_loss pred")
    S.check(dl.base[..., :2], torch.stack([r["v0"], r["v1"]], -1), torch.stack([r["d_v0"], r["d_v1"]], -1), f"dlogits {tag}", "relu1_loss dlogits")
    assert float(dl.base[..., 2:].float().abs().max()) == 0.0, "channels 2 ... of dlogits are exact zeros"
    outside = (z <= 0) | (z >= 1)
    assert bool((dl.base[..., :2][outside].float() == 0.0).all()), "gradients are exactly 0 outside 0 < logit < 1"
    S.check(out[:3], r["sums"], r["d_sums"], f"loss, amplitude sum, phase sum {tag}", "relu1_loss sums")
    assert bool(torch.isfinite(out[:3]).all()) and float(out[3]) == -1.0
    assert bool((logits.base[..., 2:] == 777.0).all())
    pr2 = torch.full_like(pr, -1.0)
    ops.relu1_nchw(logits, pr2)
    torch.cuda.synchronize()
    assert torch.equal(pr, pr2)
    # the bridge: g where the STORED prediction lies strictly inside (0, 1), else 0 - no arithmetic: determined (d = 0; bf16: its rounding)
    dpred = ur((Bq, 2, Hq, Wq), -1, 1)
    dl2 = ops.Act(torch.full((Bq, Hq, Wq, ldd), 9.0, dtype=dt, device=DEV))
    ops.relu1_bwd(pr, dpred, dl2)
    torch.cuda.synchronize()
    v = torch.where((pr > 0) & (pr < 1), dpred.double(), torch.zeros_like(dpred, dtype=D64)).permute(0, 2, 3, 1)
    S.check(dl2.base[..., :2], v, 0.0, f"relu1_bwd {tag}", "relu1_bwd")
    assert float(dl2.base[..., 2:].float().abs().max()) == 0.0


def _engine(U, dtype="f32", overlap=False):
    eng = U.AENetEngine(H, W, B, F0=4 if dtype == "f32" else 16, device=DEV, dtype=dtype, overlap_wgrad=overlap)
    eng.reset_parameters(torch.Generator().manual_seed(3))
    eng.dropout_seed = 77
    return eng


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
             torch.rand((B, 2, H, W), generator=gen).to(DEV)) for _ in range(n)]


def _state(eng):
    return (eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}, eng.adam_t,
            eng._shared["dropout_step"])


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_three_steps_twice_from_the_same_seed_are_bit_identical(U, dtype, overlap):
    data = _batches(3)
    res = []
    for _ in range(2):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng.pred.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 6                              # two Dropout draws per step
    assert all(math.isfinite(x) for x in res[0][0])


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_graph_replay_is_the_same_step(U, dtype, overlap):
    data = _batches(3)
    res = []
    for mode in ("graph", "eager_dev"):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, graph=(mode == "graph"))
        if mode == "eager_dev":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng.pred.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])


def test_checkpoint_after_step_2_resumes_to_a_bit_identical_step_3(U, tmp_path):
    data = _batches(3)
    e0 = _engine(U)
    t0 = U.Trainer(e0, lr=1e-3)
    for a, e, b in data:
        t0.step(a, e, b)
    torch.cuda.synchronize()
    e1 = _engine(U)
    t1 = U.Trainer(e1, lr=1e-3)
    for a, e, b in data[:2]:
        t1.step(a, e, b)
    path = U.CheckpointManager(t1, str(tmp_path)).save(epoch=0)
    e2 = U.AENetEngine(H, W, B, F0=4, device=DEV)
    e2.reset_parameters(torch.Generator().manual_seed(99))
    e2.dropout_seed = 5
    t2 = U.Trainer(e2, lr=1e-3)
    U.CheckpointManager(t2, str(tmp_path)).restore(path)
    assert e2._shared["dropout_step"] == 4 and e2.dropout_seed == 77
    t2.step(*data[2])
    torch.cuda.synchronize()
    _same(_state(e0), _state(e2))
    assert torch.equal(e0.pred, e2.pred)


def test_inference_uses_the_moving_statistics_and_the_evaluator_scores_a_batch(U):
    cfg, params, (spec_in, emb, spec_out), _ = _case(4, 0)
    model = U.AENet((H, W, 2), (2, 16), number_filters_0=4, batch_size=B, device=DEV)
    eng = model.engine
    eng.load_keras_params(params)
    g = torch.Generator().manual_seed(4)
    for n, b in eng.moving.items():
        b.copy_((torch.rand(b.shape, generator=g) * 0.5 + (0.75 if n.endswith("variance") else -0.25)).to(DEV))
    moving = {n: b.double().cpu() for n, b in eng.moving.items()}
    t = lambda a: torch.tensor(a).to(DEV)
    eng.training = False
    pred = eng.forward(t(spec_in), t(emb)).double().cpu()
    torch.cuda.synchronize()
    P = {k: torch.tensor(np.asarray(v), dtype=D64) for k, v in params.items()}
    ref = A.forward(P, torch.tensor(spec_in, dtype=D64), torch.tensor(emb), cfg, training=False, bn_state=moving)
    assert float((pred - ref).abs().max()) <= 1e-4 and float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0
    for n, b in eng.moving.items():
        assert torch.equal(b.double().cpu(), moving[n]), n
    ev = U.Evaluator(model)
    with torch.no_grad():
        out = model.model([t(spec_in).permute(0, 2, 3, 1), t(emb)], training=False)
    ev.update_scored(out.permute(0, 3, 1, 2).contiguous(), t(spec_in), t(spec_out), None, None, [ev.rooms[0]] * B)
    res = ev.result()
    torch.cuda.synchronize()
    assert res is not None and float((out.permute(0, 3, 1, 2).double().cpu() - ref).abs().max()) <= 1e-4


def test_module_surface_and_save_load(U, tmp_path):
    import inspect
    import pickle
    sig = inspect.signature(U.AENet.__init__)
    assert list(sig.parameters)[1:10] == ["input_shape", "inf_vector_shape", "learning_rate", "mode", "number_filters_0", "BatchNorm",
                                          "resize_factor_0", "res_factor", "name"]
    assert sig.parameters["name"].default == "AENet" and sig.parameters["number_filters_0"].default == 32
    assert sig.parameters["learning_rate"].default == 1e-5 and sig.parameters["BatchNorm"].default is True
    with pytest.raises(ValueError):
        U.AENetEngine(40, 48, B, F0=4, device=DEV)                       # 40 does not halve four times
    model = U.AENet((H, W, 2), (2, 16), number_filters_0=4, mode=3, batch_size=B, device=DEV)
    assert isinstance(model.engine, U.AENetEngine) and len(model.model.losses) == 9
    gen = torch.Generator(); gen.manual_seed(2)
    spec = torch.rand((B, H, W, 2), generator=gen).to(DEV)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV)
    with torch.no_grad():
        out = model.model([spec, emb], training=False).clone()
    assert tuple(out.shape) == (B, H, W, 2) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f)[:6] == [(H, W, 2), (2, 16), 1e-5, 3, 4, True]
    again = U.AENet.load(str(tmp_path), batch_size=B, device=DEV)
    assert torch.equal(again.engine.theta, model.engine.theta) and again.mode == 3
    with torch.no_grad():
        assert torch.equal(again.model([spec, emb], training=False), out)
    shared = U.AENetEngine(H, W, 1, F0=4, mode=3, device=DEV, share=model.engine)
    assert shared.theta.data_ptr() == model.engine.theta.data_ptr()       # share= aliases the parameters
    # the autograd bridge: dL/dprediction through the clipped ReLU into every parameter
    model.train()
    y = model(spec.permute(0, 3, 1, 2).contiguous(), emb)
    (y ** 2).mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_default_model_forward_and_backward(U):
    """The default model (144 x 160, number_filters_0 = 32, batch 2, bf16): finite values, predictions in [0, 1], a gradient for every
    parameter."""
    eng = U.AENetEngine(144, 160, 2, device=DEV, dtype="bf16")
    eng.reset_parameters(torch.Generator().manual_seed(1))
    assert tuple(eng.specs["rec.dense.kernel"].keras_shape) == (9 * 10 * 512 + 2048, 180)
    gen = torch.Generator(); gen.manual_seed(8)
    spec, tgt = torch.rand((2, 2, 144, 160), generator=gen).to(DEV), torch.rand((2, 2, 144, 160), generator=gen).to(DEV)
    emb = torch.randint(26, 1282, (2, 2, 16), generator=gen).to(DEV)
    pred = eng.forward(spec, emb, dropout_mask=eng.make_dropout_mask(), target=tgt)
    eng.backward()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(pred).all()) and float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0
    assert math.isfinite(float(eng.loss_out[0]))
    for n, gk in eng.export_keras_grads().items():
        assert bool(torch.isfinite(gk).all()), n
        if not (n.endswith(".bias") and eng.batchnorm and ("cb1" in n or ".fb." in n)):
            assert float(gk.abs().max()) > 0.0, n
