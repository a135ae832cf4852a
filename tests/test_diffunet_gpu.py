"""unet_rir_amd.DiffUNetEngine / DiffUNet (dl_models/diff_u_net.py) on the GPU at 32 x 48, batch 2, against tests/diffunet_ref.py; the
step machinery; the evaluator under diff_gen; one forward + backward of the default model.  Trained with diff_loss=True throughout:
the phase target is phase_true - phase_x (main_training.py:214-217), the loss this model exists for."""
import math

import numpy as np
import pytest
import torch

import diffunet_ref as DU
import eval_ref
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
    cfg = DU.config(H, W, F0, mode, batchnorm)
    params = DU.init_params(cfg, f"diffunet{F0}m{mode}")
    # without BatchNorm a random net lets little through and the logits stay near the head's bias: a wider head and a bias on either
    # side of [0, 1] keep a fair share of the predictions outside it in every case (what a sigmoid or a clipped ReLU could not put out)
    params["head.kernel"] = params["head.kernel"] * 4.0
    params["head.bias"] = np.array([-0.3, 0.9], dtype=params["head.bias"].dtype)
    batch = R.synthetic_batch(cfg, B, f"diffunet-d{F0}")
    g = torch.Generator().manual_seed(11)
    masks = (((torch.rand((B, DU.vec_units(cfg)), generator=g) >= 0.5).double() / 0.5).numpy(),)
    return cfg, params, batch, masks


def _run(eng, params, batch, masks):
    eng.load_keras_params(params)
    eng.loss_diff = True                                      # Trainer(diff_loss=True) sets this
    t = lambda a: torch.tensor(np.asarray(a)).to(DEV)
    eng.forward(t(batch[0]).float(), t(batch[1]), dropout_mask=t(masks[0]).float().view(B, 1, 1, -1), target=t(batch[2]).float())
    eng.reg_loss()
    eng.backward()
    torch.cuda.synchronize()
    return (eng.pred.double().cpu().clone(), float(eng.loss_out[0]), float(eng.reg_out[0]),
            {k: v.double().cpu() for k, v in eng.export_keras_grads().items()})


@pytest.mark.parametrize("mode,batchnorm", [(0, True), (3, True), (0, False), (3, False)])
def test_fp32_engine_against_the_restatement(U, mode, batchnorm):
    """Forward, loss and every gradient in fp32 storage (all layers on the generic kernels) at the bounds
    test_aenet_gpu.test_fp32_engine_against_the_restatement uses."""
    cfg, params, batch, masks = _case(4, mode, batchnorm)
    loss, data, pred, z, grads = DU.loss_and_grads(params, *batch, cfg, masks, diff_loss=True)
    outside = float(((pred < 0) | (pred > 1)).double().mean())
    print(f"diffunet fp32 mode {mode} bn {batchnorm}: {outside:.1%} of the reference's predictions lie outside [0, 1]")
    assert outside > 0.1                                      # the linear output is exercised, not merely allowed
    eng = U.DiffUNetEngine(H, W, B, F0=4, mode=mode, batchnorm=batchnorm, device=DEV)
    assert eng.head_passes == 0 and set(eng.c22_passes.values()) == {0} and eng.dropout_p == 0.5 and eng.n_dropout_draws == 1
    assert sorted(eng.specs) == sorted(DU.param_shapes(cfg)) and set(eng.l2_names) == set(DU.l2_regularized(cfg))
    pred_h, data_h, reg_h, g_h = _run(eng, params, batch, masks)
    assert float((pred_h - pred).abs().max()) <= 1e-4
    assert abs(data_h - data) <= 1e-5 * abs(data) and abs(data_h + reg_h - loss) <= 1e-5 * abs(loss)
    for n, gx in grads.items():
        e = float((g_h[n] - gx).abs().max())
        assert e <= 1e-3 * float(gx.abs().max()) + 1e-9, (n, e)


def test_bf16_engine_runs_the_head_kernels_and_is_as_close_as_the_storage_model(U):
    """number_filters_0 = 16: the head runs the passes the predicate answers, the 2x2 layers what AENet's do.  Accuracy by the criterion of
    test_aenet_gpu.test_bf16_engine_runs_the_conv2x2_kernels_and_is_as_close_as_the_storage_model: the restatement with bf16 roundings
    where the product stores bf16 IS the storage model; the HIP path is as close to the exact result as it is - with head1x1 (fp32
    logits) and with generic_head=True (the generic kernels store bf16 logits)."""
    ops = U.ops
    cfg, params, batch, masks = _case(16, 0)
    eng = U.DiffUNetEngine(H, W, B, F0=16, device=DEV, dtype="bf16")
    assert eng.head_passes == ops.head1x1_supported(16)
    assert eng.c22_passes == U.AENetEngine(H, W, B, F0=16, device=DEV, dtype="bf16").c22_passes
    generic = U.DiffUNetEngine(H, W, B, F0=16, device=DEV, dtype="bf16", generic_head=True)
    assert generic.head_passes == 0 and generic.c22_passes == eng.c22_passes
    _, data_x, pred_x, _, g_x = DU.loss_and_grads(params, *batch, cfg, masks, diff_loss=True)
    nx = float(pred_x.norm())
    for what, e_, hs in (("head1x1", eng, "f32" if eng.head_passes & 1 else "bf16"), ("generic", generic, "bf16")):
        pred, data, _, g = _run(e_, params, batch, masks)
        _, data_q, pred_q, _, g_q = DU.loss_and_grads(params, *batch, cfg, masks, diff_loss=True, storage="bf16", head_storage=hs)
        e_h, e_q = float((pred - pred_x).norm()) / nx, float((pred_q - pred_x).norm()) / nx
        print(f"diffunet bf16 {what}: pred rel L2 error hip {e_h:.2e} model {e_q:.2e}; loss hip {data:.6f} model {data_q:.6f} exact {data_x:.6f}")
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


def _engine(U, dtype="f32", overlap=False):
    eng = U.DiffUNetEngine(H, W, B, F0=4 if dtype == "f32" else 16, device=DEV, dtype=dtype, overlap_wgrad=overlap)
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
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, diff_loss=True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng.pred.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 3                              # one Dropout draw per step
    assert all(math.isfinite(x) for x in res[0][0])


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_graph_replay_is_the_same_step(U, dtype, overlap):
    data = _batches(3)
    res = []
    for mode in ("graph", "eager_dev"):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, graph=(mode == "graph"), diff_loss=True)
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
    t0 = U.Trainer(e0, lr=1e-3, diff_loss=True)
    for a, e, b in data:
        t0.step(a, e, b)
    torch.cuda.synchronize()
    e1 = _engine(U)
    t1 = U.Trainer(e1, lr=1e-3, diff_loss=True)
    for a, e, b in data[:2]:
        t1.step(a, e, b)
    path = U.CheckpointManager(t1, str(tmp_path)).save(epoch=0)
    e2 = U.DiffUNetEngine(H, W, B, F0=4, device=DEV)
    e2.reset_parameters(torch.Generator().manual_seed(99))
    e2.dropout_seed = 5
    t2 = U.Trainer(e2, lr=1e-3, diff_loss=True)
    U.CheckpointManager(t2, str(tmp_path)).restore(path)
    assert e2._shared["dropout_step"] == 2 and e2.dropout_seed == 77
    t2.step(*data[2])
    torch.cuda.synchronize()
    _same(_state(e0), _state(e2))
    assert torch.equal(e0.pred, e2.pred)


def test_inference_uses_the_moving_statistics_and_the_evaluator_scores_a_batch_under_diff_gen(U):
    cfg, params, (spec_in, emb, spec_out), _ = _case(4, 0)
    model = U.DiffUNet((H, W, 2), (2, 16), number_filters_0=4, batch_size=B, device=DEV)
    eng = model.engine
    assert isinstance(eng, U.DiffUNetEngine)
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
    ref = DU.forward(P, torch.tensor(spec_in, dtype=D64), torch.tensor(emb), cfg, training=False, bn_state=moving)
    assert float((pred - ref).abs().max()) <= 1e-4 and (float(pred.min()) < 0.0 or float(pred.max()) > 1.0)
    for n, b in eng.moving.items():
        assert torch.equal(b.double().cpu(), moving[n]), n
    ev = U.Evaluator(model, diff_gen=True)
    with torch.no_grad():
        out = model.model([t(spec_in).permute(0, 2, 3, 1), t(emb)], training=False).clone()           # NHWC
    ev.update_scored(out.permute(0, 3, 1, 2).contiguous(), t(spec_in), t(spec_out), None, None, [ev.rooms[0]] * B)
    res = ev.result()
    torch.cuda.synchronize()
    assert float((out.permute(0, 3, 1, 2).double().cpu() - ref).abs().max()) <= 1e-4
    nhwc = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))
    want = eval_ref.batch_metrics(out.cpu().numpy(), nhwc(spec_out), None, None, nhwc(spec_in)).mean(0)
    for c, name in enumerate(eval_ref.METRICS[:3]):            # the phase figure is that of the SUMMED phase (rir_generation.py:190-193)
        got = res[name][0]
        print(f"evaluator diff_gen {name}: got {got!r} want {want[c]!r}")
        assert abs(got - want[c]) <= 1e-10 * abs(want[c]), (name, got, want[c])
    plain = eval_ref.batch_metrics(out.cpu().numpy(), nhwc(spec_out)).mean(0)
    assert abs(plain[2] - want[2]) > 1e-3 * abs(want[2])       # ... and differs from the raw prediction's


def test_module_autograd_bridge_and_train_script_surface(U, tmp_path):
    model = U.DiffUNet((H, W, 2), (2, 16), number_filters_0=4, mode=3, batch_size=B, device=DEV)
    assert len(model.model.losses) == 9
    gen = torch.Generator(); gen.manual_seed(2)
    spec = torch.rand((B, H, W, 2), generator=gen).to(DEV)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV)
    with torch.no_grad():
        out = model.model([spec, emb], training=False).clone()
    model.save(str(tmp_path))
    again = U.DiffUNet.load(str(tmp_path), batch_size=B, device=DEV)
    with torch.no_grad():
        assert torch.equal(again.model([spec, emb], training=False), out)
    # the autograd bridge (linear_bwd): dL/dprediction = 2 y / N passes into the logits unchanged, so the head's bias gradient is its sum
    model.train()
    y = model(spec.permute(0, 3, 1, 2).contiguous(), emb)
    (y ** 2).mean().backward()
    torch.cuda.synchronize()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    want = (2.0 * y.detach().double() / y.numel()).sum(dim=(0, 2, 3)).cpu()
    got = model.engine.export_keras_grads()["head.bias"].double().cpu()
    assert float((got - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_default_model_forward_and_backward(U):
    """The default model (144 x 160, number_filters_0 = 32, batch 2, bf16): finite values, the head kernels run, a gradient for every
    parameter."""
    eng = U.DiffUNetEngine(144, 160, 2, device=DEV, dtype="bf16")
    eng.reset_parameters(torch.Generator().manual_seed(1))
    eng.loss_diff = True
    assert eng.head_passes == U.ops.head1x1_supported(32)
    assert tuple(eng.specs["encoder_inf_dense.kernel"].keras_shape) == (32 * 128, 9 * 10 * 512)
    calls = []
    real_f, real_b = U.ops.head1x1_fwd, U.ops.head1x1_bwd
    mp = pytest.MonkeyPatch()
    mp.setattr(U.ops, "head1x1_fwd", lambda *a: (calls.append("fwd"), real_f(*a))[1])
    mp.setattr(U.ops, "head1x1_bwd", lambda *a: (calls.append("bwd"), real_b(*a))[1])
    try:
        gen = torch.Generator(); gen.manual_seed(8)
        spec, tgt = torch.rand((2, 2, 144, 160), generator=gen).to(DEV), torch.rand((2, 2, 144, 160), generator=gen).to(DEV)
        emb = torch.randint(26, 1282, (2, 2, 16), generator=gen).to(DEV)
        pred = eng.forward(spec, emb, dropout_mask=eng.make_dropout_mask(), target=tgt)
        eng.backward()
        torch.cuda.synchronize()
    finally:
        mp.undo()
    assert calls == [n for n, bit in (("fwd", 1), ("bwd", 2)) if eng.head_passes & bit]
    assert bool(torch.isfinite(pred).all()) and math.isfinite(float(eng.loss_out[0]))
    for n, gk in eng.export_keras_grads().items():
        assert bool(torch.isfinite(gk).all()), n
        if not (n.endswith(".bias") and eng.batchnorm and ("cb1" in n or ".fb." in n)):
            assert float(gk.abs().max()) > 0.0, n
