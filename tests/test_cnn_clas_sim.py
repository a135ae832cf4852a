"""The PRODUCT's DeepCNNEngine + Trainer + fit + deep_CNN on CPU tensors: only the kernels (tests/cnn_clas_cpu_ops.py: fp64 arithmetic)
and the stream runtime (tests/sim_runtime.py: vector clocks + race check) are stand-ins.  21 x 24 x 2, five classes, batch 3, against
tests/cnn_clas_ref.py: the sizes run 19x22 -> 9x11 -> 7x9 -> 3x4 -> 1x2, so the first pool drops a row, the second a row and a column
and the global pool runs over two pixels.  A missing happens-before edge would raise RaceError."""
import pickle

import numpy as np
import pytest
import torch

H, W, B, CLASSES = 21, 24, 3, 5
LR, N_STEPS = 1e-3, 2
P_ATOL = 0.02 * LR * N_STEPS          # the bound of tests/test_aenet_sim.py


def _install(monkeypatch):
    import cnn_clas_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, cnn_clas_cpu_ops.install(monkeypatch, rt)


def _setup(batchnorm, n=B, tag="d"):
    import cnn_clas_ref as A
    cfg = A.config(H, W, 2, CLASSES, batchnorm)
    batch = A.synthetic_batch(cfg, n, f"sim/{tag}")
    return cfg, A.keep_clear_of_flat_biases(cfg, A.init_params(cfg, f"sim{batchnorm}"), batch[0]), batch


def _mask(seed=100):
    return ((np.random.RandomState(seed).uniform(size=(B, 256)) >= 0.5) / 0.5).astype(np.float32)


def _build(rt, cfg, params, overlap=False, world=1, dropout=False, lr=LR, share=None, batch=B, optimizer="adam"):
    import unet_rir_amd as U
    eng = U.DeepCNNEngine(H, W, batch, classes=cfg.classes, batchnorm=cfg.batchnorm, device="cpu", runtime=rt, n_replicas=world,
                          overlap_wgrad=overlap, share=share)
    if share is None:
        eng.load_keras_params(params)
    return eng, U.Trainer(eng, lr=lr, dropout=dropout, world_size=world, bucket_bytes=8192, optimizer=optimizer)


@pytest.mark.parametrize("batchnorm,overlap", [(True, False), (True, True), (False, False), (False, True)])
def test_two_adam_steps_on_the_product_schedule_match_the_restatement(monkeypatch, batchnorm, overlap):
    import cnn_clas_ref as A
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(batchnorm)
    y[1] = [0.1, 0.5, 0.0, 0.7, 0.2]                       # a soft row that does not sum to 1
    eng, tr = _build(rt, cfg, params, overlap)
    assert {n: tuple(s.keras_shape) for n, s in eng.specs.items()} == A.param_shapes(cfg)
    assert eng.n_params() == A.n_params(cfg) and sorted(eng.moving) == sorted(A.moving_shapes(cfg))
    assert eng.l2_names == [] and eng.n_dropout_draws == 1 and eng.dropout_p == 0.5 and eng.mask_width == {"fc": 256}
    sizes = [(n.a.H, n.a.W, n.a.C) for n in eng.nodes[:6]]
    assert sizes == [(21, 24, 4), (19, 22, 16), (9, 11, 16), (7, 9, 32), (3, 4, 32), (1, 2, 64)]
    mask = _mask()
    tx, ty, tm = torch.tensor(x), torch.tensor(y), torch.tensor(mask).view(B, 1, 1, -1)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    for t in range(1, N_STEPS + 1):
        loss, ce, probs, z, ok, grads = A.loss_and_grads(p64, x, y, cfg, mask=mask)
        got = tr.step(tx, None, ty, dropout_mask=tm, return_loss=True)
        assert abs(got - loss) <= 1e-5 * abs(loss), (t, got, loss)
        assert float(eng.reg_out[0]) == 0.0 and float(eng.loss_out[2]) == 0.0
        assert abs(float(eng.loss_out[1]) - ce) <= 1e-5 * ce and float(eng.acc_out[0]) == ok
        assert float((eng.probs.double() - probs).abs().max()) <= 1e-5
        if t == 1:
            got_g = eng.export_keras_grads()
            floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
            for n, g in grads.items():
                e = float((got_g[n].double() - g).abs().max())
                assert e <= 1e-4 * float(g.abs().max()) + floor, (n, e)
                assert float(g.abs().max()) > 0, n
            if cfg.classes % 4:                            # the zero rows behind `classes` of the padded output layer stay zero
                assert float(eng.g["dense_1.kernel"][cfg.classes:].abs().max()) == 0.0
        for k in p64:
            new, m[k], v_[k] = R.adam_update(torch.tensor(p64[k]), grads[k], m[k], v_[k], t, LR)
            p64[k] = new.numpy()
    got = eng.export_keras_params()
    for n, w in p64.items():
        assert float(np.abs(got[n].double().numpy() - w).max()) <= P_ATOL, n
    assert float(eng.p["dense_1.kernel"][cfg.classes:].abs().max()) == 0.0 and float(eng.p["Conv0_A.kernel"][..., 2:].abs().max()) == 0.0
    assert rt.n_cross_stream > 10 if overlap else rt.n_cross_stream == 0


def test_moving_statistics_and_inference_follow_the_restatement(monkeypatch):
    import cnn_clas_ref as A
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(True)
    eng, tr = _build(rt, cfg, params, lr=0.0)
    state = {n: (torch.ones(s, dtype=torch.float64) if n.endswith("variance") else torch.zeros(s, dtype=torch.float64))
             for n, s in A.moving_shapes(cfg).items()}
    P = A.to_torch(params)
    tx = torch.tensor(x)
    A.logits(P, tx.double(), cfg, bn_state=state)
    eng.forward(tx, target=torch.tensor(y))
    for n, want in state.items():
        assert float((eng.moving[n].double() - want).abs().max()) <= 1e-6 * float(want.abs().max()), n
    eng.training = False
    probs = eng.forward(tx)
    want = A.forward(P, tx.double(), cfg, training=False, bn_state=state)
    assert float((probs.double() - want).abs().max()) <= 1e-5
    assert float((probs.double().sum(1) - 1).abs().max()) <= 2.0 ** -22 * CLASSES


@pytest.mark.parametrize("dropout", [False, True])
def test_one_dropout_draw_per_step(monkeypatch, dropout):
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(True)
    eng, tr = _build(rt, cfg, params, dropout=dropout, lr=0.0)
    for _ in range(3):
        tr.step(torch.tensor(x), None, torch.tensor(y))
    assert eng._shared["dropout_step"] == (3 if dropout else 0)
    assert (eng.masks["fc"] is not None) == dropout
    if dropout:
        assert set(torch.unique(eng.masks["fc"]).tolist()) == {0.0, 2.0}          # Dropout(.5): keep scaled by 1 / (1 - 0.5)


def test_fit_reports_the_restatements_accuracy_counts(monkeypatch):
    import unet_rir_amd as U
    import cnn_clas_ref as A
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    cfg, params, _ = _setup(True)
    train = [A.synthetic_batch(cfg, B, f"sim/fit{i}") for i in range(2)]
    val = [A.synthetic_batch(cfg, B, "sim/val")]
    eng, tr = _build(rt, cfg, params)
    manager = None
    tt = lambda bs: [(torch.tensor(x), None, torch.tensor(y)) for x, y, _ in bs]
    hist = U.fit(tr, lambda ep: tt(train), 2, val_batches=lambda ep: tt(val), manager=manager, log=None, lr_exp_decay=(False, 80))
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    m = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    v_ = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}
    t = 0
    for epoch in range(2):
        ok_t, ce_t = 0, 0.0
        for x, y, _ in train:
            t += 1
            loss, ce, probs, z, ok, grads = A.loss_and_grads(p64, x, y, cfg)
            ok_t, ce_t = ok_t + ok, ce_t + ce
            for k in p64:
                new, m[k], v_[k] = R.adam_update(torch.tensor(p64[k]), grads[k], m[k], v_[k], t, LR)
                p64[k] = new.numpy()
        ok_v = sum(A.loss_and_grads(p64, x, y, cfg)[4] for x, y, _ in val)
        rec = hist[epoch]
        assert rec["train_acc"] == ok_t / (len(train) * B) and rec["val_acc"] == ok_v / (len(val) * B), (epoch, rec, ok_t, ok_v)
        assert abs(rec["train_amp"] - ce_t / (len(train) * B)) <= 1e-5 * rec["train_amp"] and rec["train_phase"] == 0.0 and rec["val_phase"] == 0.0
        assert abs(rec["train_loss"] - ce_t / (len(train) * B)) <= 1e-5 * rec["train_loss"]
    # without a validation pass the training accuracy is still reported
    eng2, tr2 = _build(rt, cfg, params, lr=0.0)
    rec = U.fit(tr2, lambda ep: tt(train), 1, log=None)[0]
    assert rec["train_acc"] == sum(A.loss_and_grads(params, x, y, cfg)[4] for x, y, _ in train) / (len(train) * B) and "val_acc" not in rec


def test_other_engines_records_have_no_accuracy_column(monkeypatch):
    import unet_rir_amd as U
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    eng = U.UNetGraphEngine(32, 32, 2, F0=4, k=3, mode=1, device="cpu", runtime=rt)
    eng.reset_parameters()
    tr = U.Trainer(eng, lr=0.0, dropout=False)
    tb = tuple(torch.tensor(a) for a in R.synthetic_batch(R.Config(32, 32, 4, 3), 2))
    rec = U.fit(tr, lambda ep: [tb], 1, val_batches=lambda ep: [tb], log=None)[0]
    assert "train_acc" not in rec and "val_acc" not in rec and rec["train_phase"] > 0


def test_share_checkpoint_and_two_replicas(monkeypatch, tmp_path):
    import unet_rir_amd as U
    import cnn_clas_ref as A
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(True)
    eng, tr = _build(rt, cfg, params, overlap=True, world=2, lr=0.0)
    loss = tr.step(torch.tensor(x), None, torch.tensor(y), dropout_mask=torch.tensor(_mask()).view(B, 1, 1, -1), return_loss=True)
    want = A.loss_and_grads(params, x, y, cfg, mask=_mask(), global_batch=2 * B)[0]           # replica 0 of 2: sum CE / global batch
    assert abs(loss - want) <= 1e-5 * want
    other, _ = _build(rt, cfg, params, share=eng, batch=2)
    assert other.theta.data_ptr() == eng.theta.data_ptr() and other.moving["bn3.moving_mean"].data_ptr() == eng.moving["bn3.moving_mean"].data_ptr()
    eng1, tr1 = _build(rt, cfg, params, optimizer="nadam")
    tr1.step(torch.tensor(x), None, torch.tensor(y))
    mgr = U.CheckpointManager(tr1, str(tmp_path))
    path = mgr.save(epoch=0)
    theta = eng1.theta.clone()
    tr1.step(torch.tensor(x), None, torch.tensor(y))
    assert not torch.equal(eng1.theta, theta)
    assert mgr.restore(path) == 0 and torch.equal(eng1.theta, theta) and eng1.adam_t == 1
    lamb_eng, lamb_tr = _build(rt, cfg, params, optimizer=U.LAMB(learning_rate=1e-3))
    assert lamb_eng.optimizer == "lamb" and len(lamb_eng._shared["lamb"]["opt"].segments(lamb_eng.specs)) == len(lamb_eng.specs)


def test_deep_cnn_class_round_trips_save_and_load(monkeypatch, tmp_path):
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(True)
    model = U.deep_CNN(H, W, 2, CLASSES, True, "adam", 1e-3, batch_size=B, device="cpu", runtime=rt)
    assert model.model is None and model.criterion is None
    model.build_model()
    model.set_optimizer_criterion()
    net, opt, crit = model.return_params()
    assert opt == "adam" and model.optimizer_kind == "adam" and isinstance(model.engine, U.DeepCNNEngine)
    assert U.deep_CNN(H, W, 2, CLASSES, True, "my_nadam_sgd", 1e-3).optimizer == "my_nadam_sgd"
    m2 = U.deep_CNN(H, W, 2, CLASSES, True, "sgd_then_adam", 1e-3); m2.set_optimizer_criterion()
    assert m2.optimizer_kind == "sgd"                    # the reference's substring order: nadam, sgd, adam
    assert len(net.trainable_variables) == len(model.engine.specs) == 18
    # freshly initialised: glorot-uniform kernels (within their limit, zero padding), zero biases, gamma 1
    k = model.engine.export_keras_params()
    assert float(k["Conv1_A.kernel"].abs().max()) <= (6.0 / (9 * 16 + 9 * 32)) ** 0.5 and float(k["Conv1_A.kernel"].abs().max()) > 0
    assert float(k["dense_1.bias"].abs().max()) == 0.0 and float((k["bn2.gamma"] - 1).abs().max()) == 0.0
    assert float(model.engine.p["dense_1.kernel"][CLASSES:].abs().max()) == 0.0
    model.engine.load_keras_params(params)
    nhwc = torch.tensor(x).permute(0, 2, 3, 1).contiguous()
    a = net(nhwc, training=False).clone()
    assert tuple(a.shape) == (B, CLASSES) and torch.equal(net(torch.tensor(x)), a)          # NCHW is accepted too
    yt = torch.tensor(y)
    ce = crit(yt, a)
    assert tuple(ce.shape) == (B,) and torch.allclose(ce, -(yt * a.clamp(1e-7, 1 - 1e-7).log()).sum(1), rtol=1e-5, atol=0)
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [H, W, 2, CLASSES, True, "adam", 1e-3]
    again = U.deep_CNN.load(str(tmp_path), batch_size=B, device="cpu", runtime=rt)
    assert torch.equal(again.engine.theta, model.engine.theta) and torch.equal(again.model(nhwc), a)
    for n, b in model.engine.moving.items():
        assert torch.equal(again.engine.moving[n], b), n
    assert tuple(net(nhwc[:2], training=True).shape) == (2, CLASSES)                        # another batch size: an aliasing engine
    assert model._engines[2].theta.data_ptr() == model.engine.theta.data_ptr() and model.engine._shared["dropout_step"] == 1
    tr = U.Trainer(again, optimizer=again.optimizer, lr=again.learning_rate, dropout=False)
    assert tr.engine is again.engine and np.isfinite(tr.step(torch.tensor(x), None, yt, return_loss=True))


def test_gate_refuses_bad_tensors_before_any_launch(monkeypatch):
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(True)
    eng, tr = _build(rt, cfg, params)
    tx, ty = torch.tensor(x), torch.tensor(y)
    n0 = rt.main.clock["main"]
    bad_x = [tx[:2], tx.double(), tx.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), torch.empty(tx.shape, device="meta")]
    bad_y = [ty[:, :4], ty.double(), ty.t().contiguous().t(), torch.empty(ty.shape, device="meta")]
    for bx in bad_x:
        with pytest.raises(ValueError):
            eng.forward(bx, target=ty)
    for by in bad_y:
        with pytest.raises(ValueError):
            eng.forward(tx, target=by)
        with pytest.raises(ValueError):
            eng.loss_from_logits(by)
        with pytest.raises(ValueError):
            eng.backward(dpred=by)
    assert rt.main.clock["main"] == n0 and rt.accesses == []


def test_unsupported_configurations_are_refused(monkeypatch):
    import unet_rir_amd as U
    rt, impl = _install(monkeypatch)
    with pytest.raises(NotImplementedError, match="follow-up"):
        U.DeepCNNEngine(H, W, B, dtype="bf16", device="cpu", runtime=rt)
    with pytest.raises(ValueError):
        U.DeepCNNEngine(H, W, B, depth=3, device="cpu", runtime=rt)
    with pytest.raises(ValueError):
        U.DeepCNNEngine(H, W, B, classes=1025, device="cpu", runtime=rt)
    with pytest.raises(ValueError):
        U.DeepCNNEngine(17, 24, B, device="cpu", runtime=rt)           # 15 -> 7 -> 5 -> 2: no third convolution


def test_upstream_gradient_on_the_probabilities(monkeypatch):
    """backward(dpred=...) seeds the pass through the softmax bridge: the gradients of sum(c * p)."""
    import cnn_clas_ref as A
    rt, impl = _install(monkeypatch)
    cfg, params, (x, y, _) = _setup(False)
    eng, tr = _build(rt, cfg, params)
    c = torch.tensor(np.random.RandomState(5).uniform(-1, 1, size=(B, CLASSES)).astype(np.float32))
    eng.forward(torch.tensor(x))
    eng.backward(dpred=c)
    P = A.to_torch(params, torch.float64, True)
    (A.forward(P, torch.tensor(x, dtype=torch.float64), cfg) * c.double()).sum().backward()
    got = eng.export_keras_grads()
    for n, p in P.items():
        assert float((got[n].double() - p.grad).abs().max()) <= 1e-4 * float(p.grad.abs().max()) + 1e-9, n


def test_training_script_builds_one_hot_rows_from_room_indices():
    """scripts/train_classifier.py: the room indices of DataGenerator(characteristics=True) -> one-hot rows, -1 (no known room) -> a zero
    row; the classifier's batches are (target spectrogram, None, rows)."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "train_classifier.py")
    spec = importlib.util.spec_from_file_location("train_classifier", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    rows = mod.one_hot(torch.tensor([3, 0, -1, 4], dtype=torch.int32), 5)
    assert rows.dtype == torch.float32 and rows.tolist() == [[0, 0, 0, 1, 0], [1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 1]]

    class Gen:
        def batches(self, epoch=None):
            yield "in", "emb", "out", (torch.tensor([1, 2], dtype=torch.int32), "wav")
    (x, emb, y), = list(mod.classifier_batches(Gen(), 5)(0))
    assert x == "out" and emb is None and y.tolist() == [[0, 1, 0, 0, 0], [0, 0, 1, 0, 0]]
