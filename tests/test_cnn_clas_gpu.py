"""unet_rir_amd.DeepCNNEngine / deep_CNN (dl_models/cnn_clas.py) on the GPU against tests/cnn_clas_ref.py at the fp32 tolerances of
tests/test_aenet_gpu.py (loss 1e-5 relative, output 1e-4, gradients 1e-3 of the largest one): 21 x 24 x 2, batch 3, two steps under each
optimizer; 144 x 160 x 2, batch 4, one step; determinism, the captured step, the inference output and fit's accuracy column."""
import math

import numpy as np
import pytest
import torch

import cnn_clas_ref as A
import lamb_ref
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = 5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


_CASES = {}


def _case(H, W, B, batchnorm=True):
    """(cfg, params, x, y, mask) - computed once per geometry and shared."""
    key = (H, W, B, batchnorm)
    if key not in _CASES:
        cfg = A.config(H, W, 2, CLASSES, batchnorm)
        x, y, _ = A.synthetic_batch(cfg, B, f"gpu{H}x{W}")
        y[B - 1] = [0.1, 0.5, 0.0, 0.7, 0.2]                  # a soft row that does not sum to 1
        params = A.keep_clear_of_flat_biases(cfg, A.init_params(cfg, f"gpu{H}{batchnorm}"), x)
        mask = ((np.random.RandomState(7).uniform(size=(B, 256)) >= 0.5) / 0.5).astype(np.float32)
        _CASES[key] = (cfg, params, x, y, mask)
    return _CASES[key]


def _check_step(eng, got_loss, ref, what):
    loss, ce, probs, z, ok, grads = ref
    assert abs(got_loss - loss) <= 1e-5 * abs(loss), (what, got_loss, loss)
    assert float((eng.probs.double().cpu() - probs).abs().max()) <= 1e-4, what
    assert float(eng.acc_out[0]) == ok and float(eng.reg_out[0]) == 0.0, what
    g_h = {k: v.double().cpu() for k, v in eng.export_keras_grads().items()}
    for n, gx in grads.items():
        e = float((g_h[n] - gx).abs().max())
        assert e <= 1e-3 * float(gx.abs().max()) + 1e-9, (what, n, e)


def _ref_update(kind, p64, grads, state, t, lr, lamb=None):
    if kind == "lamb":
        names = list(p64)
        vs = [(torch.tensor(p64[n]), grads[n], state["m"][n], state["v"][n], (True, True)) for n in names]
        out = lamb_ref.step(vs, lr, lamb.beta_1, lamb.beta_2, lamb.epsilon, lamb.weight_decay, t=t)
        for n, o in zip(names, out):
            p64[n], state["m"][n], state["v"][n] = o["w"].numpy(), o["m"], o["v"]
        return
    for n in p64:
        w, g = torch.tensor(p64[n]), grads[n]
        if kind == "adam":
            new, state["m"][n], state["v"][n] = R.adam_update(w, g, state["m"][n], state["v"][n], t, lr)
        elif kind == "sgd":
            new = R.sgd_update(w, g, lr)
        else:
            new, state["m"][n], state["v"][n], ms = R.nadam_update(w, g, state["m"][n], state["v"][n], t, lr, state["ms"])
            state["ms_next"] = ms
        p64[n] = new.numpy()
    if kind == "nadam":
        state["ms"] = state["ms_next"]


@pytest.mark.parametrize("batchnorm", [True, False], ids=["bn", "nobn"])
@pytest.mark.parametrize("kind", ["adam", "nadam", "sgd", "lamb", "adam-valid-kernels-only"])
def test_two_steps_against_the_restatement(U, kind, batchnorm):
    """By default the passes the measured record gives to the 'same' kernels run composed from them; valid_kernels_only=True keeps
    every pass on csrc/cnn_clas.hip.  Both are held to the restatement."""
    H, W, B, lr = 21, 24, 3, 1e-3
    cfg, params, x, y, mask = _case(H, W, B, batchnorm)
    only = kind.endswith("valid-kernels-only")
    kind = kind.split("-")[0]
    eng = U.DeepCNNEngine(H, W, B, classes=CLASSES, batchnorm=batchnorm, device=DEV, valid_kernels_only=only)
    assert eng.twin_passes == {"Conv0_A": (False, False), "Conv1_A": (False, not only), "Conv0_C": (not only, not only)}
    eng.load_keras_params(params)
    assert sorted(eng.specs) == sorted(A.param_shapes(cfg)) and eng.n_params() == A.n_params(cfg)
    lamb = U.LAMB(learning_rate=lr) if kind == "lamb" else None
    tr = U.Trainer(eng, lr=lr, optimizer=lamb if lamb is not None else kind)
    tx, ty, tm = torch.tensor(x).to(DEV), torch.tensor(y).to(DEV), torch.tensor(mask).to(DEV).view(B, 1, 1, -1)
    p64 = {k: np.asarray(v, np.float64) for k, v in params.items()}
    state = {"m": {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()},
             "v": {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in p64.items()}, "ms": 1.0}
    for t in (1, 2):
        ref = A.loss_and_grads(p64, x, y, cfg, mask=mask)
        got = tr.step(tx, None, ty, dropout_mask=tm, return_loss=True)
        torch.cuda.synchronize()
        _check_step(eng, got, ref, (kind, t))
        _ref_update(kind, p64, ref[5], state, t, lr, lamb)
    assert float(eng.p["dense_1.kernel"][CLASSES:].abs().max()) == 0.0 and float(eng.p["Conv0_A.kernel"][..., 2:].abs().max()) == 0.0


def test_one_step_at_the_models_own_size(U):
    H, W, B = 144, 160, 4
    cfg, params, x, y, mask = _case(H, W, B)
    eng = U.DeepCNNEngine(H, W, B, classes=CLASSES, device=DEV)
    eng.load_keras_params(params)
    assert eng.n_params() == 42101 and sum(b.numel() for b in eng.moving.values()) == 736
    assert [(n.a.H, n.a.W) for n in eng.nodes[1:6]] == [(142, 158), (71, 79), (69, 77), (34, 38), (32, 36)]
    tr = U.Trainer(eng, lr=1e-3)
    got = tr.step(torch.tensor(x).to(DEV), None, torch.tensor(y).to(DEV), dropout_mask=torch.tensor(mask).to(DEV).view(B, 1, 1, -1),
                  return_loss=True)
    torch.cuda.synchronize()
    _check_step(eng, got, A.loss_and_grads(params, x, y, cfg, mask=mask), "144x160")


def _engine(U, overlap=False):
    eng = U.DeepCNNEngine(21, 24, 3, classes=CLASSES, device=DEV, overlap_wgrad=overlap)
    eng.reset_parameters(torch.Generator().manual_seed(3))
    eng.dropout_seed = 77
    return eng


def _batches(n, B=3):
    gen = torch.Generator(); gen.manual_seed(5)
    out = []
    for _ in range(n):
        y = torch.zeros((B, CLASSES))
        y[torch.arange(B), torch.randint(0, CLASSES, (B,), generator=gen)] = 1.0
        out.append((torch.rand((B, 2, 21, 24), generator=gen).to(DEV), None, y.to(DEV)))
    return out


def _state(eng):
    return (eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}, eng.adam_t,
            eng._shared["dropout_step"])


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("overlap", [False, True])
def test_three_steps_twice_from_the_same_seed_are_bit_identical(U, overlap):
    data = _batches(3)
    res = []
    for _ in range(2):
        eng = _engine(U, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng.probs.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 3 and all(math.isfinite(v) for v in res[0][0])          # one Dropout draw per step


def test_graph_replay_is_the_same_step(U):
    """Trainer(graph=True) replays three steps bit-identical to three ordinary steps with the counters in device memory, Dropout on."""
    data = _batches(3)
    res = []
    for mode in ("graph", "eager_dev"):
        eng = _engine(U)
        tr = U.Trainer(eng, lr=1e-3, graph=(mode == "graph"))
        if mode == "eager_dev":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng.probs.clone(), eng.acc_out.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 3 and eng.masks["fc"] is not None


def test_inference_rows_sum_to_one(U):
    eng = _engine(U)
    eng.training = False
    (x, _, _), = _batches(1)
    p = eng.forward(x)
    torch.cuda.synchronize()
    assert tuple(p.shape) == (3, CLASSES) and float((p.double().sum(1) - 1).abs().max()) <= 2.0 ** -22 * CLASSES
    assert float(p.min()) > 0


def test_fit_reports_the_accuracy_of_a_host_recount(U):
    """One epoch of four synthetic batches at a zero rate (the parameters stay, so the pass can be repeated): train_acc equals the
    count of argmax(probs) == label over the same batches, and the validation column the same over its batches."""
    eng = _engine(U)
    tr = U.Trainer(eng, lr=0.0, dropout=False)
    data = _batches(4)
    rec = U.fit(tr, lambda ep: data, 1, val_batches=lambda ep: data[:2], log=None, val_updates_moving=False)[0]
    ok = 0
    for x, _, y in data:
        p = eng.forward(x, target=y).clone()
        torch.cuda.synchronize()
        ok += int((torch.argmax(p, 1) == torch.argmax(y, 1)).sum())
    ok_v = 0
    for x, _, y in data[:2]:
        ok_v += int((torch.argmax(eng.forward(x, target=y), 1) == torch.argmax(y, 1)).sum())
    assert rec["train_acc"] == ok / 12 and rec["val_acc"] == ok_v / 6 and rec["train_phase"] == 0.0
    assert rec["train_amp"] > 0 and abs(rec["train_loss"] - rec["train_amp"]) <= 1e-5 * rec["train_amp"]


def test_deep_cnn_class_on_the_device(U, tmp_path):
    model = U.deep_CNN(21, 24, 2, CLASSES, True, "adam", 1e-3, batch_size=3, device=DEV)
    model.build_model()
    model.set_optimizer_criterion()
    net, opt, crit = model.return_params()
    (x, _, y), = _batches(1)
    a = net(x.permute(0, 2, 3, 1).contiguous()).clone()
    model.save(str(tmp_path))
    again = U.deep_CNN.load(str(tmp_path), batch_size=3, device=DEV)
    assert torch.equal(again.engine.theta, model.engine.theta) and torch.equal(again.model(x), a)
    tr = U.Trainer(model, optimizer=opt, lr=model.learning_rate)
    assert math.isfinite(tr.step(x, None, y, return_loss=True)) and tuple(crit(y, a).shape) == (3,)
