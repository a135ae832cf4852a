"""resize_factor_0 = [2, 2] (dl_models/u_net.py:213, :247-248) through the PRODUCT's UNet / UNetEngine / UNetGraphEngine / Trainer on CPU
tensors: only the kernels (tests/head_up2_cpu_ops.py over tests/cpu_ops.py, fp64 arithmetic) and the stream runtime
(tests/sim_runtime.py: vector clocks + race check) are stand-ins.  The reference is tests/head_up2_ref.unet_loss_and_grads - the
oracle's own blocks with the literal up-sampling in front of the head - at the tolerances of tests/test_schedule_sim.py (fp32 buffers,
fp64 arithmetic): loss 1e-5 relative, gradients 1e-4 of the tensor's largest entry."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H = W = 32
F0, DEPTH, B = 8, 3, 2


def _install(monkeypatch):
    import head_up2_cpu_ops
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    return rt, head_up2_cpu_ops.install(monkeypatch, rt)


def _engine(U, rt, kind, overlap, s0=2, h=H, w=W, depth=DEPTH, batch=B, dtype="f32", f0=F0):
    if kind == "unet":
        return U.UNetEngine(h, w, batch, F0=f0, k=3, depth=depth, s0=s0, device="cpu", runtime=rt, overlap_wgrad=overlap, dtype=dtype)
    return U.UNetGraphEngine(h, w, batch, F0=f0, k=3, depth=depth, mode=int(kind[-1]), s0=s0, device="cpu", runtime=rt,
                             overlap_wgrad=overlap, dtype=dtype)


@pytest.mark.parametrize("kind,overlap", [("unet", False), ("unet", True), ("graph0", False), ("graph0", True), ("graph2", True)])
def test_full_step_at_half_resolution_matches_the_restatement(monkeypatch, kind, overlap):
    """One Trainer step: loss, prediction and every gradient equal the restatement's, and no cross-stream access is unordered (a
    missing happens-before edge raises sim_runtime.RaceError)."""
    import unet_rir_amd as U
    import head_up2_ref as HR
    from oracle import torch_ref as R
    rt, impl = _install(monkeypatch)
    cfg = R.Config(H, W, F0, 3, depth=DEPTH, s0=2, mode=0 if kind == "unet" else int(kind[-1]))
    params = R.init_params(cfg, f"s0{kind}", randomize_all=True, dtype=np.float64)
    spec_in, emb, spec_out = R.synthetic_batch(cfg, B, "s0/d")
    loss, pred, grads = HR.unet_loss_and_grads(params, spec_in, emb, spec_out, cfg)
    eng = _engine(U, rt, kind, overlap)
    eng.load_keras_params(params)
    tr = U.Trainer(eng, lr=1e-3, dropout=False)
    t = lambda a: torch.tensor(np.asarray(a))
    got = tr.step(t(spec_in).float(), t(emb), t(spec_out).float(), return_loss=True)
    assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
    assert float((eng.pred.double() - pred).abs().max()) <= 1e-5
    kg = eng.export_keras_grads()
    assert set(kg) == set(grads)
    for n, g in grads.items():
        err = float((kg[n].double() - g).abs().max())
        assert err <= 1e-4 * float(g.abs().max()) + 1e-12, (n, err)
    c = dict(impl.head_up2.calls)
    assert c["fwd"] == 1 and c["dgrad"] == 1 and c["wgrad"] == 1 and c["fold"] >= 1          # the head ran on the folded entry points
    # the work copy follows the optimizer: a second forward pass reads the fold of the kernel the first step's Adam left
    eng.forward(t(spec_in).float(), t(emb))
    assert impl.head_up2.calls["fold"] == c["fold"] + 1 and impl.head_up2.calls["fwd"] == 2
    assert torch.equal(eng.pf["head.kernel"].view(8, 4, 4, F0), HR.fold(eng.p["head.kernel"][:2].float(), torch.float32))


def _buffers(eng):
    """Every activation / gradient buffer an engine holds: the Acts among its attributes and in its dicts, the nodes of a graph."""
    from unet_rir_amd.ops import Act
    seen = {}

    def add(a):
        if isinstance(a, Act):
            seen[a.base.data_ptr()] = a.base
    for v in vars(eng).values():
        add(v)
        if isinstance(v, dict):
            for x in v.values():
                add(x)
    for n in getattr(eng, "nodes", ()):
        add(n.a); add(n.g)
    return list(seen.values())


@pytest.mark.parametrize("kind", ["unet", "graph0", "graph3"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_no_full_resolution_feature_tensor_exists(monkeypatch, kind, dtype):
    import unet_rir_amd as U
    rt, _ = _install(monkeypatch)
    h = w = 64
    # bf16 storage keeps dL/dlogits as [B,H,W,8] (the loss kernels' layout, at either factor): as large as a feature tensor of 8
    # channels, so the bf16 engines are built with 16 filters
    f0 = F0 if dtype == "f32" else 16
    half, full = (_engine(U, rt, kind, False, s0, h, w, 4, dtype=dtype, f0=f0) for s0 in (2, 1))
    limit = B * h * w * f0
    assert max(b.numel() for b in _buffers(half)) < limit
    assert max(b.numel() for b in _buffers(full)) >= limit                     # the walk does see the buffers
    assert len(_buffers(half)) >= 0.9 * len(_buffers(full))
    # the parameters are those of the full-resolution model, except the Dense layer that feeds the (smaller) bottleneck
    sh = lambda e: {n: (s.shape, s.keras_shape, s.kind) for n, s in e.specs.items() if not n.startswith("vec.dense")}
    assert sh(half) == sh(full) and list(half.specs) == list(full.specs)
    assert half.vec_dim * 4 == full.vec_dim
    assert half.specs["vec.dense.kernel"].keras_shape == (full.specs["vec.dense.kernel"].keras_shape[0], half.vec_dim)
    assert half.specs["head.kernel"].keras_shape == (6, 6, f0, 2) and half.pred.shape == (B, 2, h, w)
    assert [s.offset for n, s in half.specs.items()][:2] == [s.offset for n, s in full.specs.items()][:2]       # bucket layout: head first


def test_unet_honours_resize_factor_0(monkeypatch, tmp_path):
    import unet_rir_amd as U
    rt, _ = _install(monkeypatch)
    kw = dict(number_filters_0=8, runtime=rt, device="cpu")
    model = U.UNet((64, 64, 2), (2, 16), resize_factor_0=[2, 2], **kw)
    assert isinstance(model.engine, U.UNetEngine) and model.engine.s0 == 2 and model.engine.hw[0] == (32, 32)
    assert model.resize_factor_0 == [2, 2] and U.UNet((64, 64, 2), (2, 16), resize_factor_0=[1, 1], **kw).engine.s0 == 1
    assert U.UNet((64, 64, 2), (2, 16), **kw).engine.s0 == 1
    g = U.UNet((64, 64, 2), (2, 16), mode=2, resize_factor_0=(2, 2), kernels=3, **kw)
    assert isinstance(g.engine, U.UNetGraphEngine) and g.engine.s0 == 2
    for bad in (dict(resize_factor_0=[2, 1]), dict(resize_factor_0=[3, 3]), dict(resize_factor_0=[4, 4]), dict(res_factor=[1, 1]),
                dict(resize_factor_0=[2, 2], res_factor=[4, 4])):
        with pytest.raises(NotImplementedError, match=r"\[1, 1\].*\[2, 2\]"):
            U.UNet((64, 64, 2), (2, 16), **bad, **kw)
    for cls in (U.AENet, U.DiffUNet):                                            # other first level, other head: out of scope
        with pytest.raises(NotImplementedError):
            cls((64, 64, 2), (2, 16), resize_factor_0=[2, 2], **kw)
    # the reference's own 144 x 160: 2 * 2^4 = 32 does not divide 144, 2 * 2^3 = 16 divides both
    with pytest.raises(ValueError, match="multiples of"):
        U.UNet((144, 160, 2), (2, 16), resize_factor_0=[2, 2], depth=4, kernels=3, **kw)
    with pytest.raises(ValueError, match="multiples of"):
        U.UNet((144, 160, 2), (2, 16), resize_factor_0=[2, 2], depth=4, mode=1, kernels=3, **kw)
    assert U.UNet((144, 160, 2), (2, 16), resize_factor_0=[2, 2], depth=3, kernels=3, **kw).engine.hw[-1] == (9, 10)
    with pytest.raises(ValueError):
        U.UNetEngine(64, 64, 1, F0=4, s0=2, device="cpu", runtime=rt)            # the folded head needs F0 % 8 == 0
    # save -> load keeps the factor; a parameters.pkl from before it existed loads as [1, 1]
    x = [torch.rand(1, 64, 64, 2), torch.randint(0, 2000, (1, 2, 16))]
    want = model.predict_stft(x)
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        prm = pickle.load(f)
    assert prm[8:] == ["f32", [2, 2]]
    again = U.UNet.load(str(tmp_path), device="cpu", runtime=rt)
    assert again.resize_factor_0 == [2, 2] and again.engine.s0 == 2 and torch.equal(again.engine.theta, model.engine.theta)
    assert torch.equal(again.predict_stft(x), want)
    old = U.UNet((64, 64, 2), (2, 16), **kw)
    old.save(str(tmp_path / "old"))
    with open(tmp_path / "old" / "parameters.pkl", "rb") as f:
        prm = pickle.load(f)
    with open(tmp_path / "old" / "parameters.pkl", "wb") as f:
        pickle.dump(prm[:9], f)
    assert U.UNet.load(str(tmp_path / "old"), device="cpu", runtime=rt).resize_factor_0 == [1, 1]


def test_inference_uses_the_moving_statistics(monkeypatch):
    """training=False at s0 = 2: BatchNorm with the moving statistics, through the folded head."""
    import unet_rir_amd as U
    import head_up2_ref as HR
    from oracle import torch_ref as R
    rt, _ = _install(monkeypatch)
    cfg = R.Config(H, W, F0, 3, depth=DEPTH, s0=2)
    params = R.init_params(cfg, "s0inf", randomize_all=True, dtype=np.float64)
    spec_in, emb, _ = R.synthetic_batch(cfg, B, "s0/i")
    eng = _engine(U, rt, "unet", False)
    eng.load_keras_params(params)
    state = {}
    for i, b in enumerate(eng.bn_names):
        c = eng.moving[b + ".moving_mean"].numel()
        eng.moving[b + ".moving_mean"].copy_(torch.linspace(-0.2, 0.3, c) + 0.01 * i)
        eng.moving[b + ".moving_variance"].copy_(torch.linspace(0.5, 1.5, c))
        state[b] = (eng.moving[b + ".moving_mean"].double().clone(), eng.moving[b + ".moving_variance"].double().clone())
    eng.training = False
    got = eng.forward(torch.tensor(spec_in).float(), torch.tensor(emb))
    P = R.to_torch(params, torch.float64)
    bn_state = {}
    for b, (m, v) in state.items():
        bn_state[b + ".moving_mean"], bn_state[b + ".moving_variance"] = m, v
    want = HR.unet_forward(P, torch.tensor(spec_in).double(), torch.tensor(emb), cfg, False, None, bn_state)
    assert float((got.double() - want).abs().max()) <= 1e-5
