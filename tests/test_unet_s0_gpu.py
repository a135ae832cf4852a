"""The half-resolution U-Net (resize_factor_0 = [2, 2], dl_models/u_net.py:213, :247-248) on the GPU: 64 x 64, 8 filters, depth 4,
batch 2.  fp32: prediction, loss and every gradient of UNetEngine and UNetGraphEngine (modes 0 and 2) against the restatement
tests/head_up2_ref.unet_loss_and_grads - oracle/torch_ref.py's own blocks with the literal up-sampling in front of the head - at the
tolerances of tests/test_model_gpu.py::test_forward_backward_vs_oracle.  bf16: the hand schedule against the graph executor (mode 0)
to the standard of test_graph_engine_mode0_equals_hand_schedule.  Trainer steps of UNet(resize_factor_0=[2, 2]) are bit-identical
from run to run and as a replayed HIP graph; training=False reads the moving statistics."""
import functools

import numpy as np
import pytest
import torch

import head_up2_ref as HR
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = W = 64
F0, DEPTH, B = 8, 4, 2


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


@functools.lru_cache(maxsize=None)
def case(mode):
    cfg = R.Config(H, W, F0, 3, DEPTH, s0=2, mode=mode)
    params = R.init_params(cfg, f"s0gpu{mode}", randomize_all=True, dtype=np.float64)
    batch = R.synthetic_batch(cfg, B, "s0gpu/d")
    return cfg, params, batch, HR.unet_loss_and_grads(params, *batch, cfg)


def _engine(U, kind, dtype="f32", **kw):
    if kind == "unet":
        return U.UNetEngine(H, W, B, F0=F0, k=3, depth=DEPTH, s0=2, device=DEV, dtype=dtype, **kw)
    return U.UNetGraphEngine(H, W, B, F0=F0, k=3, depth=DEPTH, mode=int(kind[-1]), s0=2, device=DEV, dtype=dtype, **kw)


def _run(eng, params, batch):
    eng.load_keras_params(params)
    t = lambda a: torch.tensor(a).to(DEV)
    eng.forward(t(batch[0]), t(batch[1]), target=t(batch[2]), global_batch=B)
    eng.backward()
    eng.reg_loss()
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind", ["unet", "graph0", "graph2"])
def test_fp32_step_against_the_restatement(U, kind):
    cfg, params, batch, (loss, pred, grads) = case(0 if kind == "unet" else int(kind[-1]))
    eng = _engine(U, kind)
    assert eng.s0 == 2 and "head.kernel" in eng.pf
    _run(eng, params, batch)
    err = float((eng.pred.double().cpu() - pred).abs().max())
    assert err <= 1e-4, f"prediction max err {err}"
    got_loss = float(eng.loss_out[0]) + float(eng.reg_out[0])
    assert abs(got_loss - loss) <= 1e-5 * abs(loss), (got_loss, loss)
    kg = eng.export_keras_grads()
    assert set(kg) == set(grads)
    # biases in front of a BatchNorm have an analytically zero gradient: absolute floor relative to the largest gradient in the network
    floor = 1e-6 * max(float(g_.abs().max()) for g_ in grads.values())
    for n, g_ref in grads.items():
        g = kg[n].double()
        scale = float(g_ref.abs().max())
        e = float((g - g_ref).abs().max())
        assert e <= 1e-3 * scale + floor, f"grad {n}: err {e:.3e} scale {scale:.3e}"
        l2 = float((g - g_ref).norm()) / (float(g_ref.norm()) + 1e-30)
        assert l2 <= 1e-4 or e <= floor, f"grad {n}: relative L2 error {l2:.3e}"
    assert float(eng.p["head.kernel"][2:].abs().max()) == 0.0 and float(eng.g["head.kernel"][2:].abs().max()) == 0.0


def test_bf16_hand_schedule_equals_the_graph_executor(U):
    cfg, params, batch, _ = case(0)
    e1, e2 = _engine(U, "unet", "bf16"), _engine(U, "graph0", "bf16")
    for e in (e1, e2):
        _run(e, params, batch)
    d = float((e1.pred - e2.pred).abs().max())
    print("bf16 hand schedule vs graph executor: prediction differs by", d)
    assert d <= 1e-6
    g1, g2 = e1.export_keras_grads(), e2.export_keras_grads()
    for n in g1:
        e = float((g1[n] - g2[n]).abs().max())
        assert e <= 1e-6 * (float(g1[n].abs().max()) + 1e-12) + 1e-9, (n, e, float(g1[n].abs().max()))
    # the work copy the kernels read is the fold of the master kernel, rounded to bf16 once
    want = HR.fold_bf16(e1.p["head.kernel"][:2].cpu())
    assert torch.equal(e1.pf["head.kernel"].view(8, 4, 4, F0).double().cpu(), want)


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
             torch.rand((B, 2, H, W), generator=gen).to(DEV)) for _ in range(n)]


@pytest.mark.parametrize("dtype,overlap", [("bf16", True), ("f32", False)])
def test_trainer_steps_are_reproducible_and_replay_as_a_graph(U, dtype, overlap):
    """Three steps, dropout on: two runs that issue the launches one by one and one that replays the captured step end with the same
    bits (per-step scalars in device memory for all three, as tests/test_step_graph_gpu.py compares them)."""
    data = _batches(3)
    res = []
    for mode in ("eager", "eager", "graph"):
        model = U.UNet((H, W, 2), (2, 16), number_filters_0=F0, kernels=3, resize_factor_0=[2, 2], depth=DEPTH, batch_size=B, device=DEV,
                       dtype=dtype, overlap=overlap)
        eng = model.engine
        assert isinstance(eng, U.UNetEngine) and eng.s0 == 2
        g = torch.Generator(); g.manual_seed(3)
        eng.reset_parameters(g)
        eng.dropout_seed = 77
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, graph=(mode == "graph"))
        if mode == "eager":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}))
    for other, what in ((res[1], "second run"), (res[2], "graph replay")):
        assert other[0] == res[0][0], what
        for i in (1, 2, 3):
            assert torch.equal(other[i], res[0][i]), (what, i)
        for k in res[0][4]:
            assert torch.equal(other[4][k], res[0][4][k]), (what, k)
    assert all(np.isfinite(res[0][0]))


def test_inference_uses_the_moving_statistics(U):
    cfg, params, batch, _ = case(0)
    eng = _engine(U, "unet")
    eng.load_keras_params(params)
    bn_state = {}
    for i, b in enumerate(eng.bn_names):
        c = eng.moving[b + ".moving_mean"].numel()
        eng.moving[b + ".moving_mean"].copy_(torch.linspace(-0.2, 0.3, c) + 0.01 * i)
        eng.moving[b + ".moving_variance"].copy_(torch.linspace(0.5, 1.5, c))
        bn_state[b + ".moving_mean"] = eng.moving[b + ".moving_mean"].double().cpu()
        bn_state[b + ".moving_variance"] = eng.moving[b + ".moving_variance"].double().cpu()
    eng.training = False
    got = eng.forward(torch.tensor(batch[0]).to(DEV), torch.tensor(batch[1]).to(DEV))
    torch.cuda.synchronize()
    want = HR.unet_forward(R.to_torch(params, torch.float64), torch.tensor(batch[0]).double(), torch.tensor(batch[1]), cfg, False, None, bn_state)
    assert float((got.double().cpu() - want).abs().max()) <= 1e-4
    train = HR.unet_forward(R.to_torch(params, torch.float64), torch.tensor(batch[0]).double(), torch.tensor(batch[1]), cfg, True, None, None)
    assert float((want - train).abs().max()) > 1e-3                    # the two modes differ on this data
