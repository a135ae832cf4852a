"""tests/cnn_clas_ref.py, the restatement of deep_CNN (dl_models/cnn_clas.py:19-53), is held to autograd of the literal library
expressions, to finite differences and to the parameter count of the source's model."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cnn_clas_ref as A

H, W, B = 21, 24, 3


def _literal_loss(P, x, y, cfg, mask, gb):
    for i, name in enumerate(A.CONV_NAMES):
        x = F.relu(F.conv2d(x, P[name + ".kernel"].permute(3, 2, 0, 1), P[name + ".bias"], padding=0))
        if cfg.batchnorm:
            x = F.batch_norm(x, None, None, P[f"bn{i}.gamma"], P[f"bn{i}.beta"], training=True, eps=1e-3)
        x = F.avg_pool2d(x, 2) if i < 2 else x.mean((2, 3))
    x = F.relu(x @ P["dense.kernel"] + P["dense.bias"])
    if cfg.batchnorm:
        x = F.batch_norm(x, None, None, P["bn3.gamma"], P["bn3.beta"], training=True, eps=1e-3)
    z = (x * mask) @ P["dense_1.kernel"] + P["dense_1.bias"]
    return -(y * F.log_softmax(z, 1)).sum() / gb, z


def _case(batchnorm):
    cfg = A.config(H, W, 2, 5, batchnorm)
    params = A.init_params(cfg, f"ref{batchnorm}")
    x, y, _ = A.synthetic_batch(cfg, B, "ref/d")
    y[1] = [0.1, 0.5, 0.0, 0.7, 0.2]                       # a soft row that does not sum to 1
    mask = ((np.random.RandomState(3).uniform(size=(B, 256)) >= 0.5) / 0.5).astype(np.float64)
    return cfg, params, x, y, mask


def test_parameter_count_of_the_source_model():
    cfg = A.config(144, 160, 2, 5, True)
    shapes = A.param_shapes(cfg)
    per_layer = [sum(int(np.prod(shapes[n])) for n in shapes if n.startswith(p + ".")) for p in
                 ("Conv0_A", "bn0", "Conv1_A", "bn1", "Conv0_C", "bn2", "dense", "bn3", "dense_1")]
    assert per_layer == [304, 32, 4640, 64, 18496, 128, 16640, 512, 1285]
    assert A.n_params(cfg) == 42101
    assert sum(int(np.prod(s)) for s in A.moving_shapes(cfg).values()) == 736
    assert A.n_params(A.config(144, 160, 2, 5, False)) == 42101 - 736


def test_sizes_at_the_source_geometry_and_at_the_test_geometry():
    for (h, w), want in (((144, 160), [(142, 158), (71, 79), (69, 77), (34, 38), (32, 36)]), ((21, 24), [(19, 22), (9, 11), (7, 9), (3, 4), (1, 2)])):
        x, got = torch.zeros(1, 1, h, w, dtype=torch.float64), []
        k, b = torch.zeros(3, 3, 1, 1, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
        for i in range(3):
            x = A.conv_valid(x, k, b)
            got.append(tuple(x.shape[2:]))
            if i < 2:
                x = A.avg_pool2(x)
                got.append(tuple(x.shape[2:]))
        assert got == want


@pytest.mark.parametrize("batchnorm", [True, False])
def test_restatement_equals_autograd_of_the_literal_expressions(batchnorm):
    cfg, params, x, y, mask = _case(batchnorm)
    loss, ce, probs, z, ok, grads = A.loss_and_grads(params, x, y, cfg, mask=mask, global_batch=2 * B)
    P = A.to_torch(params, torch.float64, True)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    lit, zl = _literal_loss(P, t(x), t(y), cfg, t(mask), 2 * B)
    lit.backward()
    assert abs(loss - float(lit)) <= 1e-12 * abs(float(lit)) and abs(ce - 2 * B * loss) <= 1e-12 * ce
    assert float((z - zl.detach()).abs().max()) <= 1e-11
    assert float((probs.sum(1) - 1).abs().max()) <= 1e-14
    for n, g in grads.items():
        e = float((g - P[n].grad).abs().max())
        assert e <= 1e-10 * float(P[n].grad.abs().max()) + 1e-15, (n, e)
        assert float(g.abs().max()) > 0, n


@pytest.mark.parametrize("batchnorm", [True, False])
def test_gradients_match_finite_differences(batchnorm):
    cfg, params, x, y, mask = _case(batchnorm)
    _, _, _, _, _, grads = A.loss_and_grads(params, x, y, cfg, mask=mask)
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)

    def loss_of(p):
        z = A.logits(A.to_torch(p), t(x), cfg, mask=t(mask))
        return float(A.cross_entropy_rows(z, t(y)).sum() / B)

    rs, h = np.random.RandomState(0), 1e-6
    gmax = max(float(g.abs().max()) for g in grads.values())
    for n, w in params.items():
        for _ in range(4):
            idx = tuple(int(rs.randint(s)) for s in w.shape)
            hi, lo = {k: v.copy() for k, v in params.items()}, {k: v.copy() for k, v in params.items()}
            hi[n][idx] += h
            lo[n][idx] -= h
            fd = (loss_of(hi) - loss_of(lo)) / (2 * h)
            assert abs(fd - float(grads[n][idx])) <= 1e-5 * abs(fd) + 1e-7 * gmax, (n, idx, fd, float(grads[n][idx]))


def test_accuracy_takes_the_lowest_index_on_ties():
    z = torch.tensor([[1.0, 3.0, 3.0], [2.0, 2.0, 2.0], [0.0, 1.0, 5.0]], dtype=torch.float64)
    y = torch.tensor([[0.0, 1.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.5, 0.5]], dtype=torch.float64)
    assert A.n_correct(z, y) == 2                  # rows 0 and 1; row 2: argmax z = 2, argmax y = 1


def test_moving_statistics_follow_the_keras_update():
    cfg, params, x, y, mask = _case(True)
    state = {n: (torch.ones(s, dtype=torch.float64) if n.endswith("variance") else torch.zeros(s, dtype=torch.float64))
             for n, s in A.moving_shapes(cfg).items()}
    P = A.to_torch(params)
    xt = torch.tensor(x, dtype=torch.float64)
    A.logits(P, xt, cfg, bn_state=state)
    r = torch.relu(A.conv_valid(xt, P["Conv0_A.kernel"], P["Conv0_A.bias"]))
    n = r.numel() // 16
    assert torch.allclose(state["bn0.moving_mean"], 0.01 * r.mean((0, 2, 3)), rtol=1e-12, atol=0)
    assert torch.allclose(state["bn0.moving_variance"], 0.99 + 0.01 * r.var((0, 2, 3), unbiased=False) * n / (n - 1), rtol=1e-12, atol=0)
