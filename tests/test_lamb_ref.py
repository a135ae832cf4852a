"""tests/lamb_ref.py (the pin of the LAMB kernels: tfa.optimizers.LAMB, trainer.py:37-38, PARITY UNPINNED) held to a second form:
a per-variable loop written literally from the five lines of the arithmetic, one scalar norm at a time."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_ref  # noqa: E402

D = torch.float64


def literal(variables, t, lr, b1, b2, eps, wd, gs):
    out = []
    for w, g, m, v, (decayed, adapted) in variables:
        w, g, m, v = w.double(), g.double() * gs, m.double(), v.double()
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g ** 2
        mh = m / (1 - b1 ** t)
        vh = v / (1 - b2 ** t)
        u = mh / (vh.sqrt() + eps)
        if decayed:
            u = u + wd * w
        nw, nu = math.sqrt(float((w ** 2).sum())), math.sqrt(float((u ** 2).sum()))
        r = nw / nu if (adapted and nw > 0 and nu > 0) else 1.0
        out.append((w - lr * r * u, m, v, r))
    return out


def _vars(seed=0):
    g = torch.Generator(); g.manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=D)
    v = []
    for shape, flags in (((7,), (True, True)), ((3, 5, 2), (True, True)), ((64,), (False, False)), ((130,), (True, False)), ((9, 9), (False, True))):
        v.append((rn(*shape), rn(*shape) * 0.1, rn(*shape) * 0.01, rn(*shape).abs() * 0.01, flags))
    return v


def _same(got, want):
    for a, (w, m, v, r) in zip(got, want):
        assert float((a["w"] - w).abs().max()) <= 1e-14 * (1 + float(w.abs().max()))
        assert float((a["m"] - m).abs().max()) <= 1e-15 and float((a["v"] - v).abs().max()) <= 1e-15
        assert abs(a["r"] - r) <= 1e-13 * abs(r)


@pytest.mark.parametrize("t", [1, 2, 1000])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restatement_equals_the_literal_loop(t, wd):
    v = _vars(t)
    got = lamb_ref.step(v, 1e-3, 0.9, 0.999, 1e-6, wd, t=t, grad_scale=0.5)
    _same(got, literal(v, t, 1e-3, 0.9, 0.999, 1e-6, wd, 0.5))
    assert all(a["w"].shape == x[0].shape for a, x in zip(got, v))


def test_corner_cases():
    g = torch.Generator(); g.manual_seed(3)
    rn = lambda n: torch.randn(n, generator=g, dtype=D)
    z = torch.zeros(50, dtype=D)
    v = [(z, rn(50), z, z, (True, True)),                      # w == 0: ||w|| = 0 -> r = 1, the variable still moves by lr u
         (rn(50), z, z, z, (False, True)),                     # g == 0 and zero moments, not decayed: u == 0 -> r = 1, w stays
         (rn(50), rn(50), z, z, (False, False)),               # excluded from decay and from layer adaptation: r = 1, no decay term
         (rn(50), rn(50), z, z, (True, True))]                 # weight_decay > 0 enters u and through it the ratio
    got = lamb_ref.step(v, 0.1, 0.9, 0.999, 1e-6, 0.05, t=1)
    _same(got, literal(v, 1, 0.1, 0.9, 0.999, 1e-6, 0.05, 1.0))
    assert got[0]["r"] == 1.0 and float(got[0]["w"].abs().max()) > 0
    assert got[1]["r"] == 1.0 and torch.equal(got[1]["w"], v[1][0]) and float(got[1]["u"].abs().max()) == 0
    assert got[2]["r"] == 1.0
    # at t = 1 the update of an undecayed variable is g / (|g| + eps): the step of the excluded variable is lr sign(g) nearly everywhere
    assert float((got[2]["w"] - (v[2][0] - 0.1 * v[2][1] / (v[2][1].abs() + 1e-6))).abs().max()) <= 1e-12
    nodecay = lamb_ref.step([v[3][:4] + ((False, True),)], 0.1, 0.9, 0.999, 1e-6, 0.05, t=1)[0]
    assert float((got[3]["u"] - nodecay["u"] - 0.05 * v[3][0]).abs().max()) <= 1e-15 and got[3]["r"] != nodecay["r"]
    # the trust ratio makes the step's length lr ||w|| whatever the gradient's scale
    assert abs(float((got[3]["w"] - v[3][0]).norm()) - 0.1 * float(v[3][0].norm())) <= 1e-12


def test_corrections():
    c1, c2 = lamb_ref.corrections(0.9, 0.999, 3)
    assert abs(c1 - (1 - 0.729)) <= 1e-15 and abs(c2 - (1 - 0.999 ** 3)) <= 1e-15
