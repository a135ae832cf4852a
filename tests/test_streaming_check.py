"""CPU proof of the element-wise criterion of tests/streaming_check.py: BatchNorm apply, the BatchNormalization -> Add -> LeakyReLU
junction and the BatchNorm backward are emulated in fp32 torch arithmetic the two ways a compiler may round them (`mul` + `add`,
or one fused multiply-add), with the statistics, the stored parameters and the bf16 / fp32 stores of csrc/elementwise.hip.  The
criterion must accept both, and reject each of six mutants; the tolerance the kernel tests used so far (1e-2 of the tensor's
largest value for bf16 tensors, 1e-4 for the per-channel sums) is evaluated beside it and accepts at least the first three."""
import numpy as np
import pytest
import torch

import streaming_check as S
from oracle import detrand

EPS = 1e-3
SLOPE32 = torch.tensor(0.3, dtype=torch.float32)


def make(tag, P, C, offset, bf16):
    """x with unit spread per channel: centred, or with a per-channel mean (bf16 storage: from [-4, 4]; fp32 storage: from [-8, 8],
    channel 1 at +100 and channel 2 at -100 with spread 0.5, channel 3 constant) - the data kinds of tests/test_streaming_gpu.py."""
    x = torch.tensor(detrand.uniform(f"scx{tag}", (P, C), -3 ** 0.5, 3 ** 0.5, np.float64))
    if offset:
        m = torch.tensor(detrand.uniform(f"scm{tag}", (C,), -1, 1, np.float64)) * (4 if bf16 else 8)
        x = x + m
        if not bf16:
            x[:, 1] = 100 + 0.5 * (x[:, 1] - m[1]); x[:, 2] = -100 + 0.5 * (x[:, 2] - m[2]); x[:, 3] = m[3]
    return x.to(torch.bfloat16) if bf16 else x.float()


def params(tag, C, x, narrow=False):
    w = 0.001 if narrow else 0.5
    gamma = (1 + w * torch.tensor(detrand.uniform(f"scg{tag}", (C,), -1, 1, np.float64))).float()
    beta = (0.5 * torch.tensor(detrand.uniform(f"scb{tag}", (C,), -1, 1, np.float64))).float()
    st = S.stats_ref(x, EPS)
    mean_f, rstd_f = st["mean"].float(), st["rstd"].float()          # saved[]: stored straight from doubles
    scale = gamma * rstd_f
    shift = beta - mean_f * scale
    return gamma, beta, st, mean_f, rstd_f, scale, shift


def store(r32, like, trunc=False):
    if like.dtype == torch.bfloat16:
        return S.bf16_trunc(r32).to(torch.bfloat16) if trunc else r32.to(torch.bfloat16)
    return r32


def emu_apply(x, scale, shift, addend, act, fused, slope=SLOPE32, trunc=False, swap=False):
    """bn_apply_kernel in fp32: r = x * scale + shift (two roundings or one), + addend, activation, store."""
    if swap:                                   # mutant: the second channel vector works with its neighbour's scale
        scale = scale.clone(); scale[8:16] = scale[16:24]
    if fused:
        r = (x.double() * scale.double() + shift.double()).float()
    else:
        r = x.float() * scale + shift
    if addend is not None:
        r = r + addend.float()
    if act:
        r = torch.where(r > 0, r, r * (slope if act == 2 else 0.0))
    return store(r, x, trunc)


def test_bf16_rne_rounds_once_and_to_even():
    v = torch.tensor(detrand.uniform("rne", (200000,), -300, 300, np.float64)).float()
    assert torch.equal(S.bf16_rne(v.double()), v.to(torch.bfloat16).double())          # fp32 values: torch rounds once too
    one = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -30, -(1 + 2.0 ** -8), 0.0, 2.0 ** -133, 3 * 2.0 ** -134],
                       dtype=torch.float64)
    want = torch.tensor([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, 0.0, 2.0 ** -133, 2 * 2.0 ** -133], dtype=torch.float64)
    assert torch.equal(S.bf16_rne(one), want)
    assert float(one[2].float().to(torch.bfloat16)) == 1.0                              # through fp32: the double rounding
    assert torch.equal(S.bf16_trunc(one[:4]), torch.tensor([1.0, 1 + 2.0 ** -7, 1.0, -1.0], dtype=torch.float64))


@pytest.mark.parametrize("P,C", [(4096, 64), (20000, 24)])
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("bf16", [True, False])
def test_apply_and_junction_forward_are_accepted_either_way_of_rounding(P, C, offset, bf16):
    tag = (P, C, offset, bf16)
    x = make(tag, P, C, offset, bf16)
    gamma, beta, st, mean_f, rstd_f, scale, shift = params(tag, C, x)
    ref, d = S.scale_ref(rstd_f, gamma); S.check(scale, ref, d, "scale")
    ref, d = S.shift_ref(mean_f, scale, beta); S.check(shift, ref, d, "shift")
    S.check(mean_f, st["mean"], st["d_mean"], "mean"); S.check(rstd_f, st["rstd"], st["d_rstd"], "rstd")
    add = make(("add",) + tag, P, C, offset, bf16)
    for act in (0, 1, 2):
        for addend in (None, add):
            ref, d = S.apply_ref(x, scale, shift, addend, act)
            for fused in (False, True):
                S.check(emu_apply(x, scale, shift, addend, act, fused), ref, d, f"apply {tag} act {act} fused {fused}", "(cpu proof)", act)


def test_forward_mutants_are_rejected_and_the_old_tolerance_accepts_them(capsys):
    P, C = 20000, 24
    x = make("fm", P, C, True, True)
    gamma, beta, st, mean_f, rstd_f, scale, shift = params("fm", C, x, narrow=True)
    skip = (make("fms", P, C, False, True).float() + 3).to(torch.bfloat16)           # the Add's other operand: a positive-mean tensor
    ref, d = S.apply_ref(x, scale, shift, skip, 2)
    want = S.activate(ref, 2)
    good = emu_apply(x, scale, shift, skip, 2, False)
    assert S.accepts(good, ref, d, 2) and S.old_close(good, want, 1e-2)
    mutants = {"truncating bf16 store": emu_apply(x, scale, shift, skip, 2, False, trunc=True),
               "a channel vector with its neighbour's scale": emu_apply(x, scale, shift, skip, 2, False, swap=True),
               "LeakyReLU slope 0.25": emu_apply(x, scale, shift, skip, 2, False, slope=torch.tensor(0.25))}
    for name, got in mutants.items():
        new, old = S.accepts(got, ref, d, 2), S.old_close(got, want, 1e-2)
        wrong = float((got.double() != good.double()).double().mean())
        with capsys.disabled():
            print(f"\n  mutant '{name}': {wrong:.1%} of the elements differ from the good kernel's; element-wise criterion "
                  f"{'accepts' if new else 'rejects'}, close(1e-2) {'accepts' if old else 'rejects'}")
        assert not new, name
        assert old, name


def emu_bwd(x, da, mask, scale, mean_f, rstd_f, act, fused, gskip_add=None, drop_rows=0, mean64=None, forget_add=False):
    """chan_partial_kernel<2> + bn_bwd_finalize_kernel + bn_bwd_apply_kernel (junction form) in fp32."""
    P = x.shape[0]
    gv = da.float()
    g = torch.where(mask, gv, gv * (SLOPE32 if act == 2 else 0.0)) if act else gv
    if mean64 is None:
        xh = (x.float() - mean_f) * rstd_f
    else:                                       # mutant: xhat from the unrounded mean instead of the stored one
        xh = (x.double() - mean64).float() * rstd_f
    s = g.double().sum(0)
    ss = (g.double() * xh.double())[drop_rows:].sum(0)          # mutant: one slab's rows missing from the second sum
    dbeta, dgamma = s.float(), ss.float()
    c1, c2 = (s / P).float(), (ss / P).float()
    if fused:
        t = ((g - c1).double() - xh.double() * c2.double()).float()
    else:
        t = (g - c1) - xh * c2
    dx = store(scale * t, x)
    gs = g if (gskip_add is None or forget_add) else g + gskip_add.float()
    return dx, store(gs, x), dgamma, dbeta


def bwd_case(tag, P, C, bf16, act):
    x = make(tag, P, C, True, bf16)
    gamma, beta, st, mean_f, rstd_f, scale, shift = params(tag, C, x)
    skip = make(("s",) + tag, P, C, False, bf16)
    out = emu_apply(x, scale, shift, skip, act, False)
    # output gradient with a mean and a part that follows xhat, so that both per-channel means of the backward are far from 0
    xh = (x.double() - st["mean"]) * st["rstd"]
    da = 0.5 + 0.5 * xh + torch.tensor(detrand.uniform(f"scd{tag}", (P, C), -1, 1, np.float64))
    da = da.to(torch.bfloat16) if bf16 else da.float()
    acc = make(("a",) + tag, P, C, False, bf16)
    return x, da, out > 0, scale, mean_f, rstd_f, st, acc


def bwd_verdict(x, da, mask, scale, mean_f, rstd_f, act, acc, got):
    """Which of the four outputs the criterion rejects (empty: accepted)."""
    dx, gs, dgamma, dbeta = got
    P = x.shape[0]
    r = S.bwd_ref(x, da, mask, scale, mean_f, rstd_f, act)
    bad = []
    if not S.accepts(dbeta, r["dbeta"], r["d_dbeta"]): bad.append("dbeta")
    if not S.accepts(dgamma, r["dgamma"], r["d_dgamma"]): bad.append("dgamma")
    ref, d = S.dx_ref(r, scale, dbeta, dgamma, P)
    if not S.accepts(dx, ref, d): bad.append("dx")
    try:
        S.check_interval(gs, *S.gskip_interval(da, mask, act, acc), "gskip", "(cpu proof)")
    except AssertionError:
        bad.append("gskip")
    return bad, r


@pytest.mark.parametrize("bf16", [True, False])
@pytest.mark.parametrize("act", [1, 2])
def test_backward_is_accepted_either_way_of_rounding_and_its_mutants_are_rejected(bf16, act, capsys):
    P, C = 20000, 24
    x, da, mask, scale, mean_f, rstd_f, st, acc = bwd_case((P, C, bf16, act), P, C, bf16, act)
    args = (x, da, mask, scale, mean_f, rstd_f, act)
    for fused in (False, True):
        bad, r = bwd_verdict(*args, acc, emu_bwd(*args, fused, gskip_add=acc))
        assert bad == [], (fused, bad)
    good = emu_bwd(*args, False, gskip_add=acc)
    mutants = {"one slab's rows (10 of 20000) missing from dgamma": dict(drop_rows=10),
               "the skip gradient written without gskip_add": dict(forget_add=True)}
    if not bf16:          # fp32 storage holds the channels at mean +-100, where the stored mean is 4e-6 away from the unrounded one
        mutants["xhat from the unrounded mean"] = dict(mean64=st["mean"])
    for name, kw in mutants.items():
        got = emu_bwd(*args, False, gskip_add=acc, **kw)
        bad, r = bwd_verdict(*args, acc, got)
        old = (S.old_close(got[0], good[0], 1e-2 if bf16 else 1e-5) and S.old_close(got[1], good[1], 1e-2 if bf16 else 1e-5)
               and S.old_close(got[2], r["dgamma"], 1e-4 if bf16 else 1e-5) and S.old_close(got[3], r["dbeta"], 1e-4 if bf16 else 1e-5))
        with capsys.disabled():
            print(f"\n  mutant '{name}' ({'bf16' if bf16 else 'fp32'}, act {act}): element-wise criterion rejects {bad or 'NOTHING'}, "
                  f"the old tolerances {'accept' if old else 'reject'}")
        assert bad, name
