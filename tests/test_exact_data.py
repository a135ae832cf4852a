"""Self-test of the integer-data method (tests/exact_data.py) on the CPU: an emulated bf16 kernel - fp32 accumulation chunk by
chunk over the input channels, bias, one bf16 store, the addend added after that first rounding - must be accepted by
assert_exact whatever its chunk order, and each subtle defect a hand-written MFMA kernel can have must be rejected."""
import pytest
import torch

import exact_data as X
from oracle import torch_ref as R


def _emulate(case, x, w, b, add, chunks, drop=None, trunc=False, round_between=False, nobias_last=False, add_first=False):
    B, H, W, Ci, Co, k, s = case
    acc = None
    for c0, c1 in zip(chunks[:-1], chunks[1:]):
        wc = w[:, :, c0:c1].clone()
        if drop is not None and c0 <= drop[2] < c1:
            wc[drop[0], drop[1], drop[2] - c0, :] = 0
        part = R.conv2d_same(x[:, c0:c1].float(), wc.float(), None, s)
        acc = part if acc is None else acc + part
        if round_between:
            acc = acc.to(torch.bfloat16).float()
    bb = b.float().clone()
    if nobias_last:
        bb[-1] = 0
    acc = acc + bb.view(1, -1, 1, 1)
    if add_first:                                   # one rounding: the addend joins the fp32 accumulator
        acc = acc + add.float()
    if trunc:
        y = (acc.view(torch.int32) & ~0xFFFF).view(torch.float32)
    else:
        y = acc.to(torch.bfloat16).float()
    if not add_first:
        y = (y + add.float()).to(torch.bfloat16).float()
    return X.nhwc(y.double())


CASES = [((1, 10, 12, 40, 72, 3, 1), (0, 32, 40), (0, 8, 24, 40)),
         ((2, 9, 7, 72, 40, 3, 2), (0, 64, 72), (0, 8, 40, 72))]       # stride 2, odd size; K = 648: partial sums leave the exact bf16 integers


@pytest.mark.parametrize("case,order_a,order_b", CASES)
def test_integer_data_accepts_the_correct_kernel_and_rejects_every_mutant(case, order_a, order_b):
    B, H, W, Ci, Co, k, s = case
    x, w, b = X.acts(f"x{case}", (B, Ci, H, W)), X.kernels(f"w{case}", (k, k, Ci, Co)), X.biases(f"b{case}", (Co,))
    y = R.conv2d_same(x, w, b, s)
    add = X.addends(f"a{case}", tuple(y.shape))
    # the conditions, from the oracle's side: integers, bf16-representable, every partial sum below 2^24, ties present
    bound = float((R.conv2d_same(x.abs(), w.abs(), b.abs(), s) + add.abs()).max())
    assert bound <= X.conv_abs_bound(k * k * Ci)
    ties = X.check_exactness_conditions({"x": (x, True), "w": (w, True), "bias": (b, False), "addend": (add, True)}, bound, y, add,
                                        what=str(case))
    assert ties > 0
    with pytest.raises(AssertionError):
        X.check_exactness_conditions({"x": (x + 0.5, True)}, bound)
    with pytest.raises(AssertionError):
        X.check_exactness_conditions({"x": (x + 257, True)}, bound)              # odd integers above 256 are not bf16 values
    with pytest.raises(AssertionError):
        X.check_exactness_conditions({"x": (x, True)}, float(1 << 24))
    want = X.nhwc(X.expected_bf16(y, add))
    # the correct kernel in two summation orders
    X.assert_exact(_emulate(case, x, w, b, add, order_a), want, "order a", tile=(16, 32))
    X.assert_exact(_emulate(case, x, w, b, add, order_b), want, "order b", tile=(16, 32))
    # the mutants
    mutants = dict(dropped_term=dict(drop=(2, 1, Ci - 1)), truncating_store=dict(trunc=True), bf16_between_chunks=dict(round_between=True),
                   no_bias_on_last_channel=dict(nobias_last=True), addend_before_first_rounding=dict(add_first=True))
    for name, kw in mutants.items():
        with pytest.raises(AssertionError) as e:
            X.assert_exact(_emulate(case, x, w, b, add, order_a, **kw), want, name, tile=(16, 32))
        assert name in str(e.value) and "elements differ" in str(e.value) and "pixel tiles" in str(e.value), str(e.value)
    # the localisation: a missing bias on the last channel is reported as one channel, the last
    with pytest.raises(AssertionError) as e:
        X.assert_exact(_emulate(case, x, w, b, add, order_a, nobias_last=True), want, "bias", tile=(16, 32))
    assert f"1 distinct channels (lowest {Co - 1}, highest {Co - 1})" in str(e.value)


def test_tie_detection_and_rounding():
    v = torch.tensor([0.0, 1.0, 255.0, 256.0, 257.0, 258.0, 259.0, 511.0, 512.0, 514.0, 516.0, 518.0, -257.0, -1030.0, 1028.0, 0.5, 128.5, 129.0],
                     dtype=torch.float64)
    tie = [False, False, False, False, True, False, True, True, False, True, False, True, True, False, True, False, True, False]
    assert X.is_tie(v).tolist() == tie
    # ties go to the even neighbour
    assert X.bf16(torch.tensor([257.0, 259.0, 514.0, 518.0, -257.0], dtype=torch.float64)).tolist() == [256.0, 260.0, 512.0, 520.0, -256.0]
    # two roundings differ from one: bf16(257) + 2 = 258, but bf16(257 + 2) = 260
    y, a = torch.tensor([257.0, 258.0], dtype=torch.float64), torch.tensor([2.0, 1.0], dtype=torch.float64)
    assert X.expected_bf16(y, a).tolist() == [258.0, 260.0] and X.bf16(y + a).tolist() == [260.0, 260.0]
    assert +0.0 == -0.0
    X.assert_exact(torch.tensor([[0.0, 1.0]]), torch.tensor([[-0.0, 1.0]]), "signed zero")
    with pytest.raises(AssertionError):
        X.assert_exact(torch.tensor([float("nan")]), torch.tensor([float("nan")]), "nan")


def test_ints_covers_its_range_and_repeats():
    t = X.ints("range", (4000,), -1, 3)
    assert sorted(set(t.tolist())) == [-1.0, 0.0, 1.0, 2.0, 3.0]
    assert torch.equal(t, X.ints("range", (4000,), -1, 3))
    a = X.addends("add", (4000,))
    assert float(a.abs().max()) == 240.0 and torch.equal(a % 4, torch.zeros_like(a)) and torch.equal(X.bf16(a), a)


def _emulate_dense(x, w, b, ks, drop_bias_when_one_slice=False, skip_slice=None):
    """The small-batch Dense launcher (csrc/igemm.hip launch_dense_fwd) in fp32: ks == 1 - the kernel's epilogue adds the bias;
    ks > 1 - one fp32 slab per K slice, then bias + the slabs in slab order."""
    K = x.shape[1]
    edges = [round(i * K / ks) for i in range(ks + 1)]
    slabs = [x[:, a:e].float() @ w[:, a:e].float().t() for a, e in zip(edges[:-1], edges[1:])]
    if ks == 1:
        return (slabs[0] if drop_bias_when_one_slice else slabs[0] + b.float()).double()
    y = b.float().expand_as(slabs[0]).clone()
    for i, s_ in enumerate(slabs):
        if i != skip_slice:
            y = y + s_
    return y.double()


def _within_tolerance(got, want, K):
    """The criterion of the uniform data kind for fp32 outputs (test_kernels_gpu.close with 2e-6 sqrt(K) + 1e-6)."""
    return float((got - want).abs().max()) <= (2e-6 * K ** 0.5 + 1e-6) * float(want.abs().max())


@pytest.mark.parametrize("K,N,ks,mutant", [(64, 46080, 1, dict(drop_bias_when_one_slice=True)), (48128, 64, 128, dict(skip_slice=127)),
                                           (48128, 64, 128, dict(skip_slice=0))])
def test_both_data_kinds_reject_a_dense_that_drops_the_bias_or_a_slice(K, N, ks, mutant):
    """The Dense plans of the auto-encoders at main_training.py's size (tests/test_fullsize_ae_vae_gpu.py): one slice, where the bias is
    the igemm epilogue's, and the cap of 128 slices.  The correct emulation passes both data kinds; a launcher that drops the bias
    when ks == 1, or sums 127 of the 128 slabs, passes neither."""
    from oracle import detrand
    Bn = 32
    for data in X.DATA_KINDS:
        if data == "int":
            x, w, b = X.acts(f"dx{K}", (Bn, K)), X.kernels(f"dw{K, N}", (N, K)), X.biases(f"db{N}", (N,))
            X.check_exactness_conditions({"x": (x, False), "w": (w, False), "bias": (b, False)}, X.conv_abs_bound(K, has_addend=False), what="dense")
        else:
            x = torch.tensor(detrand.uniform(f"dx{K}", (Bn, K), -1, 1)).double()
            w = (torch.tensor(detrand.uniform(f"dw{K, N}", (N, K), -1, 1)) * 0.05).double()
            b = torch.tensor(detrand.uniform(f"db{N}", (N,), -1, 1)).double()
        want = x @ w.t() + b
        good, bad = _emulate_dense(x, w, b, ks), _emulate_dense(x, w, b, ks, **mutant)
        if data == "int":
            X.assert_exact(good, want, "dense")
            with pytest.raises(AssertionError) as e:
                X.assert_exact(bad, want, "mutant")
            assert "elements differ" in str(e.value)
        else:
            assert _within_tolerance(good, want, K) and not _within_tolerance(bad, want, K)
