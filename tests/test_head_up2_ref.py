"""The identity csrc/head_up2.hip rests on, checked on the CPU in fp64 on integer data (every sum exact, so equality is demanded):
nearest-neighbour x2 followed by the 6x6 'same' convolution equals fold + 4x4 'same' convolution + depth-to-space, unfold is the
transpose of fold, and the folded kernel has 3 / 4 taps per parity (tests/head_up2_ref.py states the forms)."""
import pytest
import torch

import exact_data as X
import head_up2_ref as HR

SHAPES = [(1, 1, 3, 8), (2, 5, 7, 8), (1, 4, 6, 16), (1, 1, 1, 8), (1, 2, 1, 8)]


def _data(B, h, w, C):
    tag = f"up2ref{B, h, w, C}"
    x = X.acts("x" + tag, (B, C, h, w))
    k = X.kernels("k" + tag, (2, 6, 6, C))
    b = X.biases("b" + tag, (2,))
    d = X.acts("d" + tag, (B, 2, 2 * h, 2 * w)) + 40
    return x, k, b, d


@pytest.mark.parametrize("B,h,w,C", SHAPES)
def test_fold_conv4x4_depth_to_space_equals_the_literal_form(B, h, w, C):
    x, k, b, d = _data(B, h, w, C)
    want, dx, dk, db = HR.literal_grads(x, k, b, d)
    kf = HR.fold(k)
    assert torch.equal(HR.folded(x, kf, b), want)
    gx, gkf = HR.folded_grads(x, kf, d)
    assert torch.equal(gx, dx)
    assert torch.equal(HR.unfold(gkf), dk)
    assert torch.equal(d.sum((0, 2, 3)), db)                       # the bias gradient is the column sum of the fine dlogits
    assert torch.equal(HR.space_to_depth(HR.depth_to_space(HR.space_to_depth(d))), HR.space_to_depth(d))


def test_unfold_is_the_transpose_of_fold():
    k = X.kernels("adjk", (2, 6, 6, 8))
    g = X.acts("adjg", (8, 4, 4, 8))
    assert float((HR.fold(k) * g).sum()) == float((k * HR.unfold(g)).sum())
    # ... on every basis vector too: fold's matrix is 0 / 1 with exactly one 1 per (parity, 6x6 tap)
    e = torch.zeros(2 * 36)
    cols = []
    for i in range(72):
        e.zero_(); e[i] = 1
        cols.append(HR.fold(e.view(2, 6, 6, 1)).reshape(-1))
    m = torch.stack(cols, 1)                                        # [128, 72]
    assert torch.equal(m.sum(0), torch.full((72,), 4.0, dtype=m.dtype))           # one tap per (a, b)
    assert float(m.sum(1).max()) == 4.0                             # a folded tap sums at most 4 weights
    g1 = X.acts("adjg1", (8, 4, 4, 1))
    assert torch.equal(HR.unfold(g1).reshape(-1), m.t() @ g1.reshape(-1))


def test_folded_taps_outside_the_supports_are_zero():
    kf = HR.fold(torch.ones(2, 6, 6, 3, dtype=torch.float64)).view(2, 2, 2, 4, 4, 3)           # [o][a][b][u][v][c]
    assert float(kf[:, 0, :, 3].abs().max()) == 0 and float(kf[:, :, 0, :, 3].abs().max()) == 0
    # 3 taps for parity 0 (2 + 2 + 2 weights), 4 for parity 1 (1 + 2 + 2 + 1): 49 non-zero taps per output channel
    assert kf[0, 0, 0, :, 0, 0].tolist() == [4.0, 4.0, 4.0, 0.0] and kf[0, 1, 0, :, 0, 0].tolist() == [2.0, 4.0, 4.0, 2.0]
    assert kf[0, 1, 1, :, :, 0].tolist() == [[1, 2, 2, 1], [2, 4, 4, 2], [2, 4, 4, 2], [1, 2, 2, 1]]
    assert int((kf[0] != 0).sum()) == 49 * 3 and float(kf.sum()) == 2 * 4 * 36 * 3


def test_the_bf16_work_copy_is_the_fp32_sum_rounded_once():
    from oracle import detrand
    k = torch.tensor(detrand.uniform("up2bf", (2, 6, 6, 16), -1, 1)).float()
    kf = HR.fold_bf16(k)
    assert torch.equal(kf, kf.float().to(torch.bfloat16).double())                 # bf16 values
    s32 = HR.fold(k, torch.float32)
    assert torch.equal(kf, s32.to(torch.bfloat16).double())
    # not the sum of bf16-rounded taps: that differs somewhere on such data
    assert not torch.equal(kf, HR.fold(k.to(torch.bfloat16).double()))
    assert float((kf - HR.fold(k.double())).abs().max()) <= 2.0 ** -8 * float(HR.fold(k.double()).abs().max())
