"""The 2x2 stride-2 kernels (csrc/conv2x2.hip; dl_models/ae_net.py:273-279, :301-307) through their six entry points, against
(a) oracle.torch_ref in fp64 and (b) the generic unetrir_conv2d_* / unetrir_conv2d_transpose_* entry points on the same buffers.

Two data sets, as tests/test_kernels_gpu.py: the integers of tests/exact_data.py, where every stored element must EQUAL the oracle's
(bf16 rounding included, the weight gradient with reg = 0.5 exactly), and uniform(-1, 1) values under close(..., 1e-2), the bound of
the existing bf16 convolution tests.  Every case runs as a Conv2D layer (fine -> coarse) and as a Conv2DTranspose layer (coarse ->
fine) of the same channel pair; each case picks out one way the kernels can go wrong (CASES)."""
import math

import numpy as np
import pytest
import torch

import exact_data as X
from oracle import detrand, torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def close(actual, expected, tol, what=""):
    a, e = actual.detach().double().cpu(), expected.detach().double().cpu()
    assert a.shape == e.shape, (what, a.shape, e.shape)
    scale = float(e.abs().max()) + 1e-30
    err = float((a - e).abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def q16(t):
    return t.to(torch.bfloat16).double()


def rand(name, shape, data, role="act"):
    if data == "int":
        return dict(act=X.acts, kernel=X.kernels, bias=X.biases, addend=X.addends)[role](name, shape)
    return torch.tensor(detrand.uniform(name, tuple(shape), -1, 1, np.float64))


POISON = 768.0


def embed(x_nchw, half):
    """An Act over the NCHW tensor as bf16 NHWC: a buffer of its own, or (half) the upper half of a poisoned buffer twice as wide."""
    import unet_rir_amd
    B, C, H, W = x_nchw.shape
    buf = torch.full((B, H, W, 2 * C if half else C), POISON, dtype=torch.bfloat16)
    buf[..., C if half else 0:] = x_nchw.permute(0, 2, 3, 1).to(torch.bfloat16)
    return unet_rir_amd.ops.Act(buf.to(DEV), C if half else 0, C)


def blank(B, H, W, C, half):
    import unet_rir_amd
    return unet_rir_amd.ops.Act(torch.full((B, H, W, 2 * C if half else C), POISON, dtype=torch.bfloat16, device=DEV), C if half else 0, C)


def lower_half_untouched(a):
    lo = a.base[..., :a.c0].float()
    return lo.numel() == 0 or (float(lo.min()) == POISON and float(lo.max()) == POISON)


def nchw(a):
    return a.dense().double().cpu().permute(0, 3, 1, 2)


#        B  Hf  Wf  Cin  Cout  input in a concat half, output in a concat half     (Hf x Wf: the fine grid)
CASES = [(1, 6, 10, 16, 32, False, False),       # 15 coarse pixels: fewer than one strip of 32, one K block of the weight gradient
         (3, 12, 20, 16, 16, False, False),      # 180 coarse pixels: a tail strip, coarse width 10 (no multiple of 8), pixels of 3 images in one strip
         (2, 8, 16, 32, 64, True, False),        # input ld = 2 C: a concat-half view into a poisoned buffer
         (2, 8, 8, 64, 128, False, False),       # several K groups, several channel tiles
         (2, 8, 8, 256, 512, False, False),      # K = 1024 (gather) / 512 (scatter), 16 channel tiles, 8 x 4 weight-gradient tiles
         (2, 8, 8, 512, 256, False, True)]       # output into the upper half of a ld = 2 C buffer whose lower half must stay untouched


def check(exact, got, want, addend, what):
    """got: an Act; want: the oracle's fp64 NCHW result before the storage rounding."""
    if exact:
        X.assert_exact(got.dense(), X.expected_bf16(want, addend).permute(0, 2, 3, 1), what, tile=(4, 8))
    else:
        close(nchw(got), want if addend is None else want + addend, 1e-2, what)
    assert lower_half_untouched(got), what + ": the other half of the buffer was written"


def twin(exact, got, ref, what):
    """The generic entry point on the same buffers: the same elements on integer data (both exact), within the bf16 bound else."""
    assert lower_half_untouched(ref), what
    if exact:
        assert torch.equal(got.dense(), ref.dense()), what
    else:
        close(got.dense(), ref.dense(), 1e-2, what)


def run_wgrad(ops, fn, twin_fn, ws_bytes, g, xa, gya, w32, want_dw, reg, exact, P, what):
    """One weight gradient: exactly *_ws_bytes in front of a canary, two runs, direct against _partials_ + batched reduce, the oracle
    and the generic twin."""
    need = int(ws_bytes(g))
    assert need > 0
    big = torch.full((need + 256,), 0xAB, dtype=torch.uint8, device=DEV)
    ws = ops.Workspace(DEV)
    ws.buf = big[:need]
    runs = []
    for _ in range(2):
        dw = torch.full(tuple(want_dw.shape), 111.0, device=DEV)
        fn(g, xa, gya, dw, ws, reg=reg, w=w32)
        runs.append(dw)
    rb = ops.ReduceBatch(DEV, need + 4096)
    parked = torch.full(tuple(want_dw.shape), 111.0, device=DEV)
    fn(g, xa, gya, parked, ws, reg=reg, w=w32, defer=rb)
    rb.flush()
    ref = torch.full(tuple(want_dw.shape), 111.0, device=DEV)
    twin_fn(g, xa, gya, ref, ops.Workspace(DEV), reg=reg, w=w32)
    torch.cuda.synchronize()
    assert ws.buf.data_ptr() == big.data_ptr() and int(big[need:].min()) == 0xAB and int(big[need:].max()) == 0xAB, what + ": canary"
    assert torch.equal(runs[0], runs[1]), what + ": two runs differ"
    assert torch.equal(parked, runs[0]), what + ": parked reduction differs"
    if exact:
        X.assert_exact(runs[0], want_dw, what)
        X.assert_exact(ref, want_dw, what + " (generic)")
    else:
        tol = 2e-6 * math.sqrt(P) + 1e-6            # fp32 accumulation order over P exactly stored products (test_conv2d_bf16)
        close(runs[0], want_dw, tol, what)
        close(runs[0], ref, 2 * tol, what + " against the generic kernel")


@X.parametrize_kinds("case", CASES)
def test_conv2d_2x2_stride_2(U, case, data):
    """Conv2D(k=2, strides=2): forward = gather-GEMM (with and without addend), data gradient = scatter-GEMM (written, and
    accumulated behind an addend), weight gradient."""
    ops = U.ops
    exact = data == "int"
    B, Hf, Wf, Ci, Co, in_half, out_half = case
    Hc, Wc = Hf // 2, Wf // 2
    x = q16(rand(f"c22x{case}", (B, Ci, Hf, Wf), data)).requires_grad_(True)
    w = q16(rand(f"c22w{case}", (2, 2, Ci, Co), data, "kernel")).requires_grad_(True)        # HWIO
    b = rand(f"c22b{case}", (Co,), data, "bias")
    y = R.conv2d_same(x, w, b, 2)
    assert tuple(y.shape) == (B, Co, Hc, Wc)
    add = q16(rand(f"c22a{case}", (B, Co, Hc, Wc), data, "addend"))
    gy = q16(rand(f"c22g{case}", (B, Co, Hc, Wc), data))
    dadd = q16(rand(f"c22da{case}", (B, Ci, Hf, Wf), data, "addend"))
    (y * gy).sum().backward()
    reg = X.REG if exact else 0.002
    if exact:
        X.check_exactness_conditions({"x": (x.detach(), True), "w": (w.detach(), True), "bias": (b, False), "addend": (add, True)},
                                     X.conv_abs_bound(4 * Ci), y.detach(), add, what=f"fwd {case}")
        X.check_exactness_conditions({"dy": (gy, True), "addend": (dadd, True)}, X.conv_abs_bound(Co, has_bias=False), x.grad, dadd,
                                     what=f"dgrad {case}")
        X.check_exactness_conditions({"w": (w.detach(), False)}, B * Hc * Wc * 9 + 1, quantum=0.5, what=f"wgrad {case}")
    g = ops.geom(B, Hf, Wf, Ci, Co, 2, 2)
    xa = embed(x.detach(), in_half)
    w32 = w.detach().permute(3, 0, 1, 2).contiguous().float().to(DEV)                        # [Co][2][2][Ci] fp32 master
    wh = torch.empty((Co, 4, Ci), dtype=torch.bfloat16, device=DEV)
    ops.cast_weight_bf16(w32, wh, Co, 4, Ci, Ci)
    wt = torch.zeros((Ci, 4, Co), dtype=torch.bfloat16, device=DEV)
    ops.transpose_cast_weight_bf16(w32, wt, Co, 4, Ci, Co)
    bias = b.float().to(DEV)
    assert ops.conv2x2s2_supported(g, xa, blank(B, Hc, Wc, Co, out_half))
    for ad in (None, add):
        adda = embed(ad, False) if ad is not None else None
        ya, yr = blank(B, Hc, Wc, Co, out_half), blank(B, Hc, Wc, Co, out_half)
        ops.conv2x2s2_fwd(g, xa, wh, bias, ya, adda)
        ops.conv2d_fwd(g, xa, wh, bias, yr, adda)
        torch.cuda.synchronize()
        check(exact, ya, y.detach(), ad, f"conv2x2 fwd {case} addend {ad is not None}")
        twin(exact, ya, yr, f"conv2x2 fwd against conv2d_fwd {case} addend {ad is not None}")
    gya = embed(gy, out_half)
    for ad in (None, dadd):
        adda = embed(ad, False) if ad is not None else None
        dxa, dxr = blank(B, Hf, Wf, Ci, in_half), blank(B, Hf, Wf, Ci, in_half)
        ops.conv2x2s2_dgrad(g, gya, wt, dxa, adda)
        ops.conv2d_dgrad(g, gya, wt, dxr, adda)
        torch.cuda.synchronize()
        check(exact, dxa, x.grad, ad, f"conv2x2 dgrad {case} addend {ad is not None}")
        twin(exact, dxa, dxr, f"conv2x2 dgrad against conv2d_dgrad {case} addend {ad is not None}")
    acc = embed(dadd, in_half)                 # in place behind an earlier writer, as the engines accumulate a skip gradient
    ops.conv2x2s2_dgrad(g, gya, wt, acc, acc)
    torch.cuda.synchronize()
    check(exact, acc, x.grad, dadd, f"conv2x2 dgrad in place {case}")
    for r in (reg, 0.0):
        run_wgrad(ops, ops.conv2x2s2_wgrad, ops.conv2d_wgrad, ops.conv2x2s2_wgrad_ws_bytes, g, xa, gya, w32,
                  (w.grad + r * w.detach()).permute(3, 0, 1, 2), r, exact, B * Hc * Wc, f"conv2x2 wgrad {case} reg {r}")


@X.parametrize_kinds("case", CASES)
def test_conv2d_transpose_2x2_stride_2(U, case, data):
    """Conv2DTranspose(k=2, strides=2): forward = scatter-GEMM, data gradient = gather-GEMM (with and without addend), weight
    gradient in the primary layout [Cin][2][2][Cout]."""
    ops = U.ops
    exact = data == "int"
    B, Hf, Wf, Ci, Co, in_half, out_half = case
    Hc, Wc = Hf // 2, Wf // 2
    x = q16(rand(f"t22x{case}", (B, Ci, Hc, Wc), data)).requires_grad_(True)
    w = q16(rand(f"t22w{case}", (2, 2, Co, Ci), data, "kernel")).requires_grad_(True)        # HWOI
    b = rand(f"t22b{case}", (Co,), data, "bias")
    y = R.conv2d_transpose_same(x, w, b, 2)
    assert tuple(y.shape) == (B, Co, Hf, Wf)
    gy = q16(rand(f"t22g{case}", (B, Co, Hf, Wf), data))
    dadd = q16(rand(f"t22da{case}", (B, Ci, Hc, Wc), data, "addend"))
    (y * gy).sum().backward()
    reg = X.REG if exact else 0.002
    if exact:
        X.check_exactness_conditions({"x": (x.detach(), True), "w": (w.detach(), True), "bias": (b, False)},
                                     X.conv_abs_bound(Ci, has_addend=False), y.detach(), what=f"convT fwd {case}")
        X.check_exactness_conditions({"dy": (gy, True), "addend": (dadd, True)}, X.conv_abs_bound(4 * Co, has_bias=False), x.grad, dadd,
                                     what=f"convT dgrad {case}")
        X.check_exactness_conditions({"w": (w.detach(), False)}, B * Hc * Wc * 9 + 1, quantum=0.5, what=f"convT wgrad {case}")
    g = ops.geom(B, Hc, Wc, Ci, Co, 2, 2)
    xa = embed(x.detach(), in_half)
    w32 = w.detach().permute(3, 0, 1, 2).contiguous().float().to(DEV)                        # primary [Ci][2][2][Co]
    wprim = torch.empty((Ci, 4, Co), dtype=torch.bfloat16, device=DEV)
    ops.cast_weight_bf16(w32, wprim, Ci, 4, Co, Co)
    wt = torch.zeros((Co, 4, Ci), dtype=torch.bfloat16, device=DEV)
    ops.transpose_cast_weight_bf16(w32, wt, Ci, 4, Co, Ci)
    bias = b.float().to(DEV)
    ya, yr = blank(B, Hf, Wf, Co, out_half), blank(B, Hf, Wf, Co, out_half)
    assert ops.conv2x2s2_supported(g, xa, ya, transpose=True)
    ops.conv2x2s2_transpose_fwd(g, xa, wt, bias, ya)
    ops.conv2d_transpose_fwd(g, xa, wt, bias, yr)
    torch.cuda.synchronize()
    check(exact, ya, y.detach(), None, f"conv2x2 transpose fwd {case}")
    twin(exact, ya, yr, f"conv2x2 transpose fwd against conv2d_transpose_fwd {case}")
    gya = embed(gy, out_half)
    for ad in (None, dadd):
        adda = embed(ad, False) if ad is not None else None
        dxa, dxr = blank(B, Hc, Wc, Ci, in_half), blank(B, Hc, Wc, Ci, in_half)
        ops.conv2x2s2_transpose_dgrad(g, gya, wprim, dxa, adda)
        ops.conv2d_transpose_dgrad(g, gya, wprim, dxr, adda)
        torch.cuda.synchronize()
        check(exact, dxa, x.grad, ad, f"conv2x2 transpose dgrad {case} addend {ad is not None}")
        twin(exact, dxa, dxr, f"conv2x2 transpose dgrad against conv2d_transpose_dgrad {case} addend {ad is not None}")
    for r in (reg, 0.0):
        run_wgrad(ops, ops.conv2x2s2_transpose_wgrad, ops.conv2d_transpose_wgrad, ops.conv2x2s2_transpose_wgrad_ws_bytes, g, xa, gya, w32,
                  (w.grad + r * w.detach()).permute(3, 0, 1, 2), r, exact, B * Hc * Wc, f"conv2x2 transpose wgrad {case} reg {r}")


def layer_fwd(ops, g, xa, wh, bias, ya):
    """What a caller does: the 2x2 kernels where `supported` says so, the generic entry point otherwise."""
    if ops.conv2x2s2_supported(g, xa, ya):
        ops.conv2x2s2_fwd(g, xa, wh, bias, ya)
        return "conv2x2"
    ops.conv2d_fwd(g, xa, wh, bias, ya)
    return "generic"


@pytest.mark.parametrize("case", [(2, 7, 10, 16, 32), (2, 8, 9, 16, 32), (2, 8, 10, 8, 32), (2, 8, 10, 16, 8), (1, 4, 4, 48, 32)])
def test_unsupported_shapes_are_refused_and_the_fallback_serves_them(U, case):
    """supported == 0 for an odd H or W, 8 channels on either side, a channel count that is no power of two: the entry points return
    UNETRIR_EINVAL without launching, and the caller's fallback computes the layer ('same' pads an odd size at the bottom / right)."""
    ops = U.ops
    B, H, W, Ci, Co = case
    x = q16(rand(f"u22x{case}", (B, Ci, H, W), "uniform"))
    w = q16(rand(f"u22w{case}", (2, 2, Ci, Co), "uniform", "kernel"))
    b = rand(f"u22b{case}", (Co,), "uniform", "bias")
    y = R.conv2d_same(x, w, b, 2)
    g = ops.geom(B, H, W, Ci, Co, 2, 2)
    xa = embed(x, False)
    w32 = w.permute(3, 0, 1, 2).contiguous().float().to(DEV)
    wh = torch.empty((Co, 4, Ci), dtype=torch.bfloat16, device=DEV)
    ops.cast_weight_bf16(w32, wh, Co, 4, Ci, Ci)
    ya = blank(B, y.shape[2], y.shape[3], Co, False)
    with pytest.raises(U._lib.UnetrirError, match="10001"):
        ops.conv2x2s2_fwd(g, xa, wh, b.float().to(DEV), ya)
    assert layer_fwd(ops, g, xa, wh, b.float().to(DEV), ya) == "generic"
    torch.cuda.synchronize()
    close(nchw(ya), y, 1e-2, f"fallback {case}")


def test_supported_predicate(U):
    """Every 2x2 stride-2 layer of AENet at number_filters_0 in {16, 32, 64} (channels 16 ... 1024, input pixel stride C or 2 C) is
    offered at least its weight gradient, and its forward / data gradient exactly where the measured rule keeps them (K <= 256:
    include/unetrir.h); a pixel stride that is no multiple of 8, or smaller than the channel count, gets nothing."""
    ops = U.ops

    class Ld:
        sfx = "bf16"

        def __init__(self, ld):
            self.ld = ld
    for F0 in (16, 32, 64):
        h, w = 144, 160
        for l in range(1, 5):
            ci, co = F0 << (l - 1), F0 << l
            g = ops.geom(32, h, w, ci, co, 2, 2)
            for ld in (ci, 2 * ci):
                want = ops.C22_WGRAD | (ops.C22_FWD if 4 * ci <= 256 else 0) | (ops.C22_DGRAD if co <= 256 else 0)
                assert ops.conv2x2s2_supported(g, Ld(ld), Ld(co)) == want, (F0, l, ld)
            h, w = h // 2, w // 2
            gt = ops.geom(32, h, w, co, ci, 2, 2)                  # the decoder's way back, written into a concat half
            want = ops.C22_WGRAD | (ops.C22_FWD if co <= 256 else 0) | (ops.C22_DGRAD if 4 * ci <= 256 else 0)
            assert ops.conv2x2s2_supported(gt, Ld(co), Ld(2 * ci), transpose=True) == want, (F0, l)
    g = ops.geom(2, 8, 8, 32, 64, 2, 2)
    assert ops.conv2x2s2_supported(g, Ld(32), Ld(64)) == 7
    for ld_in, ld_out in ((36, 64), (32, 68), (24, 64), (32, 32)):
        assert not ops.conv2x2s2_supported(g, Ld(ld_in), Ld(ld_out)), (ld_in, ld_out)
    assert not ops.conv2x2s2_supported(ops.geom(2, 8, 8, 1024, 1024, 2, 2), Ld(1024), Ld(1024))      # 4 x 1024 values per kernel row: no tile fits LDS
    assert not ops.conv2x2s2_supported(ops.geom(2, 8, 8, 32, 64, 3, 2), Ld(32), Ld(64))
    assert not ops.conv2x2s2_supported(ops.geom(2, 8, 8, 32, 64, 2, 1), Ld(32), Ld(64))
