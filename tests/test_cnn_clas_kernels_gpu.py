"""The kernels of csrc/cnn_clas.hip through the C ABI (unet_rir_amd.ops), element by element.

  'valid' convolution   integer data (tests/exact_data.py): forward, data gradient, weight gradient and bias gradient EQUAL the fp64
                        restatement (tests/cnn_clas_ref.py + autograd) and EQUAL the twin - the existing 'same' fp32 entry points on
                        the same input, whose interior is the 'valid' result (forward) and whose gradients of a zero-ringed dy are
                        the 'valid' gradients.  Uniform data: every element within a bound from the accumulation length.
  pooling               integer data: EQUAL the one value the kernel's expression can produce; the dropped row / column is zero.
  BatchNorm forms       the affine folded into the pooling kernels and the backward composition the engine runs, within the bounds
                        tests/streaming_check.py derives for bn_apply / bn_bwd.
  softmax               probabilities, dlogits, loss and the exact count of correct rows.
Every tensor has a pixel stride larger than its channel count, with NaN in the columns no kernel may read or write."""
import numpy as np
import pytest
import torch

import cnn_clas_ref as A
import exact_data as E
import streaming_check as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D64 = torch.float64


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def embed(ops, t_nhwc, extra=4):
    """fp64 / fp32 [B,H,W,C] (CPU) -> an Act on the device with pixel stride C + extra, NaN in the columns behind C."""
    B, H, W, C_ = t_nhwc.shape
    base = torch.full((B, H, W, C_ + extra), float("nan"), dtype=torch.float32, device=DEV)
    base[..., :C_] = t_nhwc.to(DEV, torch.float32)
    return ops.Act(base, 0, C_)


def blank(ops, B, H, W, C_, extra=4):
    return ops.Act(torch.full((B, H, W, C_ + extra), float("nan"), dtype=torch.float32, device=DEV), 0, C_)


def body(a):
    """The channels of an Act as fp64 [B,H,W,C] on the CPU, after asserting that the columns behind them are still NaN."""
    torch.cuda.synchronize()
    assert bool(torch.isnan(a.base[..., a.C:]).all()), "a kernel wrote behind the channels of its output"
    return a.base[..., :a.C].double().cpu()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


class Guarded:
    """A Workspace of exactly `adv` bytes in front of a canary (tests/test_streaming_gpu.py)."""
    CANARY = 0xA5

    def __init__(self, ops, adv, tail=1 << 20):
        self.big = torch.full((int(adv + tail),), self.CANARY, dtype=torch.uint8, device=DEV)
        self.ws = ops.Workspace(DEV)
        self.ws.buf = self.big[:int(adv)]
        self.adv = int(adv)

    def assert_intact(self, what):
        torch.cuda.synchronize()
        assert self.ws.buf.data_ptr() == self.big.data_ptr() and self.ws.nbytes == self.adv, f"{what}: the wrapper asked for more than advertised"
        assert int((self.big[self.adv:] != self.CANARY).sum()) == 0, f"{what}: bytes behind the advertised workspace were overwritten"


# ----------------------------------------------------------------------------------------------------------------------
# 'valid' convolution
# ----------------------------------------------------------------------------------------------------------------------
# (B, H, W, Cin stored, Cout): the sim test's three layers, a single output pixel, and two of the model's own layers at 144 x 160
CONV_CASES = [(3, 21, 24, 4, 16), (3, 9, 11, 16, 32), (3, 3, 4, 32, 64), (2, 3, 3, 16, 32), (2, 144, 160, 4, 16), (2, 34, 38, 32, 64)]


def conv_data(case, data):
    B, H, W, ci, co = case
    tag = f"cnn_clas/{B}-{H}-{W}-{ci}-{co}"
    if data == "int":
        x, k, b, dy = E.acts(tag + "/x", (B, ci, H, W)), E.kernels(tag + "/w", (3, 3, ci, co)), E.biases(tag + "/b", (co,)), E.acts(tag + "/dy", (B, co, H - 2, W - 2))
    else:
        g = torch.Generator().manual_seed(B * H * W + ci + co)
        u = lambda shape, lo, hi: (torch.rand(shape, generator=g) * (hi - lo) + lo).float().double()
        x, k, b, dy = u((B, ci, H, W), -1, 1), u((3, 3, ci, co), -0.5, 0.5), u((co,), -0.5, 0.5), u((B, co, H - 2, W - 2), -1, 1)
    if ci == 4:
        x[:, 2:] = 0          # the first layer: two input channels, zero-padded as unetrir_nchw_to_nhwc_pad_f32 writes them
    return x, k, b, dy


def conv_reference(x, k, b, dy, relu, mask=None):
    """(pre-activation, dx, dw [Cout][3][3][Cin], dbias) in fp64; mask: the activation decisions to use (default: pre > 0)."""
    x, k, b = x.clone().requires_grad_(True), k.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = A.conv_valid(x, k, b)
    gm = dy * ((pre.detach() > 0) if mask is None else mask) if relu else dy
    pre.backward(gm)
    return pre.detach(), x.grad, k.grad.permute(3, 0, 1, 2).contiguous(), b.grad


def run_conv(U, case, x, k, b, dy, relu, ws=None):
    ops = U.ops
    B, H, W, ci, co = case
    g = ops.geom(B, H, W, ci, co, 3, 1)
    w = k.permute(3, 0, 1, 2).contiguous().to(DEV, torch.float32)             # [Cout][3][3][Cin]
    wt = torch.empty(ci * 9 * co, device=DEV)
    ops.transpose_weight(w, wt, co, 9, ci)
    bias = b.to(DEV, torch.float32)
    xa, dya = embed(ops, nhwc(x)), embed(ops, nhwc(dy), extra=8)
    ya, dxa = blank(ops, B, H - 2, W - 2, co, extra=8), blank(ops, B, H, W, ci)
    dw, db = torch.full((co, 3, 3, ci), float("nan"), device=DEV), torch.full((co,), float("nan"), device=DEV)
    ops.conv3x3_valid_fwd(g, xa, w, bias, ya, relu)
    ops.conv3x3_valid_dgrad(g, dya, ya, wt, dxa, relu)
    ops.conv3x3_valid_wgrad(g, xa, dya, ya, dw, db, ws if ws is not None else ops.Workspace(DEV), relu)
    return body(ya), body(dxa), dw.double().cpu(), db.double().cpu(), (g, w, wt, bias, xa)


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("case", CONV_CASES, ids=["-".join(map(str, c)) for c in CONV_CASES])
def test_valid_convolution_exact_on_integer_data(U, case, relu):
    ops = U.ops
    B, H, W, ci, co = case
    x, k, b, dy = conv_data(case, "int")
    P = B * (H - 2) * (W - 2)
    E.check_exactness_conditions({"x": (x, False), "w": (k, False), "bias": (b, False), "dy": (dy, False)},
                                 max(E.conv_abs_bound(9 * max(ci, co), True, False), P * 9 + 0.0), what=str(case))
    pre, dx, dw, dbias = conv_reference(x, k, b, dy, relu)
    want_y = torch.relu(pre) if relu else pre
    adv = ops.conv3x3_valid_wgrad_ws_bytes(ops.geom(B, H, W, ci, co, 3, 1))
    gd = Guarded(ops, adv)
    y, gx, gw, gb, (g, w, wt, bias, xa) = run_conv(U, case, x, k, b, dy, relu, gd.ws)
    gd.assert_intact(f"conv3x3_valid_wgrad {case}")
    E.assert_exact(y, nhwc(want_y), f"forward {case}")
    E.assert_exact(gx, nhwc(dx), f"data gradient {case}")
    E.assert_exact(gw, dw, f"weight gradient {case}")
    E.assert_exact(gb, dbias, f"bias gradient {case}")
    if ci == 4:
        assert float(gw[..., 2:].abs().max()) == 0.0          # the padded input channels get a zero gradient
    # the twin: the 'same' entry points on the same input
    gs = ops.geom(B, H, W, ci, co, 3, 1)
    ys = ops.new_act(B, H, W, co, DEV)
    ops.conv2d_fwd(gs, xa, w, bias, ys)
    twin = ys.base[:, 1:-1, 1:-1].double().cpu()
    E.assert_exact(y, torch.relu(twin) if relu else twin, f"forward against the 'same' twin {case}")
    gm = dy * (pre > 0) if relu else dy
    dyp = torch.zeros((B, H, W, co), dtype=D64)
    dyp[:, 1:-1, 1:-1] = nhwc(gm)
    dys, dxs = ops.Act(dyp.to(DEV, torch.float32)), ops.new_act(B, H, W, ci, DEV)
    ops.conv2d_dgrad(gs, dys, wt, dxs)
    dws, dbs = torch.zeros((co, 3, 3, ci), device=DEV), torch.zeros(co, device=DEV)
    ws = ops.Workspace(DEV)
    ops.conv2d_wgrad(gs, xa, dys, dws, ws)
    ops.colsum(dys, dbs, ws)
    torch.cuda.synchronize()
    E.assert_exact(gx, dxs.base.double().cpu(), f"data gradient against the 'same' twin {case}")
    E.assert_exact(gw, dws.double().cpu(), f"weight gradient against the 'same' twin {case}")
    E.assert_exact(gb, dbs.double().cpu(), f"bias gradient against the 'same' twin {case}")


@pytest.mark.parametrize("relu", [1, 0], ids=["relu", "linear"])
@pytest.mark.parametrize("case", CONV_CASES, ids=["-".join(map(str, c)) for c in CONV_CASES])
def test_valid_convolution_within_its_accumulation_bound_on_uniform_data(U, case, relu):
    """Bounds from the accumulation length, as tests/streaming_check.py derives its own: an fmaf chain of n terms rounds n times,
    each time at most 2^-24 of a partial sum that the sum S of the absolute values of the terms bounds.
      forward          n = 9 Cin products + the bias:  d = (9 Cin + 1) 2^-24 S
      data gradient    n = 9 Cout:                     d = 9 Cout 2^-24 S      (dy * [y > 0] is a selection: exact)
      weight gradient  n = P pixels, chained within a slab and then across the slabs - any order of P additions:  d = P 2^-24 S
      bias gradient    the same P additions of exact values
    The activation decisions of the backward kernels are taken from the STORED forward output (chained passes)."""
    B, H, W, ci, co = case
    x, k, b, dy = conv_data(case, "uniform")
    y, gx, gw, gb, _ = run_conv(U, case, x, k, b, dy, relu)
    pre, _, _, _ = conv_reference(x, k, b, dy, relu)
    S_pre, _, _, _ = conv_reference(x.abs(), k.abs(), b.abs(), dy.abs(), 0)
    S.check(y.float(), nhwc(pre), (9 * ci + 1) * S.U32 * nhwc(S_pre), f"forward {case}", kernel="conv3x3_valid_fwd", act=relu)
    mask = nchw(y) > 0
    _, dx, dw, dbias = conv_reference(x, k, b, dy, relu, mask)
    _, S_dx, S_dw, S_db = conv_reference(x.abs(), k.abs(), b.abs(), dy.abs(), relu, mask)
    P = B * (H - 2) * (W - 2)
    S.check(gx.float(), nhwc(dx), 9 * co * S.U32 * nhwc(S_dx), f"data gradient {case}", kernel="conv3x3_valid_dgrad")
    S.check(gw.float(), dw, P * S.U32 * S_dw, f"weight gradient {case}", kernel="conv3x3_valid_wgrad")
    S.check(gb.float(), dbias, P * S.U32 * S_db, f"bias gradient {case}", kernel="conv3x3_valid_wgrad (bias)")
    if relu:
        assert 0.2 < float(mask.double().mean()) < 0.8          # both sides of the ReLU are exercised


def test_valid_convolution_is_bit_identical_across_runs(U):
    case = (2, 34, 38, 32, 64)
    x, k, b, dy = conv_data(case, "uniform")
    a, c = run_conv(U, case, x, k, b, dy, 1)[:4], run_conv(U, case, x, k, b, dy, 1)[:4]
    for p, q in zip(a, c):
        assert torch.equal(p, q)


# ----------------------------------------------------------------------------------------------------------------------
# pooling
# ----------------------------------------------------------------------------------------------------------------------
POOL_SIZES = [(19, 22), (7, 9), (2, 2), (3, 3), (142, 158)]
F32 = lambda v: float(torch.tensor(v, dtype=torch.float32))


def pool_data(h, w, C_, B=2):
    tag = f"cnn_clas/pool{h}-{w}-{C_}"
    x = E.acts(tag + "/x", (B, C_, h, w))
    scale = torch.tensor([0.5, 2.0, -4.0, 1.0], dtype=D64).repeat(C_ // 4)          # powers of two: the products are exact
    shift = E.ints(tag + "/s", (C_,), -20, 20)
    return x, scale, shift


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("h,w", POOL_SIZES)
def test_average_pooling_exact_on_integer_data(U, h, w, affine):
    ops = U.ops
    B, C_ = 2, 16
    x, scale, shift = pool_data(h, w, C_)
    aff = torch.cat([scale, shift]).to(DEV, torch.float32) if affine else None
    xa, ya = embed(ops, nhwc(x)), blank(ops, B, h // 2, w // 2, C_, extra=8)
    ops.avgpool2_fwd(xa, aff, ya)
    want = A.avg_pool2(x)                                   # quarters of integer sums: exact
    if affine:
        want = want * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    E.assert_exact(body(ya), nhwc(want), f"avgpool2_fwd {h}x{w}")
    dy = E.acts(f"cnn_clas/pool{h}-{w}/dy", (B, C_, h // 2, w // 2))
    dxa = blank(ops, B, h, w, C_)
    ops.avgpool2_bwd(embed(ops, nhwc(dy), extra=8), dxa)
    x0 = torch.zeros((B, C_, h, w), dtype=D64, requires_grad=True)
    (gx,) = torch.autograd.grad(A.avg_pool2(x0), x0, dy)
    got = body(dxa)
    E.assert_exact(got, nhwc(gx), f"avgpool2_bwd {h}x{w}")
    if h % 2:
        assert float(got[:, -1].abs().max()) == 0.0          # the dropped trailing row ...
    if w % 2:
        assert float(got[:, :, -1].abs().max()) == 0.0       # ... and column
    assert float(got[:, :2 * (h // 2), :2 * (w // 2)].abs().max()) > 0


def test_pooling_to_an_empty_output_is_refused(U):
    ops = U.ops
    x, y = ops.new_act(2, 1, 2, 16, DEV), ops.new_act(2, 1, 1, 16, DEV)
    with pytest.raises(U.UnetrirError):
        ops.avgpool2_fwd(x, None, y)
    with pytest.raises(U.UnetrirError):
        ops.avgpool2_bwd(y, x)


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("h,w", POOL_SIZES + [(1, 2), (32, 36)])
def test_global_pooling_exact_on_integer_data(U, h, w, affine):
    """The sum of h w integers is exact; the kernel multiplies it by the fp32 constant 1 / (h w) (one rounding of an exact product)
    and, with the affine, takes fmaf(., scale, shift) with a power-of-two scale and an integer shift (one rounding of an exact
    expression): each output can take ONE value, computed here in fp64 and rounded once."""
    ops = U.ops
    B, C_ = 2, 64
    x, scale, shift = pool_data(h, w, C_)
    inv = F32(1.0) / F32(float(h * w))
    inv = F32(inv)
    aff = torch.cat([scale, shift]).to(DEV, torch.float32) if affine else None
    ya = blank(ops, B, 1, 1, C_)
    ops.gap_fwd(embed(ops, nhwc(x)), aff, ya)
    want = (x.sum((2, 3)) * inv).float().double()
    if affine:
        want = (want * scale + shift).float().double()
    E.assert_exact(body(ya).view(B, C_), want, f"gap_fwd {h}x{w}")
    dy = E.acts(f"cnn_clas/gap{h}-{w}/dy", (B, C_))
    dxa = blank(ops, B, h, w, C_, extra=8)
    ops.gap_bwd(embed(ops, dy.view(B, 1, 1, C_)), dxa)
    E.assert_exact(body(dxa), (dy * inv).float().double().view(B, 1, 1, C_).expand(B, h, w, C_), f"gap_bwd {h}x{w}")


# ----------------------------------------------------------------------------------------------------------------------
# the BatchNorm forms: statistics -> pooling with the folded affine; pooling adjoint -> bn_bwd
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("glob", [False, True], ids=["avgpool2", "gap"])
@pytest.mark.parametrize("h,w,C_", [(19, 22, 16), (7, 9, 32), (142, 158, 16)])
def test_batchnorm_folded_into_the_pooling_kernels(U, h, w, C_, glob):
    """Forward: m = 0.25 ((a + b) + (c + d)) rounds three times on at most M = 0.25 sum |x| (the quarter is exact), the fmaf once more:
    d = 2^-24 (3 M |scale| + M |scale| + |shift|); the global mean: h w additions, the product with 1 / (h w) (the constant itself is
    rounded: 2 more), the fmaf: d = 2^-24 ((h w + 2) M |scale| + M |scale| + |shift|).  The affine is READ BACK from bn_stats.
    Backward: the pooling adjoint is one exact product (a quarter) or one rounded one (1 / (h w)), then unetrir_bn_bwd_f32 within
    the bounds of streaming_check.bwd_ref / dx_ref with da as stored."""
    ops = U.ops
    B = 2
    g = torch.Generator().manual_seed(h * w + C_)
    x = torch.relu(torch.rand((B, C_, h, w), generator=g) * 3 - 1).float().double()          # a ReLU output: statistics over it
    gamma, beta = (torch.rand(C_, generator=g) + 0.5).float(), (torch.rand(C_, generator=g) - 0.5).float()
    xa = embed(ops, nhwc(x))
    aff, saved = torch.zeros(2 * C_, device=DEV), torch.zeros(2 * C_, device=DEV)
    ws = ops.Workspace(DEV)
    ops.bn_stats(xa, gamma.to(DEV), beta.to(DEV), aff, saved, ws)
    ph, pw = (1, 1) if glob else (h // 2, w // 2)
    ya = blank(ops, B, ph, pw, C_, extra=8)
    (ops.gap_fwd if glob else ops.avgpool2_fwd)(xa, aff, ya)
    torch.cuda.synchronize()
    sc, sh = aff[:C_].double().cpu().view(1, -1, 1, 1), aff[C_:].double().cpu().view(1, -1, 1, 1)
    if glob:
        m, M, k = x.mean((2, 3), keepdim=True), x.abs().mean((2, 3), keepdim=True), h * w + 2
    else:
        m, M, k = A.avg_pool2(x), A.avg_pool2(x.abs()), 3
    S.check(body(ya).float(), nhwc(m * sc + sh), nhwc(S.U32 * (k * M * sc.abs() + M * sc.abs() + sh.abs())), f"pool(bn) {h}x{w}",
            kernel="gap_fwd" if glob else "avgpool2_fwd")
    # backward as the engine composes it
    dp = (torch.rand((B, C_, ph, pw), generator=g) * 2 - 1).float().double()
    dpa, da = embed(ops, nhwc(dp), extra=8), ops.new_act(B, h, w, C_, DEV)
    outs = []
    for _ in range(2):
        dxa, dg, db = blank(ops, B, h, w, C_), torch.zeros(C_, device=DEV), torch.zeros(C_, device=DEV)
        (ops.gap_bwd if glob else ops.avgpool2_bwd)(dpa, da)
        ops.bn_bwd(da, xa, None, aff, saved, dxa, dg, db, ws, relu=0)
        outs.append((body(dxa), dg.cpu().clone(), db.cpu().clone()))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][2], outs[1][2]) and torch.equal(outs[0][0], outs[1][0])
    x0 = torch.zeros((B, C_, h, w), dtype=D64, requires_grad=True)
    pooled = x0.sum((2, 3), keepdim=True) * F32(F32(1.0) / F32(float(h * w))) if glob else A.avg_pool2(x0)
    (da_ref,) = torch.autograd.grad(pooled, x0, dp)
    da_got = da.base.double().cpu()
    S.check(da_got.float(), nhwc(da_ref), S.U32 * nhwc(da_ref).abs() if glob else 0.0, f"pool adjoint {h}x{w}")
    Pn = B * h * w
    flat = lambda t: t.reshape(Pn, C_)
    mean_f, rstd_f = saved[:C_].cpu(), saved[C_:].cpu()
    r = S.bwd_ref(flat(nhwc(x)), flat(da_got), torch.ones((Pn, C_), dtype=torch.bool), None, mean_f, rstd_f, 0)
    dx, dgm, dbt = outs[0]
    S.check(dbt, r["dbeta"], r["d_dbeta"], f"dbeta {h}x{w}", kernel="bn_bwd behind pooling")
    S.check(dgm, r["dgamma"], r["d_dgamma"], f"dgamma {h}x{w}", kernel="bn_bwd behind pooling")
    ref, d = S.dx_ref(r, aff[:C_].cpu(), dbt, dgm, Pn)
    S.check(flat(dx).float(), ref, d, f"dx {h}x{w}", kernel="bn_bwd behind pooling")
    if not glob and (h % 2 or w % 2):          # da is zero in the dropped row / column, dx is not: the statistics reach every pixel
        assert float(da_got[:, 2 * (h // 2):].abs().sum() + da_got[:, :, 2 * (w // 2):].abs().sum()) == 0.0
        assert float(dx[:, 2 * (h // 2):].abs().sum() + dx[:, :, 2 * (w // 2):].abs().sum()) > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# softmax + categorical cross-entropy + accuracy
# ----------------------------------------------------------------------------------------------------------------------
SOFTMAX_CASES = [(K, B) for K in (2, 5, 64, 1024) for B in (1, 3, 32)]


def softmax_inputs(K, B):
    """Logits in [-4, 4) with +-80 planted (exp overflows without the max subtraction, and exp(-160) underflows), exact ties in the
    logits and in the targets at the row maximum, one-hot rows and soft rows that do not sum to 1."""
    g = torch.Generator().manual_seed(K * 100 + B)
    z = (torch.rand((B, K), generator=g) * 8 - 4).float()
    y = torch.zeros((B, K))
    lab = torch.randint(0, K, (B,), generator=g)
    y[torch.arange(B), lab] = 1.0
    for b in range(B):
        kind = b % 4
        if kind == 1:            # a soft row that does not sum to 1, with a tie at its maximum
            y[b] = torch.rand(K, generator=g).float() * 0.5
            y[b, [K - 1, 0]] = 0.75
        elif kind == 2:          # +-80 and a tie at the maximum of the logits
            z[b, 0], z[b, K - 1] = -80.0, 80.0
            if K > 2:
                z[b, 1] = 80.0
        elif kind == 3:          # a tie in the logits at the label
            z[b, lab[b]] = z[b].max() + 1
            z[b, (lab[b] + 1) % K] = z[b, lab[b]]
    return z, y


def softmax_formula(z, y, inv_norm, dt):
    """The kernel's formula evaluated in `dt` on the CPU."""
    z, y = z.to(dt), y.to(dt)
    m = z.max(1, keepdim=True).values
    e = torch.exp(z - m)
    s = e.sum(1, keepdim=True)
    p = e / s
    ce = -(y * ((z - m) - torch.log(s))).sum(1)
    d = (p * y.sum(1, keepdim=True) - y) * torch.tensor(inv_norm, dtype=dt)
    return p, d, ce


_FIGS = {}


def softmax_bounds():
    """Four times the largest error of the fp32 evaluation against fp64 over ALL of this module's softmax inputs: the device's exp /
    log may differ from libm by a few ulp and the loss and gradient pass through a handful of roundings more.  Measured on the CPU
    (printed by the test; the figures depend on the host's libm - two hosts gave): probabilities 7.2e-8 -> bound 2.9e-7 absolute;
    dlogits (inv_norm 1 / B) 9.0e-8 / 1.9e-7 -> 3.6e-7 / 7.8e-7 absolute; row cross-entropy 2.4e-4 -> 9.5e-4 absolute, on values up to
    2.4e3 (soft rows of 1024 classes)."""
    if not _FIGS:
        ep = ed = ec = 0.0
        for K, B in SOFTMAX_CASES:
            z, y = softmax_inputs(K, B)
            p32, d32, c32 = softmax_formula(z, y, 1.0 / B, torch.float32)
            p64, d64, c64 = softmax_formula(z, y, 1.0 / B, D64)
            ep = max(ep, float((p32.double() - p64).abs().max()))
            ed = max(ed, float((d32.double() - d64).abs().max()))
            ec = max(ec, float((c32.double() - c64).abs().max()))
        _FIGS.update(p=ep, d=ed, ce=ec)
        print(f"softmax fp32-vs-fp64 on the CPU: probabilities {ep:.3e}, dlogits {ed:.3e}, row cross-entropy {ec:.3e}")
    return 4 * _FIGS["p"], 4 * _FIGS["d"], 4 * _FIGS["ce"]


@pytest.mark.parametrize("K,B", SOFTMAX_CASES)
def test_softmax_cross_entropy_and_accuracy(U, K, B):
    ops = U.ops
    bp, bd, bc = softmax_bounds()
    z, y = softmax_inputs(K, B)
    ld = -(-K // 4) * 4 + 4
    la = embed(ops, z.view(B, 1, 1, K), extra=ld - K)
    dl = blank(ops, B, 1, 1, K, extra=ld - K)
    probs = torch.full((B, K), float("nan"), device=DEV)
    loss, acc = torch.full((4,), float("nan"), device=DEV), torch.full((1,), float("nan"), device=DEV)
    inv = 1.0 / B
    ops.softmax_ce(la, K, y.to(DEV), inv, probs, dl, loss, acc)
    torch.cuda.synchronize()
    p64, d64, c64 = softmax_formula(z, y, inv, D64)
    got_p, got_d = probs.double().cpu(), dl.base.view(B, ld).double().cpu()
    assert bool(torch.isfinite(got_p).all()) and bool(torch.isfinite(got_d).all())
    assert float((got_p - p64).abs().max()) <= bp, (float((got_p - p64).abs().max()), bp)
    assert float((got_d[:, :K] - d64).abs().max()) <= bd, (float((got_d[:, :K] - d64).abs().max()), bd)
    assert float(got_d[:, K:].abs().max()) == 0.0               # the columns behind `classes` are written with zeros
    assert float((got_p.sum(1) - 1).abs().max()) <= 2.0 ** -22 * K
    raw = float(c64.sum())
    assert abs(float(loss[1]) - raw) <= B * bc + S.U32 * abs(raw), (float(loss[1]), raw)
    assert abs(float(loss[0]) - raw * inv) <= (B * bc + 2 * S.U32 * abs(raw)) * inv and float(loss[2]) == 0.0
    assert float(acc[0]) == A.n_correct(z.double(), y.double())              # lowest index on ties on both sides: exact
    # the inference form and the bridge from an upstream gradient on the probabilities
    p2 = torch.full((B, K), float("nan"), device=DEV)
    ops.softmax_fwd(la, K, p2)
    assert torch.equal(p2, probs)
    dp = (torch.rand((B, K), generator=torch.Generator().manual_seed(K + B)) * 2 - 1).float()
    d2 = blank(ops, B, 1, 1, K, extra=ld - K)
    ops.softmax_bwd(probs, dp.to(DEV), K, d2)
    torch.cuda.synchronize()
    # dz = p (dp - s), s = sum dp p, from the STORED probabilities: the products and the K-term sum of s round at most K + 1 times on
    # sum |dp p|, the difference and the last product once each
    pg, dpd = got_p, dp.double()
    s_, s_abs = (dpd * pg).sum(1, keepdim=True), (dpd.abs() * pg).sum(1, keepdim=True)
    want = pg * (dpd - s_)
    bound = S.U32 * pg * ((K + 1) * s_abs + 2 * (dpd.abs() + s_.abs())) + S.TINY
    got = d2.base.view(B, ld).double().cpu()
    assert bool(((got[:, :K] - want).abs() <= bound).all()) and float(got[:, K:].abs().max()) == 0.0


def test_softmax_is_bit_identical_across_runs(U):
    ops = U.ops
    z, y = softmax_inputs(1024, 32)
    la = ops.Act(z.view(32, 1, 1, 1024).to(DEV))
    outs = []
    for _ in range(2):
        dl, probs = ops.new_act(32, 1, 1, 1024, DEV), torch.zeros((32, 1024), device=DEV)
        loss, acc = torch.zeros(4, device=DEV), torch.zeros(1, device=DEV)
        ops.softmax_ce(la, 1024, y.to(DEV), 1 / 32, probs, dl, loss, acc)
        torch.cuda.synchronize()
        outs.append((probs.cpu(), dl.base.cpu(), loss.cpu(), acc.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
