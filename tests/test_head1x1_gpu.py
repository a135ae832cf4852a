"""csrc/head1x1.hip - the Conv2D(2, (1, 1)) head of DiffUNet on a bf16 trunk (dl_models/diff_u_net.py:247) - on the GPU.

Integer data (tests/exact_data.py; at most 46 080 pixels, so every sum stays below 2^24): every stored element of y, dx, dw[0:2] and
dbias[0:2] EQUALS the fp64 oracle (bf16 outputs: its bf16 rounding), y[..., 2:4] is zero, the canaries beyond are intact, and the generic
path - tap-table forward, data gradient, weight gradient, colsum - gives the same bits.  Uniform data: every element against the fp64
reference over the bf16-rounded inputs, bound n * 2^-24 * sum |terms| for an fp32 sum of n terms in any order (dx, a sum of two exact
products rounded once and stored as bf16, is determined: equality).  Two runs and a captured graph's replay give the same bits."""
import ctypes as C

import pytest
import torch

import exact_data as X
import streaming_check as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D64 = torch.float64
# (B, H, W, C, ldx): one pixel; 561 pixels with a partial last block, the input a view of a wider buffer; C no multiple of 16; many
# workgroups and slabs; the widest C
SHAPES = [(1, 1, 1, 8, 8), (1, 33, 17, 32, 64), (1, 33, 17, 40, 40), (2, 144, 160, 64, 64), (1, 16, 16, 256, 256)]
LDY, LDDY, PAD = 8, 8, 8
CANARY = -12345.0


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def _data(kind, B, H, W, Cc):
    tag = f"head1x1/{kind}/{B}x{H}x{W}x{Cc}"
    if kind == "int":
        x, dy = X.acts(tag + "/x", (B, H, W, Cc)), X.acts(tag + "/dy", (B, H, W, 2))
        w, b = X.kernels(tag + "/w", (2, Cc)), X.biases(tag + "/b", (2,))
        n_ties = X.check_exactness_conditions({"x": (x, True), "dy": (dy, True), "w": (w, True), "bias": (b, False)},
                                              max(X.conv_abs_bound(Cc, True, False), B * H * W * 9), what=tag)
        X.note_ties(n_ties)
    else:
        g = torch.Generator().manual_seed(B * H * W + Cc)
        u = lambda shape: torch.rand(shape, generator=g, dtype=D64) * 2 - 1
        x, dy = X.bf16(u((B, H, W, Cc))), X.bf16(u((B, H, W, 2)))
        w, b = u((2, Cc)).float().double(), u((2,)).float().double()
    return x, dy, w, b


class _Bufs:
    """Device buffers of one case, every one with canaries where the kernels must not write."""

    def __init__(self, U, shape, x, dy, w, b):
        ops = U.ops
        B, H, W, Cc, ldx = shape
        self.shape = shape
        xb = torch.full((B, H, W, ldx), 5.0, dtype=torch.bfloat16, device=DEV)
        xb[..., :Cc] = x.to(DEV).to(torch.bfloat16)
        self.x = ops.Act(xb, 0, Cc)
        dyb = torch.zeros((B, H, W, LDDY), dtype=torch.bfloat16, device=DEV)
        dyb[..., :2] = dy.to(DEV).to(torch.bfloat16)
        dyb[..., 2:] = 3.0                                       # channels 2.. are not read
        self.dy = ops.Act(dyb, 0, LDDY)
        self.w = torch.zeros((PAD, Cc), dtype=torch.float32, device=DEV)
        self.w[:2] = w.float().to(DEV)
        self.bias = torch.zeros(PAD, dtype=torch.float32, device=DEV)
        self.bias[:2] = b.float().to(DEV)
        self.fresh()
        self.need = ops.head1x1_bwd_ws_bytes(B, H, W, Cc)
        self.ws = torch.full((self.need + 256,), 0xA5, dtype=torch.uint8, device=DEV)

    def fresh(self):
        ops_act = self.x.__class__
        B, H, W, Cc, ldx = self.shape
        self.y = ops_act(torch.full((B, H, W, LDY), CANARY, dtype=torch.float32, device=DEV), 0, LDY)
        self.dx = ops_act(torch.full((B, H, W, ldx), 7.0, dtype=torch.bfloat16, device=DEV), 0, Cc)
        self.dw = torch.full((PAD, Cc), CANARY, dtype=torch.float32, device=DEV)
        self.db = torch.full((PAD,), CANARY, dtype=torch.float32, device=DEV)

    def fwd(self, U):
        U.ops.head1x1_fwd(self.x, self.w, self.bias, self.y)

    def bwd(self, U):
        """The C entry point itself, with exactly the workspace the query asks for."""
        B, H, W, Cc, ldx = self.shape
        p = lambda t: C.c_void_p(t.ptr if hasattr(t, "ptr") else t.data_ptr())
        err = U._lib.lib().unetrir_head1x1_bwd_bf16(p(self.x), self.x.ld, p(self.dy), self.dy.ld, B, H, W, Cc, p(self.w), p(self.dx), self.dx.ld,
                                                   p(self.dw), p(self.db), p(self.ws), self.need,
                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert err == 0, err

    def canaries_intact(self):
        B, H, W, Cc, ldx = self.shape
        assert bool((self.y.base[..., 4:] == CANARY).all()), "y beyond channel 3"
        assert bool((self.dw[2:] == CANARY).all()) and bool((self.db[2:] == CANARY).all()), "rows / entries 2.. of the padded gradients"
        assert bool((self.ws[self.need:] == 0xA5).all()), "behind ws_bytes of workspace"
        if ldx > Cc:
            assert bool((self.dx.base[..., Cc:] == 7.0).all()), "dx beyond its channels"


def _oracle(x, dy, w, b):
    wq = X.bf16(w)                                               # rounded to bf16 on load
    P = x.shape[0] * x.shape[1] * x.shape[2]
    x2, d2 = x.reshape(P, -1), dy.reshape(P, 2)
    y = x2 @ wq.T + b
    dx = d2 @ wq
    dw = d2.T @ x2
    db = d2.sum(0)
    absb = dict(y=x2.abs() @ wq.abs().T + b.abs(), dx=d2.abs() @ wq.abs(), dw=d2.abs().T @ x2.abs(), db=d2.abs().sum(0))
    return y, dx, dw, db, absb, wq


@pytest.mark.parametrize("kind", ["int", "uniform"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_head1x1_against_the_oracle(U, shape, kind):
    ops = U.ops
    B, H, W, Cc, ldx = shape
    P = B * H * W
    assert ops.head1x1_supported(Cc) in (0, 1, 2, 3)
    x, dy, w, b = _data(kind, B, H, W, Cc)
    y, dx, dw, db, absb, wq = _oracle(x, dy, w, b)
    bufs = _Bufs(U, shape, x, dy, w, b)
    bufs.fwd(U)
    bufs.bwd(U)
    torch.cuda.synchronize()
    bufs.canaries_intact()
    got_y, got_dx = bufs.y.base[..., :2].reshape(P, 2), bufs.dx.base[..., :Cc].reshape(P, Cc)
    assert float(bufs.y.base[..., 2:4].abs().max()) == 0.0, "y[..., 2:4] is exactly zero"
    if kind == "int":
        X.assert_exact(got_y, y, f"y {shape}")
        X.assert_exact(got_dx, X.bf16(dx), f"dx {shape}")
        X.assert_exact(bufs.dw[:2], dw, f"dw {shape}")
        X.assert_exact(bufs.db[:2], db, f"dbias {shape}")
        # the generic path on the same data: the same bits (its forward pass stores bf16 logits: the rounding of these)
        g = ops.geom(B, H, W, Cc, PAD, 1, 1)
        wh = torch.zeros((PAD, 1, 1, Cc), dtype=torch.bfloat16, device=DEV)
        wh[:2, 0, 0] = w.to(DEV).to(torch.bfloat16)
        wth = wh.permute(3, 1, 2, 0).contiguous()
        yg = ops.new_act(B, H, W, PAD, DEV, dtype=torch.bfloat16)
        dxg = ops.Act(torch.full((B, H, W, ldx), 7.0, dtype=torch.bfloat16, device=DEV), 0, Cc)
        dwg, dbg = torch.zeros((PAD, 1, 1, Cc), device=DEV), torch.zeros(PAD, device=DEV)
        dyz = ops.Act(bufs.dy.base.clone(), 0, PAD)
        dyz.base[..., 2:] = 0.0                                  # the generic kernels read all 8 channels
        ws = ops.Workspace(DEV)
        ops.conv2d_fwd(g, bufs.x, wh, bufs.bias, yg)
        ops.conv2d_dgrad(g, dyz, wth, dxg)
        ops.conv2d_wgrad(g, bufs.x, dyz, dwg, ws)
        ops.colsum(dyz, dbg, ws)
        torch.cuda.synchronize()
        X.assert_exact(yg.base[..., :2].reshape(P, 2), X.bf16(got_y.double().cpu()), f"generic y {shape}")
        X.assert_exact(dxg.base[..., :Cc].reshape(P, Cc), got_dx.double().cpu(), f"generic dx {shape}")
        X.assert_exact(dwg.reshape(PAD, Cc)[:2], bufs.dw[:2].double().cpu(), f"generic dw {shape}")
        X.assert_exact(dbg[:2], bufs.db[:2].double().cpu(), f"generic dbias {shape}")
    else:
        # fp32 sums of n terms in any order (products of two bf16 numbers are exact in fp32): n * 2^-24 * sum |terms|
        S.check(got_y, y, (Cc + 1) * S.U32 * absb["y"], f"y {shape}", "head1x1_fwd")
        # dx is a sum of TWO products that are exact in fp32 (bf16 x bf16): the fp32 sum is ONE rounding of the exact value - and so is
        # an fma, whose product is exact too - so the value before the store is DETERMINED, fl32(dx), and the stored one is its bf16
        # rounding: equality in every element (d = 0).  An interval bound would leave the exact bf16 ties undecided, and a sum of two
        # 16-bit products is one in about 1 % of the elements.
        assert bool((dx.abs() <= absb["dx"]).all())
        S.check(got_dx, dx.float().double(), 0.0, f"dx {shape}", "head1x1_bwd dx")
        S.check(bufs.dw[:2], dw, P * S.U32 * absb["dw"], f"dw {shape}", "head1x1_bwd dw")
        S.check(bufs.db[:2], db, P * S.U32 * absb["db"], f"dbias {shape}", "head1x1_bwd dbias")
    # a second run gives the same bits
    first = (bufs.y.base.clone(), bufs.dx.base.clone(), bufs.dw.clone(), bufs.db.clone())
    bufs.fresh()
    bufs.fwd(U)
    bufs.bwd(U)
    torch.cuda.synchronize()
    for a_, b_ in zip(first, (bufs.y.base, bufs.dx.base, bufs.dw, bufs.db)):
        assert torch.equal(a_, b_)


def test_the_pair_of_launches_replays_in_a_captured_graph_to_the_same_bits(U):
    shape = (2, 144, 160, 64, 64)
    B, H, W, Cc, ldx = shape
    bufs = _Bufs(U, shape, *_data("uniform", B, H, W, Cc))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                   # warm-up outside the capture
        bufs.fwd(U)
        bufs.bwd(U)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = (bufs.y.base.clone(), bufs.dx.base.clone(), bufs.dw.clone(), bufs.db.clone())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        bufs.fwd(U)
        bufs.bwd(U)
    for _ in range(2):
        bufs.y.base.fill_(CANARY); bufs.dx.base.fill_(7.0); bufs.dw.fill_(CANARY); bufs.db.fill_(CANARY)
        graph.replay()
        torch.cuda.synchronize()
        for a_, b_ in zip(eager, (bufs.y.base, bufs.dx.base, bufs.dw, bufs.db)):
            assert torch.equal(a_, b_)
        bufs.canaries_intact()


def test_slab_count_is_a_function_of_the_shape_alone(U):
    """The workspace query fixes the number of slabs: [2 C + 8] floats each, one per workgroup, from (B, H, W, C) - no device property."""
    q = U.ops.head1x1_bwd_ws_bytes
    assert q(1, 1, 1, 8) == (2 * 8 + 8) * 4
    assert q(1, 33, 17, 32) == 3 * (2 * 32 + 8) * 4                   # 561 pixels: blocks of 256
    assert q(2, 144, 160, 64) == 180 * (2 * 64 + 8) * 4
    assert q(32, 144, 160, 32) == 1024 * (2 * 32 + 8) * 4             # the default head: 1024 blocks of 720 pixels
    assert q(1, 1, 1, 12) == 0 and q(1, 1, 1, 264) == 0


def test_strides_that_rule_out_vector_accesses_take_the_scalar_paths(U):
    """ldy = 6 (rows of y not 16-byte aligned: four scalar stores instead of one float4) and lddy = 9 (odd: two 2-byte loads of dy
    instead of one 4-byte load) are valid strides of the C entry points (ldy >= 4, lddy >= 8), though ops.Act cannot describe
    them: raw buffers, integer data, every stored element equal to the oracle, canaries in the gaps."""
    B, H, W, Cc, ldy, lddy = 1, 33, 17, 32, 6, 9
    P = B * H * W
    x, dy, w, b = _data("int", B, H, W, Cc)
    y, dx, dw, db, _, _ = _oracle(x, dy, w, b)
    xb = x.to(DEV).to(torch.bfloat16).contiguous()
    dyb = torch.full((P, lddy), 3.0, dtype=torch.bfloat16, device=DEV)
    dyb[:, :2] = dy.reshape(P, 2).to(DEV).to(torch.bfloat16)
    wd = torch.zeros((PAD, Cc), dtype=torch.float32, device=DEV)
    wd[:2] = w.float().to(DEV)
    bd = torch.zeros(PAD, dtype=torch.float32, device=DEV)
    bd[:2] = b.float().to(DEV)
    yb = torch.full((P, ldy), CANARY, dtype=torch.float32, device=DEV)
    dxb = torch.full((P, Cc), 7.0, dtype=torch.bfloat16, device=DEV)
    dwb, dbb = torch.full((PAD, Cc), CANARY, dtype=torch.float32, device=DEV), torch.full((PAD,), CANARY, dtype=torch.float32, device=DEV)
    need = U.ops.head1x1_bwd_ws_bytes(B, H, W, Cc)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L = U._lib.lib()
    assert L.unetrir_head1x1_fwd_bf16(p(xb), Cc, B, H, W, Cc, p(wd), p(bd), p(yb), ldy, s) == 0
    assert L.unetrir_head1x1_bwd_bf16(p(xb), Cc, p(dyb), lddy, B, H, W, Cc, p(wd), p(dxb), Cc, p(dwb), p(dbb), p(ws), need, s) == 0
    torch.cuda.synchronize()
    X.assert_exact(yb[:, :2], y, "y, ldy = 6")
    assert float(yb[:, 2:4].abs().max()) == 0.0 and bool((yb[:, 4:] == CANARY).all())
    X.assert_exact(dxb, X.bf16(dx), "dx, lddy = 9")
    X.assert_exact(dwb[:2], dw, "dw, lddy = 9")
    X.assert_exact(dbb[:2], db, "dbias, lddy = 9")
    assert bool((dwb[2:] == CANARY).all()) and bool((dbb[2:] == CANARY).all()) and bool((ws[need:] == 0xA5).all())
    assert bool((dyb[:, 2:] == 3.0).all())
