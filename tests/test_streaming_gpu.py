"""Every streaming kernel of csrc/elementwise.hip against an fp64 reference, ELEMENT BY ELEMENT, with the criterion and the bounds
of tests/streaming_check.py (no tolerance relative to a tensor's largest value), at the shapes and on the data that reach every
path of the kernels - and the workspace contract of every entry point that takes (ws, ws_bytes), pinned with a guard band.

Shape table of the BatchNorm family (V = 4 fp32 / 8 bf16 channels per lane, CQ = C / V channel vectors per pixel):
  row 1  one vector per pixel, 256 rows per block             fp32 C = 4, bf16 C = 8;  P = 5, 240, 70 000
  row 2  idle lanes in the last channel group (CQ = 3, 5),    C = 24, 40 (bf16), 12, 20, 40 (fp32), 96, 160; P = 240 and P with
         the re-fetching loops (grid * 256 % CQ != 0)          P * CQ > 2^20: the grid is capped at 4096 blocks, its stride 2^20
  row 3  register-resident parameters, several loop passes    C = 64, 128; same two sizes
  row 4  two and more channel groups (CQ > 256)               C = 1536, 2048 at P = 16 384; C = 4096 at P = 8 192
  row 5  slab counts 1, 2, many, 2048                         follows from the sizes above
  row 6  strides: ld > C, channel offset c0 > 0, poison       the P = 240 cases of rows 1-3, input and output strides different
  row 7  finalize guards: C not a multiple of FIN_CH = 8      fp32 C = 4, 12, 20
Data kinds: zero-centred uniform with unit spread, and OFFSET data (streaming_check / make_x)."""
import math

import numpy as np
import pytest
import torch

import streaming_check as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS, MOM = 1e-3, 0.99
COLSTAT_RSTD = []          # (case, observed |rstd - fp64| / rstd, derived bound / rstd) of the fused-statistics tables


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    tot = dict(comparisons=sum(s["comparisons"] for s in S.STATS.values()), elements=sum(s["elements"] for s in S.STATS.values()))
    print("\nelement-wise comparisons of this process:", tot)
    for k in sorted(S.STATS):
        s = S.STATS[k]
        print(f"  {k:24s} {s['comparisons']:5d} comparisons {s['elements']:12d} elements  largest undecided share {s['undecided']:.2e}"
              f"  largest error / bound {s['ratio']:.3f}")
    for row in COLSTAT_RSTD:
        print("  colstat rstd:", row)


def gen(seed):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    return g


def urand(g, shape, lo=-1.0, hi=1.0):
    return torch.rand(shape, device=DEV, generator=g, dtype=torch.float64) * (hi - lo) + lo


def make_x(g, P, C, kind, dtype):
    """[P, C] with unit spread per channel.  "centred": mean 0.  "offset": per-channel mean from [-4, 4] (bf16) / [-8, 8] (fp32);
    fp32 tensors also carry channel 1 at +100 and channel 2 at -100 with spread 0.5 and the CONSTANT channel 3 (variance 0)."""
    x = urand(g, (P, C), -3 ** 0.5, 3 ** 0.5)
    if kind == "offset":
        m = urand(g, (C,)) * (4 if dtype == torch.bfloat16 else 8)
        x = x + m
        if dtype == torch.float32:
            x[:, 1] = 100 + 0.5 * (x[:, 1] - m[1]); x[:, 2] = -100 + 0.5 * (x[:, 2] - m[2]); x[:, 3] = m[3]
    return x.to(dtype)


POISON = {torch.float32: 777.0, torch.bfloat16: 768.0}


def embed(ops, t, pad=0, c0=0, fill=None):
    """The [P, C] tensor t as an Act: dense (pad = 0), or channels [c0, c0 + C) of a poisoned [1, 1, P, C + pad] buffer."""
    P, C = t.shape
    base = torch.full((1, 1, P, C + pad), POISON[t.dtype] if fill is None else fill, dtype=t.dtype, device=DEV)
    base[0, 0, :, c0:c0 + C] = t
    return ops.Act(base, c0, C)


def blank(ops, P, C, dtype, pad=0, c0=0):
    return embed(ops, torch.zeros((P, C), dtype=dtype, device=DEV), pad, c0)


def flat(a):
    return a.base[0, 0, :, a.c0:a.c0 + a.C]


def poison_intact(a):
    b = a.base[0, 0]
    rest = torch.cat([b[:, :a.c0], b[:, a.c0 + a.C:]], dim=1)
    return bool((rest == POISON[a.base.dtype]).all())


# ----------------------------------------------------------------------------------------------------------------------
# A. the workspace contract: ws_bytes = exactly the advertised size, everything behind it is a canary
# ----------------------------------------------------------------------------------------------------------------------
CANARY = 0xA5


class Guarded:
    """A Workspace whose buffer is the first `adv` bytes of a larger allocation filled with a byte pattern."""

    def __init__(self, ops, adv, total):
        assert total > adv
        self.big = torch.full((int(total),), CANARY, dtype=torch.uint8, device=DEV)
        self.ws = ops.Workspace(DEV)
        self.ws.buf = self.big[:int(adv)]
        self.adv = int(adv)

    def assert_intact(self, what):
        torch.cuda.synchronize()
        assert self.ws.buf.data_ptr() == self.big.data_ptr() and self.ws.nbytes == self.adv, f"{what}: the wrapper asked for more than the advertised size"
        tail = self.big[self.adv:]
        n = int((tail != CANARY).sum())
        if n:
            first = int((tail != CANARY).nonzero()[0])
            last = int((tail != CANARY).nonzero()[-1])
            raise AssertionError(f"{what}: {n} bytes behind the advertised workspace size ({self.adv}) were overwritten, "
                                 f"offsets {self.adv + first} ... {self.adv + last}")


def bn_family_calls(ops, P, C, dtype, seed):
    """name -> function(ws) returning the outputs of one BatchNorm-family entry point on fixed inputs."""
    g = gen(seed)
    x = embed(ops, make_x(g, P, C, "centred", dtype)); da = embed(ops, make_x(g, P, C, "centred", dtype))
    gamma, beta = urand(g, (C,), 0.5, 1.5).float(), urand(g, (C,), -0.5, 0.5).float()
    aff, saved = torch.zeros(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
    ops.bn_stats(x, gamma, beta, aff, saved, ops.Workspace(DEV, 2048 * C * 16 + 8 * C))
    out = blank(ops, P, C, dtype)
    ops.bn_act_add(x, aff, out, act=2, addend=da)
    torch.cuda.synchronize()

    def stats(ws):
        a, s = torch.zeros(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
        ops.bn_stats(x, gamma, beta, a, s, ws)
        return a, s

    def bwd(ws):
        dx, dg, db = blank(ops, P, C, dtype), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.bn_bwd(da, x, gamma, aff, saved, dx, dg, db, ws, relu=1)
        return dx.base, dg, db

    def junction(ws):
        dx, gs, dg, db = blank(ops, P, C, dtype), blank(ops, P, C, dtype), torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.bn_bwd_junction(da, x, out, aff, saved, dx, dg, db, ws, act=2, gskip=gs)
        return dx.base, gs.base, dg, db

    def colsum(ws):
        o = torch.zeros(C, device=DEV)
        ops.colsum(da, o, ws)
        return (o,)

    return dict(bn_stats=stats, bn_bwd=bwd, bn_bwd_junction=junction, colsum=colsum)


# the pairs at which the fp32 and the bf16 plan have different slab counts; two groups with the second partly idle; small shapes
BN_WS_SHAPES = [(2048, 16384), (4096, 8192), (1536, 16384), (64, 70000), (24, 240), (8, 5)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("C,P", BN_WS_SHAPES)
def test_workspace_guard_band_batchnorm_family(U, C, P, dtype):
    """bn_stats, bn_bwd, bn_bwd_junction and colsum with ws_bytes = unetrir_bn_ws_bytes(P, C) exactly.  The enclosing allocation is
    sized from the plan's own ceiling (at most 2048 slabs: 2048 * C * 16 + 8 * C bytes) plus 1 MiB, so a library that
    under-reports its need still writes inside this test's memory: the canary shows it, nothing faults."""
    ops = U.ops
    adv = ops.bn_ws_bytes(P, C)
    total = 2048 * C * 16 + 8 * C + (1 << 20)
    assert 0 < adv < total
    for name, call in bn_family_calls(ops, P, C, dtype, 11).items():
        gd = Guarded(ops, adv, total)
        got = call(gd.ws)
        gd.assert_intact(f"{name} C={C} P={P} {dtype}")
        want = call(ops.Workspace(DEV, total))
        torch.cuda.synchronize()
        for a, b in zip(got, want):
            assert torch.equal(a, b), f"{name}: results differ between the exact and the oversized workspace"


@pytest.mark.parametrize("name", ["sigmoid_loss_f32", "sigmoid_loss_bf16", "sigmoid_loss_ex_f32", "sigmoid_loss_ex_bf16", "sumsq", "dense_fwd",
                                  "dense_dgrad", "head6x6_wgrad_f32", "head6x6_wgrad_bf16", "conv2d_wgrad_f32", "conv2d_wgrad_bf16",
                                  "conv2d_transpose_wgrad_f32", "conv2d_transpose_wgrad_bf16"])
def test_workspace_guard_band_other_entry_points(U, name):
    """The remaining (ws, ws_bytes) entry points at one small shape each, with exactly the size their *_ws_bytes function (or the
    header) advertises and a 1 MiB canary behind it."""
    ops, L = U.ops, U._lib.lib()
    g = gen(13)
    dt = torch.bfloat16 if name.endswith("bf16") else torch.float32
    f32 = lambda *sh: urand(g, sh).float()
    if name.startswith("sigmoid_loss"):
        B, H, W = 2, 33, 17
        logits = ops.Act(f32(B, H, W, 4) * 3); target = urand(g, (B, 2, H, W), 0, 1).float()
        ex = dict(phase_ref=urand(g, (B, 2, H, W), 0, 1).float(), phase_weight=urand(g, (W,), 0, 1).float()) if "_ex" in name else {}
        adv = L.unetrir_loss_ws_bytes(B * H * W)

        def call(ws):
            pr = torch.zeros((B, 2, H, W), device=DEV); out = torch.zeros(4, device=DEV)
            dl = ops.Act(torch.zeros((B, H, W, 4 if dt == torch.float32 else 8), dtype=dt, device=DEV))
            ops.sigmoid_loss(logits, target, 0.9, 1.0 / (2 * H * W * B), pr, dl, out, ws, **ex)
            return pr, dl.base, out
    elif name == "sumsq":
        x = f32(300007); adv = 512 * 8          # include/unetrir.h: ws >= 512 doubles

        def call(ws):
            out = torch.tensor([1.5], device=DEV)
            ops.sumsq(x, 0.001, out, True, ws)
            return (out,)
    elif name in ("dense_fwd", "dense_dgrad"):
        B, K, N = 3, 520, 72
        x, w, b, dy = ops.Act(f32(B, 1, 1, K)), f32(N, K), f32(N), ops.Act(f32(B, 1, 1, N))
        adv = L.unetrir_dense_fwd_ws_bytes(B, K, N) if name == "dense_fwd" else L.unetrir_dense_dgrad_ws_bytes(B, K, N)

        def call(ws):
            if name == "dense_fwd":
                y = ops.Act(torch.zeros((B, 1, 1, N), device=DEV)); ops.dense_fwd(x, w, b, y, ws)
            else:
                y = ops.Act(torch.zeros((B, 1, 1, K), device=DEV)); ops.dense_dgrad(dy, w, y, ws)
            return (y.base,)
    elif name.startswith("head6x6_wgrad"):
        B, H, W, Cc = 2, 20, 37, 32
        x = ops.Act(f32(B, H, W, Cc).to(dt)); ld = 4 if dt == torch.float32 else 8
        dy = ops.Act(torch.zeros((B, H, W, ld), dtype=dt, device=DEV)); dy.base[..., :2] = f32(B, H, W, 2).to(dt)
        adv = L.unetrir_head6x6_wgrad_ws_bytes(Cc)

        def call(ws):
            dw = torch.zeros((ld, 6, 6, Cc), device=DEV); ops.head6x6_wgrad(x, dy, dw, ws)
            return (dw,)
    else:
        tr = "transpose" in name
        B, H, W, Ci, Co, k = (2, 12, 40, 48, 72, 3) if tr else (2, 16, 24, 16, 32, 3)
        geo = ops.geom(B, H, W, Ci, Co, k, 2 if tr else 1)
        x = ops.Act(f32(B, H, W, Ci).to(dt)); dy = ops.Act(f32(B, 2 * H if tr else H, 2 * W if tr else W, Co).to(dt))
        w = f32(Ci, k, k, Co) if tr else f32(Co, k, k, Ci)
        adv = ops.conv2d_transpose_wgrad_ws_bytes(geo) if tr else ops.conv2d_wgrad_ws_bytes(geo)

        def call(ws):
            dw = torch.zeros_like(w)
            (ops.conv2d_transpose_wgrad if tr else ops.conv2d_wgrad)(geo, x, dy, dw, ws, reg=0.002, w=w)
            return (dw,)
    gd = Guarded(ops, adv, adv + (1 << 20))
    got = call(gd.ws)
    gd.assert_intact(name)
    want = call(ops.Workspace(DEV, adv + (1 << 20)))
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b), f"{name}: results differ between the exact and the oversized workspace"


# ----------------------------------------------------------------------------------------------------------------------
# C. the BatchNorm family
# ----------------------------------------------------------------------------------------------------------------------
def bn_chain(ops, C, P, dtype, kind, strided, seed, gamma_beta=True):
    """Every kernel of the family on one tensor, each output against its fp64 reference; what one pass hands to the next is
    checked, then read back and used as given."""
    g = gen(seed)
    al = 4 if dtype == torch.float32 else 8
    tag = f"C={C} P={P} {str(dtype)[6:]} {kind}{' strided' if strided else ''}"
    pads = [(2 * al, al), (al, 0), (3 * al, 2 * al)] if strided else [(0, 0)] * 3          # (pad, c0): inputs, outputs, gradients
    x64 = make_x(g, P, C, kind, dtype)
    x = embed(ops, x64, *pads[0])
    da = embed(ops, make_x(g, P, C, "centred", dtype), *pads[2])
    skip = embed(ops, make_x(g, P, C, "centred", dtype), *pads[0])
    gamma = urand(g, (C,), 0.5, 1.5).float() if gamma_beta else None
    beta = urand(g, (C,), -0.5, 0.5).float() if gamma_beta else None
    mm0, mv0 = urand(g, (C,)).float(), urand(g, (C,), 0.5, 1.5).float()
    mm, mv = mm0.clone(), mv0.clone()
    aff, saved = torch.zeros(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
    ws = ops.Workspace(DEV)
    xv, dav, skv = flat(x), flat(da), flat(skip)

    # statistics: saved, affine, moving statistics (with them here; without and with gamma / beta NULL in the callers' second run)
    if gamma_beta:
        ops.bn_stats(x, gamma, beta, aff, saved, ws, mm, mv, eps=EPS, momentum=MOM)
    else:
        ops.bn_stats(x, None, None, aff, saved, ws, eps=EPS, momentum=MOM)
    torch.cuda.synchronize()
    st = S.stats_ref(xv, EPS)
    mean_f, rstd_f, scale_f, shift_f = saved[:C], saved[C:], aff[:C], aff[C:]
    S.check(mean_f, st["mean"], st["d_mean"], f"mean {tag}", "bn_stats")
    S.check(rstd_f, st["rstd"], st["d_rstd"], f"rstd {tag}", "bn_stats")
    S.check(scale_f, *S.scale_ref(rstd_f, gamma), f"scale {tag}", "bn_stats")
    S.check(shift_f, *S.shift_ref(mean_f, scale_f, beta), f"shift {tag}", "bn_stats")
    if gamma_beta:
        ref, d, om = S.moving_ref(mm0, mean_f, MOM)
        S.check(mm, ref, d, f"moving mean {tag}", "bn_stats")
        unb = st["var"] * (P / (P - 1.0)) if P > 1 else st["var"]
        # the batch value is (float)unb: one more conversion than moving_ref counts, and the fp64 variance carries e_var
        ref, d, om = S.moving_ref(mv0, unb, MOM)
        S.check(mv, ref, d + om * (S.U32 * unb + st["e_var"] * P / max(P - 1.0, 1.0)), f"moving variance {tag}", "bn_stats")
    else:
        assert torch.equal(mm, mm0) and torch.equal(mv, mv0)

    # forward: bn_apply (relu 0 / 1), bn_act_add (act 0 / 1 / 2, with and without addend), relu_fwd
    outs = {}
    for act in (0, 1):
        y = blank(ops, P, C, dtype, *pads[1])
        ops.bn_apply(x, aff, y, relu=act)
        torch.cuda.synchronize()
        S.check(flat(y), *S.apply_ref(xv, scale_f, shift_f, None, act), f"bn_apply relu {act} {tag}", "bn_apply", act)
        assert poison_intact(y)
        outs[act] = y
    for act in (0, 1, 2):
        for addend in (None, skip):
            y = blank(ops, P, C, dtype, *pads[1])
            ops.bn_act_add(x, aff, y, act=act, addend=addend)
            torch.cuda.synchronize()
            S.check(flat(y), *S.apply_ref(xv, scale_f, shift_f, None if addend is None else skv, act),
                    f"bn_act_add act {act} addend {addend is not None} {tag}", "bn_act_add", act)
            assert poison_intact(y)
            if addend is None and act == 2:
                outs[2] = y
            if addend is not None and act:
                outs[("j", act)] = y
    y = blank(ops, P, C, dtype, *pads[1])
    ops.relu_fwd(x, y)
    torch.cuda.synchronize()
    assert torch.equal(flat(y), torch.relu(xv)), f"relu_fwd {tag}"
    S.note("relu_fwd", xv.numel(), 0.0 if dtype == torch.bfloat16 else None)

    # backward: bn_bwd (relu 0 / 1 / 2), the activation decisions taken from the library's own stored forward output
    cs = torch.zeros(C, device=DEV)
    ops.colsum(da, cs, ws)
    torch.cuda.synchronize()
    ref = dav.double().sum(0)
    S.check(cs, ref, S.U32 * ref.abs() + P * S.U64 * dav.double().abs().sum(0), f"colsum {tag}", "colsum")
    for act in (0, 1, 2):
        dx = blank(ops, P, C, dtype, *pads[1])
        dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        ops.bn_bwd(da, x, gamma, aff, saved, dx, dg, db, ws, relu=act)
        torch.cuda.synchronize()
        mask = flat(outs[act]) > 0
        r = S.bwd_ref(xv, dav, mask, scale_f, mean_f, rstd_f, act)
        S.check(db, r["dbeta"], r["d_dbeta"], f"dbeta relu {act} {tag}", "bn_bwd")
        S.check(dg, r["dgamma"], r["d_dgamma"], f"dgamma relu {act} {tag}", "bn_bwd")
        S.check(flat(dx), *S.dx_ref(r, scale_f, db, dg, P), f"dx relu {act} {tag}", "bn_bwd dx")
        assert bool(torch.isfinite(flat(dx).float()).all()) and poison_intact(dx)
        del r

    # the junction: out = act(BatchNorm(x) + skip); no gskip, gskip, gskip + gskip_add in place
    for act in (1, 2):
        out = outs[("j", act)]
        mask = flat(out) > 0
        r = S.bwd_ref(xv, dav, mask, scale_f, mean_f, rstd_f, act)
        for variant in ("none", "gskip", "in place"):
            dx = blank(ops, P, C, dtype, *pads[1])
            dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
            acc0 = make_x(gen(seed + 1), P, C, "centred", dtype)
            gs = embed(ops, acc0, *pads[2]) if variant != "none" else None
            ops.bn_bwd_junction(da, x, out, aff, saved, dx, dg, db, ws, act=act, gskip=gs, gskip_add=gs if variant == "in place" else None)
            torch.cuda.synchronize()
            S.check(db, r["dbeta"], r["d_dbeta"], f"junction dbeta act {act} {variant} {tag}", "bn_bwd_junction")
            S.check(dg, r["dgamma"], r["d_dgamma"], f"junction dgamma act {act} {variant} {tag}", "bn_bwd_junction")
            S.check(flat(dx), *S.dx_ref(r, scale_f, db, dg, P), f"junction dx act {act} {variant} {tag}", "bn_bwd_junction dx")
            assert poison_intact(dx)
            if gs is not None:
                S.check_interval(flat(gs), *S.gskip_interval(dav, mask, act, acc0 if variant == "in place" else None),
                                 f"junction gskip act {act} {variant} {tag}", "bn_bwd_junction gskip")
                assert poison_intact(gs)
        # act_bwd: g = da * act'(out), one IEEE product: determined
        gout = blank(ops, P, C, dtype, *pads[1])
        ops.act_bwd(da, out, gout, act=act)
        torch.cuda.synchronize()
        S.check_interval(flat(gout), *S.gskip_interval(dav, mask, act), f"act_bwd act {act} {tag}", "act_bwd")
        assert poison_intact(gout)
        del r
    dx = blank(ops, P, C, dtype, *pads[1])
    ops.relu_bwd(da, x, dx)
    torch.cuda.synchronize()
    assert torch.equal(flat(dx).double(), torch.where(xv > 0, dav, torch.zeros_like(dav)).double()), f"relu_bwd {tag}"
    S.note("relu_bwd", xv.numel(), 0.0 if dtype == torch.bfloat16 else None)
    assert poison_intact(x) and poison_intact(da) and poison_intact(skip)


F32, BF16 = torch.float32, torch.bfloat16
BN_CASES = [
    # C, P, dtype, strided                                              the row of the shape table the case is there for
    (4, 5, F32, False), (4, 240, F32, True), (4, 70000, F32, False),    # rows 1, 6, 7: one vector per pixel; C < FIN_CH
    (8, 5, BF16, False), (8, 240, BF16, True), (8, 70000, BF16, False),  # row 1
    (24, 240, BF16, True), (40, 240, BF16, True),                        # rows 2, 6: CQ = 3, 5 - idle lanes, re-fetching loops
    (12, 240, F32, True), (20, 240, F32, True), (40, 240, F32, False),   # rows 2, 6, 7: CQ = 3, 5, 10; C % 8 != 0
    (96, 240, BF16, True), (160, 240, BF16, False), (96, 240, F32, False), (160, 240, F32, True),   # row 2: CQ = 12, 20, 24, 40
    (24, 350000, BF16, False), (160, 53000, BF16, False),                # row 2 at the capped grid (P * CQ > 2^20), bf16
    (12, 350000, F32, False), (40, 105000, F32, False),                  # row 2 at the capped grid, fp32
    (64, 240, BF16, True), (128, 240, BF16, False), (64, 240, F32, False), (128, 240, F32, True),   # rows 3, 6: CQ divides 256
    (64, 132000, BF16, False), (64, 66000, F32, False),                  # row 3 at the capped grid: several passes, parameters in registers
    (1536, 16384, BF16, False), (2048, 16384, BF16, False), (4096, 8192, BF16, False),   # row 4 (and row 5: 1024 / 2048 slabs), bf16
    (1536, 16384, F32, False), (2048, 16384, F32, False), (4096, 8192, F32, False),      # row 4, fp32
    # BatchNorm -> ReLU / LeakyReLU of the Autoencoder and the VAE at main_training.py's size (tests/ae_vae_cases.py BN_PAIRS): batch 32 of
    # 72 x 80, 36 x 40, 18 x 20 and 9 x 10 pixels, both storage types
    (64, 184320, BF16, False), (128, 46080, BF16, False), (256, 11520, BF16, False), (512, 2880, BF16, False),
    (64, 184320, F32, False), (128, 46080, F32, False), (256, 11520, F32, False), (512, 2880, F32, False),
]


@pytest.mark.parametrize("kind", ["centred", "offset"])
@pytest.mark.parametrize("C,P,dtype,strided", BN_CASES, ids=[f"{c}-{p}-{str(t)[6:]}{'-strided' if s else ''}" for c, p, t, s in BN_CASES])
def test_batchnorm_family_element_by_element(U, C, P, dtype, strided, kind):
    bn_chain(U.ops, C, P, dtype, kind, strided, seed=1000 + C + P % 997)


@pytest.mark.parametrize("C,P,dtype", [(20, 240, F32), (40, 240, BF16), (1536, 16384, BF16)], ids=["20-f32", "40-bf16", "1536-bf16"])
def test_batchnorm_statistics_without_gamma_beta_and_moving_statistics(U, C, P, dtype):
    """gamma / beta NULL (scale = rstd, shift = -mean * scale) and no moving statistics; the chain behind them as above."""
    bn_chain(U.ops, C, P, dtype, "offset", False, seed=77, gamma_beta=False)


def colstat_table(t, rows, ldc, c0):
    """The [rows][ldc][2] fp32 table a convolution epilogue would have written for the [P, C] tensor t: `rows` contiguous row
    chunks, per chunk and channel (sum, sum of squares) accumulated in fp64 and stored as fp32; other columns poisoned."""
    P, C = t.shape
    rid = (torch.arange(P, device=DEV) * rows) // P
    t64 = t.double()
    tab = torch.full((rows, ldc, 2), 7.0, device=DEV)
    s = torch.zeros((rows, C), dtype=torch.float64, device=DEV).index_add_(0, rid, t64)
    ss = torch.zeros((rows, C), dtype=torch.float64, device=DEV).index_add_(0, rid, t64 * t64)
    tab[:, c0:c0 + C, 0] = s.float(); tab[:, c0:c0 + C, 1] = ss.float()
    return tab


@pytest.mark.parametrize("kind", ["centred", "offset"])
@pytest.mark.parametrize("rows", [1, 7, 128, 129, 2048, 5000])
@pytest.mark.parametrize("C,dtype", [(20, F32), (24, BF16), (64, BF16)], ids=["20-f32", "24-bf16", "64-bf16"])
def test_colstat_kernels_on_synthetic_tables(U, C, dtype, rows, kind):
    """bn_stats_colstat, bn_colstat_act_add and colsum_colstat on tables built on the host, apart from the convolutions.  The
    kernels sum fp32 table entries in fp64: against the fp64 sums of THE TABLE the bounds are those of bn_stats.  Against the
    fp64 statistics of THE TENSOR the distance is bounded by the table's own precision - 2^-24 * sum over rows |row value| for
    each column, propagated through ss / P - mean^2 - asserted, and recorded with the observed figure."""
    ops = U.ops
    P = 10000
    g = gen(300 + rows + C)
    t = make_x(g, P, C, kind, dtype)
    gamma, beta = urand(g, (C,), 0.5, 1.5).float(), urand(g, (C,), -0.5, 0.5).float()
    tab = colstat_table(t, rows, C, 0)
    T = tab.double()
    s, ss = T[:, :, 0].sum(0), T[:, :, 1].sum(0)
    mean = s / P
    var = (ss / P - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + EPS)
    # fp64 accumulation of `rows` entries, and the subtraction's operands
    e_var = rows * S.U64 * (T[:, :, 1].abs().sum(0) / P + 2 * mean.abs() * T[:, :, 0].abs().sum(0) / P) + 4 * S.U64 * (ss / P + mean * mean)
    aff, saved = torch.zeros(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
    mm0, mv0 = urand(g, (C,)).float(), urand(g, (C,), 0.5, 1.5).float()
    mm, mv = mm0.clone(), mv0.clone()
    ops.bn_stats_colstat(tab, rows, P, C, gamma, beta, aff, saved, mm, mv, eps=EPS, momentum=MOM)
    torch.cuda.synchronize()
    tag = f"colstat C={C} rows={rows} {kind}"
    S.check(saved[:C], mean, S.U32 * mean.abs() + rows * S.U64 * T[:, :, 0].abs().sum(0) / P, f"mean {tag}", "bn_stats_colstat")
    S.check(saved[C:], rstd, S.U32 * rstd + 0.5 * rstd ** 3 * e_var, f"rstd {tag}", "bn_stats_colstat")
    S.check(aff[:C], *S.scale_ref(saved[C:], gamma), f"scale {tag}", "bn_stats_colstat")
    S.check(aff[C:], *S.shift_ref(saved[:C], aff[:C], beta), f"shift {tag}", "bn_stats_colstat")
    ref, d, om = S.moving_ref(mm0, saved[:C], MOM)
    S.check(mm, ref, d, f"moving mean {tag}", "bn_stats_colstat")
    unb = var * (P / (P - 1.0))
    ref, d, om = S.moving_ref(mv0, unb, MOM)
    S.check(mv, ref, d + om * (S.U32 * unb + e_var * P / (P - 1.0)), f"moving variance {tag}", "bn_stats_colstat")
    # against the tensor itself: the table's precision
    st = S.stats_ref(t, EPS)
    t_var = S.U32 * (T[:, :, 1].abs().sum(0) / P + 2 * st["mean"].abs() * T[:, :, 0].abs().sum(0) / P) + e_var + st["e_var"]
    t_rstd = S.U32 * st["rstd"] + 0.5 * torch.maximum(st["rstd"], rstd) ** 3 * t_var * (1 + 1e-3)
    S.check(saved[C:], st["rstd"], t_rstd, f"rstd against the tensor {tag}", "bn_stats_colstat (tensor)")
    obs = ((saved[C:].double() - st["rstd"]).abs() / st["rstd"])
    c = int(obs.argmax())
    COLSTAT_RSTD.append((tag, f"observed {float(obs[c]):.2e}", f"bound {float(t_rstd[c] / st['rstd'][c]):.2e}",
                         f"channel mean {float(st['mean'][c]):.3g} spread {float(st['var'][c]) ** 0.5:.3g}"))

    # the fused form: the same finalize, then the apply
    x = embed(ops, t)
    skip = embed(ops, make_x(g, P, C, "centred", dtype))
    for act, addend in ((2, skip), (1, None), (0, None)):
        aff2, saved2 = torch.zeros(2 * C, device=DEV), torch.zeros(2 * C, device=DEV)
        y = blank(ops, P, C, dtype)
        ops.bn_colstat_act_add(tab, rows, x, gamma, beta, aff2, saved2, y, act=act, addend=addend, eps=EPS, momentum=MOM)
        torch.cuda.synchronize()
        assert torch.equal(aff2, aff) and torch.equal(saved2, saved)
        S.check(flat(y), *S.apply_ref(t, aff2[:C], aff2[C:], None if addend is None else flat(skip), act), f"bn_colstat_act_add act {act} {tag}",
                "bn_colstat_act_add", act)
    # colsum_colstat: channels [c0, c0 + n) of a wider table
    ldc, c0, n = C + 16, 8, C - 4
    wide = colstat_table(t, rows, ldc, 4)           # the tensor's channels sit at 4 ... 4 + C: the slice starts at its channel 4
    out = torch.full((n + 4,), 5.0, device=DEV)
    ops.colsum_colstat(wide, rows, ldc, c0, n, out)
    torch.cuda.synchronize()
    W = wide.double()[:, c0:c0 + n, 0]
    ref = W.sum(0)
    S.check(out[:n], ref, S.U32 * ref.abs() + rows * S.U64 * W.abs().sum(0), f"colsum_colstat {tag}", "colsum_colstat")
    assert bool((out[n:] == 5.0).all())


# ----------------------------------------------------------------------------------------------------------------------
# loss
# ----------------------------------------------------------------------------------------------------------------------
TWO_PI_F = float(torch.tensor(6.283185307179586, dtype=torch.float32))
PI_F = float(torch.tensor(3.141592653589793, dtype=torch.float32))
FLT_MAX = 3.4028234663852886e38


def sigmoid_ref(z):
    """p = 1.f / (1.f + expf(-z)): expf within 1 ulp = 2 * 2^-24 relative (HIP math API, single precision), the sum and the
    quotient one rounding each -> 4 * 2^-24 relative.  Saturation is what fp32 says: where e^-z exceeds FLT_MAX, expf returns inf
    and the quotient is exactly 0; where e^-z is below 2^-24, 1.f + e^-z rounds to 1 and the prediction is exactly 1 (no bound:
    the gradient factor 1 - p is then exactly 0 as well)."""
    z = z.double()
    t = torch.exp(-z)
    over, one = t > FLT_MAX * (1 + 1e-6), t < 2.0 ** -24 * (1 - 1e-6)
    p = torch.where(over, torch.zeros_like(t), torch.where(one, torch.ones_like(t), 1 / (1 + t)))
    return p, torch.where(over | one, torch.zeros_like(t), 4 * S.U32 * p)


def loss_ref(z, target, alpha, inv_norm, phase_ref=None, phase_w=None):
    """fp64 reference and bounds of sigmoid_loss_kernel for logits z [B, H, W, 2] and target [B, 2, H, W]; returns the per-element
    references (NHWC order) and the three sums."""
    a32 = float(torch.tensor(alpha, dtype=torch.float32)); inv32 = float(torch.tensor(inv_norm, dtype=torch.float32))
    oma32 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(alpha, dtype=torch.float32))
    B, _, H, W = target.shape
    p0, dp0 = sigmoid_ref(z[..., 0]); p1, dp1 = sigmoid_ref(z[..., 1])
    t0 = target[:, 0].double(); t1 = target[:, 1].double()
    e_t1 = torch.zeros_like(t1)
    if phase_ref is not None:
        t1 = t1 - phase_ref[:, 1].double(); e_t1 = S.U32 * t1.abs()
    w = torch.ones_like(t1) if phase_w is None else phase_w.double().view(1, 1, W).expand_as(t1)
    # amplitude: da = t0 - p0 (one rounding, and p0's own error); the addend da * da one more
    da = t0 - p0
    e_da = S.U32 * da.abs() + dp0
    e_sq = 2 * da.abs() * e_da + S.U32 * da * da
    # phase argument: every fp32 operation errs by at most 2^-24 of ITS result.  yt = t1 2pi - pi and yp = p1 2pi - pi (product,
    # difference), d1 = yt - yp, dd = d1 + pi, r = dd - floorf(dd / 2pi) 2pi (the floor is an integer of magnitude <= 2, its
    # product with 2pi exact; |r| <= 2pi), ph = r - pi (|ph| <= pi); the inputs' errors times 2pi; and |2pi_f - 2pi| where the
    # kernel's floor and the reference's modulo wrap differently: ph then differs by 2pi_f exactly, sin and cos by that little.
    # 1 - cos and sin are continuous across the wrap, so the fp64 reference with Python's modulo applies and |d sin|, |d cos| <= |d ph|.
    a1, a2 = t1 * TWO_PI_F, p1 * TWO_PI_F
    yt, yp = a1 - PI_F, a2 - PI_F
    d1 = yt - yp
    dd = d1 + PI_F
    e_ph = (S.U32 * (a1.abs() + yt.abs() + a2.abs() + yp.abs() + d1.abs() + dd.abs() + TWO_PI_F + PI_F) + TWO_PI_F * (e_t1 + dp1)
            + abs(TWO_PI_F - 2 * math.pi))
    ph = torch.remainder(dd, TWO_PI_F) - PI_F
    eph = 1 - torch.cos(ph)
    e_eph = e_ph + 2 * S.U32 * torch.cos(ph).abs() + S.U32 * eph.abs()          # cosf within 1 ulp, the difference
    e_ephw = w * e_eph + S.U32 * (eph * w).abs()
    N = da.numel()
    sa, sp, spw = (da * da).sum(), eph.sum(), (eph * w).sum()
    d_sa = S.U32 * sa + e_sq.sum() + N * S.U64 * sa
    d_sp = S.U32 * sp + e_eph.sum() + N * S.U64 * sp
    e_spw = e_ephw.sum() + N * S.U64 * spw
    out0 = (a32 * sa + (1 - a32) * spw) * inv32          # the finalize kernel computes 1.0 - (double)alpha in fp64
    d_out0 = S.U32 * abs(out0) + inv32 * (a32 * (e_sq.sum() + N * S.U64 * sa) + (1 - a32) * e_spw)
    # gradients.  v0 = c0 da p0 q0, c0 = -2 alpha inv (the products with alpha, inv, p0, q0: 4 roundings), q0 = 1.f - p0
    q0, q1 = 1 - p0, 1 - p1
    e_q0, e_q1 = dp0 + S.U32 * q0, dp1 + S.U32 * q1
    c0 = -2 * a32 * inv32
    v0 = c0 * da * p0 * q0
    d_v0 = abs(c0) * (e_da * p0 * q0 + da.abs() * dp0 * q0 + da.abs() * p0 * e_q0) + 4 * S.U32 * v0.abs()
    # v1 = c1 sin(ph) w p1 q1, c1 = -(1.f - alpha) inv 2pi: 1.f - alpha and five products (6), sinf within 1 ulp (2)
    c1 = -oma32 * inv32 * TWO_PI_F
    sn = torch.sin(ph)
    v1 = c1 * sn * w * p1 * q1
    d_v1 = abs(c1) * w * ((e_ph + 2 * S.U32 * sn.abs()) * p1 * q1 + sn.abs() * (dp1 * q1 + p1 * e_q1)) + 6 * S.U32 * v1.abs()
    return dict(p0=p0, dp0=dp0, p1=p1, dp1=dp1, v0=v0, d_v0=d_v0, v1=v1, d_v1=d_v1,
                sums=torch.stack([out0, sa, sp]), d_sums=torch.stack([d_out0, d_sa, d_sp]))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["plain", "phase_ref", "phase_weight", "both"])
@pytest.mark.parametrize("B,H,W,ldl", [(1, 1, 1, 4), (1, 33, 17, 8), (2, 144, 160, 4), (5, 256, 256, 8)])
@pytest.mark.parametrize("data", ["uniform", "saturated", "wrap"])
def test_sigmoid_loss_element_by_element(U, B, H, W, ldl, mode, dt, data):
    """sigmoid_loss / sigmoid_loss_ex, sigmoid_nchw and sigmoid_bwd.  (5, 256, 256) is past the capped grid of 1024 blocks."""
    ops = U.ops
    g = gen(B * H + W + len(mode) + len(data))
    alpha, inv_norm = 0.9, 1.0 / (2 * H * W * B)
    z = urand(g, (B, H, W, 2), -3, 3).float()
    if data == "saturated":
        levels = torch.tensor([20.0, -20.0, 40.0, -40.0, 90.0, -90.0, 200.0, -200.0], device=DEV)
        pick = torch.randint(0, 16, (B, H, W, 2), device=DEV, generator=g)
        z = torch.where(pick < 8, levels[pick % 8], z)
    target = urand(g, (B, 2, H, W), 0, 1).float()
    pref = urand(g, (B, 2, H, W), 0, 1).float() if mode in ("phase_ref", "both") else None
    pw = urand(g, (W,), 0, 1).float() if mode in ("phase_weight", "both") else None
    if data == "wrap":
        # phase targets ON the wrap points: t1 (- phase_ref) - p1 in {0, +-0.5, +-1} up to one fp32 rounding.  sin(ph) is 0 there, so
        # the phase gradient is 0 +- its bound and a bf16 store of it is undecided: with bf16 dlogits one pixel in 160 sits on a wrap
        # point (the cap on the undecided share holds), with fp32 dlogits every pixel does
        p1 = sigmoid_ref(z[..., 1])[0]
        k = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0], device=DEV, dtype=torch.float64)[torch.randint(0, 5, (B, H, W), device=DEV, generator=g)]
        on = p1 + k + (pref[:, 1].double() if pref is not None else 0)
        if dt == BF16:
            pix = torch.arange(B * H * W, device=DEV).view(B, H, W)
            on = torch.where(pix % 160 == 7, on, target[:, 1].double())
        target[:, 1] = on.float()
    logits = ops.Act(torch.full((B, H, W, ldl), 777.0, device=DEV), 0, ldl)
    logits.base[..., :2] = z
    ldd = 4 if dt == F32 else 8
    dl = ops.Act(torch.full((B, H, W, ldd), 9.0, dtype=dt, device=DEV))
    pr = torch.full((B, 2, H, W), -1.0, device=DEV)
    out = torch.full((4,), -1.0, device=DEV)
    ws = ops.Workspace(DEV)
    ops.sigmoid_loss(logits, target, alpha, inv_norm, pr, dl, out, ws, phase_ref=pref, phase_weight=pw)
    torch.cuda.synchronize()
    r = loss_ref(z, target, alpha, inv_norm, pref, pw)
    tag = f"{(B, H, W)} {mode} {data}"
    S.check(pr[:, 0], r["p0"], r["dp0"], f"pred 0 {tag}", "sigmoid_loss pred")
    S.check(pr[:, 1], r["p1"], r["dp1"], f"pred 1 {tag}", "sigmoid_loss pred")
    S.check(dl.base[..., :2], torch.stack([r["v0"], r["v1"]], -1), torch.stack([r["d_v0"], r["d_v1"]], -1), f"dlogits {tag}", "sigmoid_loss dlogits")
    assert float(dl.base[..., 2:].float().abs().max()) == 0.0, "channels 2 ... of dlogits are exact zeros"
    S.check(out[:3], r["sums"], r["d_sums"], f"loss, amplitude sum, phase sum {tag}", "sigmoid_loss sums")
    assert bool(torch.isfinite(out[:3]).all()) and float(out[3]) == -1.0
    assert not bool(torch.isnan(pr).any()) and not bool(torch.isnan(dl.base.float()).any())
    assert bool((logits.base[..., 2:] == 777.0).all())
    if data == "saturated":
        zz = z.permute(0, 3, 1, 2)
        assert bool((pr[zz >= 20] == 1.0).all()) and bool((pr[zz <= -90] == 0.0).all())          # where fp32 says so
        sat = (z >= 20) | (z <= -90)
        assert bool((dl.base[..., :2][sat].float() == 0.0).all()), "gradients are exactly 0 where the prediction saturates"
    pr2 = torch.full_like(pr, -1.0)
    ops.sigmoid_nchw(logits, pr2)
    torch.cuda.synchronize()
    assert torch.equal(pr, pr2)
    # sigmoid_bwd: g * p * (1.f - p) from the stored predictions: 1.f - p and two products, 3 roundings of the result
    dpred = urand(g, (B, 2, H, W)).float()
    dl2 = ops.Act(torch.full((B, H, W, ldd), 9.0, dtype=dt, device=DEV))
    ops.sigmoid_bwd(pr, dpred, dl2)
    torch.cuda.synchronize()
    v = (dpred.double() * pr.double() * (1 - pr.double())).permute(0, 2, 3, 1)
    S.check(dl2.base[..., :2], v, 3 * S.U32 * v.abs(), f"sigmoid_bwd {tag}", "sigmoid_bwd")
    assert float(dl2.base[..., 2:].float().abs().max()) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# optimisers and the step counters
# ----------------------------------------------------------------------------------------------------------------------
def f32c(v):
    return float(torch.tensor(v, dtype=torch.float32))


def one_minus(v):
    """1.f - v as the kernels compute it: in fp32."""
    return float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(v, dtype=torch.float32))


def moments_ref(g, m, v, b1, b2, gs):
    """gk = g * gs (1 rounding);  m' = b1 m + (1.f - b1) gk: two products and the sum on top of gk -> 4 roundings of at most
    |b1 m| + |(1 - b1) gk|;  v' = b2 v + (1.f - b2) gk gk: gk twice (2), two products (2), the sum (1) -> 5."""
    gk = g.double() * f32c(gs)
    a, b = f32c(b1) * m.double(), one_minus(b1) * gk
    c, d = f32c(b2) * v.double(), one_minus(b2) * gk * gk
    return gk, a + b, 4 * S.U32 * (a.abs() + b.abs()), c + d, 5 * S.U32 * (c.abs() + d.abs())


OPT_N = [1, 3, 4, 5, 10007, 8192 * 256 * 4 + 6, 2 * 8192 * 256 * 4 + 13]


def opt_data(n, data, seed):
    g = gen(seed)
    th, gr = urand(g, (n,)).float(), urand(g, (n,)).float()
    m, v = urand(g, (n,), -0.1, 0.1).float(), urand(g, (n,), 0, 0.1).float()
    if data == "small":
        th = th * 1e-4          # small parameters beside nothing large: a bound relative to the maximum would hide them anyway
    if data == "zero":
        gr, m, v = torch.zeros_like(gr), torch.zeros_like(m), torch.zeros_like(v)
    if data == "v tiny":
        v = torch.full_like(v, 1e-30)
    if data == "v huge":
        v = torch.full_like(v, 1e20)
    return th, gr, m, v


# every data set at the sizes up to 10 007, the two sizes past the grid on two of them
ADAM_CASES = [(n, d) for n in OPT_N for d in ("ordinary", "small", "zero", "v tiny", "v huge") if n < 10 ** 6 or d in ("ordinary", "zero")]


@pytest.mark.parametrize("n,data", ADAM_CASES)
def test_adam_element_by_element(U, n, data):
    """adam and adam_dev: tail elements (n % 4), the second 16-byte group absent, the grid-stride loop wrapping (8192 blocks)."""
    ops = U.ops
    th0, gr, m0, v0 = opt_data(n, data, n % 1000 + len(data))
    lr_t, b1, b2, eps, gs = 1e-3 * math.sqrt(1 - 0.999 ** 3) / (1 - 0.9 ** 3), 0.9, 0.999, 1e-7, 0.5
    th, m, v = th0.clone(), m0.clone(), v0.clone()
    ops.adam(th, gr, m, v, lr_t, b1, b2, eps, grad_scale=gs)
    torch.cuda.synchronize()
    gk, rm, dm, rv, dv = moments_ref(gr, m0, v0, b1, b2, gs)
    S.check(m, rm, dm, f"adam m n={n} {data}", "adam")
    S.check(v, rv, dv, f"adam v n={n} {data}", "adam")
    # theta -= lr_t m' / (sqrtf(v') + eps) from the STORED m', v': lr_t * m' (1), sqrtf (1 ulp = 2), + eps (1), the quotient
    # (1 ulp = 2) -> 6 roundings of the update, then the difference: one rounding of at most |theta| + |update|
    upd = f32c(lr_t) * m.double() / (torch.sqrt(v.double()) + f32c(eps))
    S.check(th, th0.double() - upd, S.U32 * (th0.double().abs() + 7 * upd.abs()), f"adam theta n={n} {data}", "adam")
    if data == "zero":
        assert torch.equal(th, th0) and float(m.abs().max()) == 0 and float(v.abs().max()) == 0
    hyper = torch.tensor([lr_t, b1, b2, eps, gs], dtype=torch.float32, device=DEV)
    th2, m2, v2 = th0.clone(), m0.clone(), v0.clone()
    ops.adam_dev(th2, gr, m2, v2, hyper)
    torch.cuda.synchronize()
    assert torch.equal(th2, th) and torch.equal(m2, m) and torch.equal(v2, v), "adam_dev equals adam bit for bit"


@pytest.mark.parametrize("n", OPT_N)
def test_sgd_and_nadam_element_by_element(U, n):
    ops = U.ops
    th0, gr, m0, v0 = opt_data(n, "ordinary", n % 1000)
    lr, gs, b1, b2, eps = 1e-2, 0.5, 0.9, 0.999, 1e-7
    th = th0.clone()
    ops.sgd(th, gr, lr, grad_scale=gs)
    torch.cuda.synchronize()
    # theta -= lr * gs * g: two products, then the difference
    upd = f32c(lr) * f32c(gs) * gr.double()
    S.check(th, th0.double() - upd, S.U32 * (th0.double().abs() + 3 * upd.abs()), f"sgd n={n}", "sgd")
    cg, cm, cv = 0.37, 1.21, 40.0
    th, m, v = th0.clone(), m0.clone(), v0.clone()
    ops.nadam(th, gr, m, v, lr, b1, b2, eps, cg, cm, cv, grad_scale=gs)
    torch.cuda.synchronize()
    gk, rm, dm, rv, dv = moments_ref(gr, m0, v0, b1, b2, gs)
    S.check(m, rm, dm, f"nadam m n={n}", "nadam")
    S.check(v, rv, dv, f"nadam v n={n}", "nadam")
    # theta -= lr (cg gk + cm m') / (sqrtf(cv v') + eps) from the STORED m', v'.  numerator: gk (1) + product (1) + sum (1) on the
    # first term, product + sum on the second; lr * num (1); denominator: cv v' (1, halved by the root), sqrtf (2), + eps (1) -> 4;
    # the quotient (2); then the difference
    a, b = f32c(cg) * gk, f32c(cm) * m.double()
    den = torch.sqrt(f32c(cv) * v.double()) + f32c(eps)
    upd = f32c(lr) * (a + b) / den
    d_upd = f32c(lr) / den * S.U32 * (3 * a.abs() + 2 * b.abs()) + 7 * S.U32 * upd.abs()
    S.check(th, th0.double() - upd, S.U32 * (th0.double().abs() + upd.abs()) + d_upd, f"nadam theta n={n}", "nadam")


def test_step_advance(U):
    ops = U.ops
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-7, 0.25
    cfg = torch.tensor([lr, b1, b2, eps, gs], dtype=torch.float32, device=DEV)
    c = cfg.double().cpu()
    for t in (1, 2, 3, 10, 10 ** 3, 10 ** 5, 10 ** 7):
        state = torch.tensor([t - 1, 40, 0], dtype=torch.int64, device=DEV)
        hyper = torch.full((8,), -1.0, device=DEV)
        ops.step_advance(state, cfg, hyper, 3)
        torch.cuda.synchronize()
        want = float(c[0]) * math.sqrt(1 - float(c[2]) ** t) / (1 - float(c[1]) ** t)
        assert abs(float(hyper[0].double()) - want) <= 2.0 ** -23 * want, (t, float(hyper[0]), want)
        assert torch.equal(hyper[1:5], cfg[1:]) and bool((hyper[5:] == -1.0).all())
        assert state.tolist() == [t, 43, 40]
    state = torch.tensor([0, 5, 1], dtype=torch.int64, device=DEV)
    hyper = torch.full((8,), -1.0, device=DEV)
    ops.step_advance(state, cfg, hyper, 2, advance_t=False)          # a forward-only pass on a fresh engine
    torch.cuda.synchronize()
    assert float(hyper[0]) == 0.0 and torch.equal(hyper[1:5], cfg[1:]) and state.tolist() == [0, 7, 5]
    # adam_dev with the hyper block step_advance wrote == adam with the same five numbers
    state = torch.tensor([6, 0, 0], dtype=torch.int64, device=DEV)
    ops.step_advance(state, cfg, hyper, 0)
    th0, gr, m0, v0 = opt_data(10007, "ordinary", 3)
    a = [t.clone() for t in (th0, m0, v0)]; b = [t.clone() for t in (th0, m0, v0)]
    ops.adam_dev(a[0], gr, a[1], a[2], hyper)
    h = hyper.cpu()
    ops.adam(b[0], gr, b[1], b[2], float(h[0]), float(h[1]), float(h[2]), float(h[3]), grad_scale=float(h[4]))
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------------------------------------------------
# dropout: a fixed function of (seed, draw, index)
# ----------------------------------------------------------------------------------------------------------------------
def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def dropout_restated(n, p, seed, draw):
    """dropout_mask_kernel in NumPy uint64 arithmetic (wrapping products)."""
    with np.errstate(over="ignore"):
        gold = np.uint64(0x9E3779B97F4A7C15)
        key = mix64(np.uint64(seed) * gold + np.uint64(draw))
        r = mix64(key + gold * np.arange(1, n + 1, dtype=np.uint64))
    u = (r >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    return np.where(u >= np.float32(p), keep, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("p", [0.0, 0.1, 0.2, 0.5])
def test_dropout_mask_equals_its_restatement(U, p):
    ops = U.ops
    n = 3 * 2 ** 20 + 5
    seen = []
    for seed in (0, 12345, 2 ** 63 + 11):
        for draw in (0, 1, 7):
            mask = torch.full((n,), -1.0, device=DEV)
            ops.dropout_mask(mask, p, seed, draw)
            state = torch.tensor([0, 0, draw - 1 if draw else 0], dtype=torch.int64, device=DEV)
            dev = torch.full((n,), -1.0, device=DEV)
            ops.dropout_mask_dev(dev, p, seed, state, 1 if draw else 0)          # draw number = state[2] + offset
            torch.cuda.synchronize()
            want = dropout_restated(n, p, seed, draw)
            got = mask.cpu().numpy()
            assert np.array_equal(got, want), (p, seed, draw, int((got != want).sum()))
            assert torch.equal(dev, mask)
            kept = float((got != 0).mean())
            if p > 0:
                z = (kept - (1 - p)) / math.sqrt(p * (1 - p) / n)
                assert abs(z) <= 4, (p, seed, draw, z)
                seen.append(got)
            else:
                assert kept == 1.0 and float(got.min()) == 1.0
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j]), "different (seed, draw) pairs give different masks"
    mask = torch.zeros(16, device=DEV)
    for bad in (1.0, 1.5, float("nan"), -0.1):
        with pytest.raises(U._lib.UnetrirError):
            ops.dropout_mask(mask, bad, 1, 0)


# ----------------------------------------------------------------------------------------------------------------------
# glue
# ----------------------------------------------------------------------------------------------------------------------
def as_act(ops, t):
    return ops.Act(t.view(1, 1, -1, 8))


def bits16(t):
    return t.view(torch.int16)


def test_casts_bit_for_bit(U):
    ops = U.ops
    hi = torch.arange(65536, dtype=torch.int64)
    lows = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)          # ties both ways around 0x8000
    bits = ((hi.view(-1, 1) << 16) | lows.view(1, -1)).reshape(-1)
    a = (bits - ((bits >> 31) << 32)).to(torch.int32).view(torch.float32).to(DEV)                   # all 65 536 upper halves x 6 lower halves
    y = torch.zeros(a.numel(), dtype=BF16, device=DEV)
    ops.cast_f32_to_bf16(as_act(ops, a), as_act(ops, y))
    torch.cuda.synchronize()
    want = a.to(BF16)                                   # torch converts to nearest even
    nan = torch.isnan(a)
    assert bool(torch.isnan(y.float())[nan].all()), "NaN stays NaN"
    assert torch.equal(bits16(y)[~nan], bits16(want)[~nan]), "cast_f32_to_bf16 differs from round-to-nearest-even"
    S.note("cast_f32_to_bf16", a.numel(), 0.0)
    # every bf16 pattern back to fp32: the upper half, exactly
    b = (hi - ((hi >> 15) << 16)).to(torch.int16).view(BF16).to(DEV)
    f = torch.zeros(65536, device=DEV)
    ops.cast_bf16_to_f32(as_act(ops, b), as_act(ops, f))
    torch.cuda.synchronize()
    nanb = torch.isnan(b.float())
    assert torch.equal(f.view(torch.int32)[~nanb], (b.view(torch.int16).to(torch.int32) << 16)[~nanb]) and bool(torch.isnan(f)[nanb].all())
    S.note("cast_bf16_to_f32", 65536, 0.0)
    # add_f32_to_bf16 = bf16(float(a) + b): one fp32 addition, then the store; b chosen so that many sums are exact ties
    g = gen(5)
    n = 1 << 20
    a16 = (urand(g, (n,), -4, 4)).to(BF16)
    b32 = urand(g, (n,), -4, 4).float()
    b32[::2] = (torch.randint(-512, 512, (n // 2,), device=DEV, generator=g).float() + 0.5) * 2.0 ** -7          # half-way points at |sum| in [1, 2)
    y = torch.zeros(n, dtype=BF16, device=DEV)
    ops.add_f32_to_bf16(as_act(ops, a16), as_act(ops, b32), as_act(ops, y))
    torch.cuda.synchronize()
    s32 = a16.float() + b32
    assert torch.equal(bits16(y), bits16(s32.to(BF16)))
    assert int((S.bf16_rne(s32.double()) != S.bf16_trunc(s32.double())).sum()) > n // 4
    from exact_data import is_tie
    assert int(is_tie(s32.double().cpu()).sum()) > 1000, "the data holds exact ties"
    S.note("add_f32_to_bf16", n, 0.0)


def test_add_mul_sumsq_pad_affine_index_embedding(U):
    ops = U.ops
    g = gen(9)
    n = 4096 * 256 * 4 + 8           # past the capped grid of add (4096 blocks of 256 lanes x 4 values)
    a, b = urand(g, (n,)).float(), urand(g, (n,)).float()
    y = torch.zeros(n, device=DEV)
    ops.add(a, b, y)
    m = torch.zeros(n + 3, device=DEV)
    a3, b3 = urand(g, (n + 3,)).float(), urand(g, (n + 3,)).float()
    ops.mul(a3, b3, m)
    torch.cuda.synchronize()
    assert torch.equal(y, a + b) and torch.equal(m, a3 * b3)          # one IEEE operation per element: determined
    # sumsq: out = (float)(coef * sum x^2) (+ out): exact fp64 squares summed in fp64; the conversion, the accumulation
    ws = ops.Workspace(DEV)
    for nn in (1, 255, 300007, 512 * 256 * 3 + 1):
        x = urand(g, (nn,)).float()
        for accumulate in (False, True):
            out = torch.tensor([1.5], device=DEV)
            ops.sumsq(x, 0.001, out, accumulate, ws)
            torch.cuda.synchronize()
            sq = (x.double() ** 2).sum()
            r = f32c(0.001) * sq
            ref = r + (1.5 if accumulate else 0.0)
            d = S.U32 * abs(r) + nn * S.U64 * abs(r) + (S.U32 * abs(ref) if accumulate else 0.0)
            S.check(out, ref.view(1), d.view(1), f"sumsq n={nn} accumulate={accumulate}", "sumsq")
    # nchw_to_nhwc_pad, both types: values exact (bf16: rounded to nearest even), padding exact zeros; past the capped grid
    for B, Cc, H, W, pad in ((2, 2, 5, 7, 4), (1, 3, 9, 4, 8), (5, 2, 512, 512, 8)):
        x = urand(g, (B, Cc, H, W)).float()
        for dt in (F32, BF16):
            if dt == F32 and pad % 4 or dt == BF16 and pad % 8:
                continue
            pa = ops.Act(torch.full((B, H, W, pad), 5.0, dtype=dt, device=DEV))
            ops.nchw_to_nhwc_pad(x, pa)
            torch.cuda.synchronize()
            assert torch.equal(pa.base[..., :Cc], x.permute(0, 2, 3, 1).to(dt)) and float(pa.base[..., Cc:].float().abs().max()) == 0.0
    # bn_inference_affine: scale = g / sqrtf(mv + eps): sum (1), sqrtf (1 ulp = 2), quotient (1 ulp = 2) -> 5; shift from the stored scale
    for Cc in (4, 20, 300):
        gamma, beta = urand(g, (Cc,), 0.5, 1.5).float(), urand(g, (Cc,)).float()
        mm, mv = urand(g, (Cc,), -5, 5).float(), urand(g, (Cc,), 0, 2).float()
        mv[0] = 0.0
        for gm, bt in ((gamma, beta), (None, None)):
            aff = torch.full((2 * Cc + 2,), 3.0, device=DEV)
            ops.bn_inference_affine(gm, bt, mm, mv, EPS, aff)
            torch.cuda.synchronize()
            sc = (1.0 if gm is None else gm.double()) / torch.sqrt(mv.double() + f32c(EPS))
            S.check(aff[:Cc], sc, 5 * S.U32 * sc.abs(), f"inference scale C={Cc}", "bn_inference_affine")
            S.check(aff[Cc:2 * Cc], *S.shift_ref(mm, aff[:Cc], bt), f"inference shift C={Cc}", "bn_inference_affine")
            assert bool((aff[2 * Cc:] == 3.0).all())
    # index_to_i32: int32 and int64 device tensors; a host tensor is refused before any pointer reaches a kernel
    idx = torch.randint(0, 2000, (3, 2, 16), device=DEV, generator=g)
    for it in (torch.int32, torch.int64):
        out = torch.full((idx.numel(),), -1, dtype=torch.int32, device=DEV)
        ops.index_to_i32(idx.to(it), out)
        torch.cuda.synchronize()
        assert torch.equal(out.long(), idx.flatten())
        with pytest.raises(ValueError):
            ops.index_to_i32(idx.to(it).cpu(), out)
    # embedding_bwd: the fp32 sum in index order, bit for bit - id 3 occurs more than 1024 times (the ordered-scan branch)
    n_idx, vocab, dim = 2500, 8, 40
    ids = torch.randint(0, vocab, (n_idx,), device=DEV, generator=g).to(torch.int32)
    ids[torch.randperm(n_idx, device=DEV, generator=g)[:1500]] = 3
    assert int((ids == 3).sum()) > 1024
    dout = urand(g, (n_idx, dim)).float()
    dt = torch.full((vocab, dim), 9.0, device=DEV)
    ops.embedding_bwd(ids, dout, dt)
    torch.cuda.synchronize()
    want = torch.zeros((vocab, dim), dtype=torch.float32)
    hid, hd = ids.cpu().tolist(), dout.cpu()
    for i, v in enumerate(hid):
        want[v] += hd[i]
    assert torch.equal(dt.cpu(), want)
