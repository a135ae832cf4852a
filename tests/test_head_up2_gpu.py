"""The kernels of csrc/head_up2.hip - UpSampling2D((2, 2)) -> Conv2D(2, (6,6), 'same') (dl_models/u_net.py:247-248) folded to the coarse
grid - against the fp64 restatement of tests/head_up2_ref.py (the LITERAL form: repeat_interleave, then the oracle's conv2d_same) and
against their literal twin on the device, in both storage types.

Coarse shapes: (1, 1, 3) every tap meets the padding; (2, 5, 7) odd sizes; (3, 16, 24) several tiles; (1, 6, 160) fine width 320, wider
than the 256-pixel column block of the matrix-core 6x6 head and 10 tiles of the new kernels in a row.  Channels: one count per
channel-chunk class of the weight-gradient kernel (24 = 3 chunks of 8, 16, 64 = 2 chunks of 32); forward and data gradient walk any
multiple of 8 in steps of 8 (3, 2 and 8 steps).  The predicate offers every pass for each of them.

data = "int" (tests/exact_data.py): every stored element of logits, dx, dK and dbias EQUALS the restatement - fp32 sums of integers
below 2^24 are exact in any order, the folded kernel (sums of at most four integers) too, and bf16 outputs are the exact value rounded
to nearest even; the dlogits are shifted by 40 as test_kernels_gpu.HEAD_DLOGITS_SHIFT does, so that the bf16 data gradient rounds.  The
same outputs of the literal composition on the device (torch repeat_interleave, head6x6_fwd / head6x6_wgrad at the fine size, the
tap-table data gradient at the fine size in fp32 and a 2x2 sum - rounded once for bf16, as the kernel rounds once) have the same bits.
data = "uniform": the bounds of tests/test_kernels_gpu.py for the 6x6 head at the same C - forward 2e-6 sqrt(36 C) + 1e-6 (fp32) /
2e-5 (bf16 in), weight gradient 2e-6 sqrt(B H W) + 1e-6 over the fine grid, bf16 data gradient 1e-2, all relative to the largest
expected entry; the fp32 data gradient sums 2 * 49 products: 2e-6 sqrt(98) + 1e-6.  In bf16 storage the restatement convolves with the
folded kernel rounded to bf16 once (head_up2_ref.fold_bf16), which the fold kernel must reproduce bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import exact_data as X
import head_up2_ref as HR
from oracle import detrand

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(1, 1, 3), (2, 5, 7), (3, 16, 24), (1, 6, 160)]
CHANNELS = [24, 16, 64]
CASES = [(B, h, w, C, st) for (B, h, w) in SHAPES for C in CHANNELS for st in ("f32", "bf16")]
DLOGITS_SHIFT = 40
CANARY = 0xA5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    print("\nexact comparisons of this process so far:", X.STATS)


def close(actual, expected, tol, what):
    a, e = actual.detach().double().cpu(), expected.detach().double().cpu()
    assert a.shape == e.shape, (what, a.shape, e.shape)
    scale = float(e.abs().max()) + 1e-30
    err = float((a - e).abs().max())
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, bound {tol * scale:.3e}")
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def q16(t):
    return t.float().to(torch.bfloat16).double()


@functools.lru_cache(maxsize=None)
def reference(B, h, w, C, storage, data):
    """Inputs (fp64, already in the values the storage type holds) and the restatement's outputs; computed once per case."""
    tag = f"up2{B, h, w, C}"
    if data == "int":
        x, k, b = X.acts("x" + tag, (B, C, h, w)), X.kernels("k" + tag, (2, 6, 6, C)), X.biases("b" + tag, (2,))
        d = X.acts("d" + tag, (B, 2, 2 * h, 2 * w)) + DLOGITS_SHIFT
    else:
        u = lambda n, s: torch.tensor(detrand.uniform(n + tag, s, -1, 1, np.float64))
        x, k, b, d = u("x", (B, C, h, w)), u("k", (2, 6, 6, C)).float().double(), u("b", (2,)).float().double(), u("d", (B, 2, 2 * h, 2 * w))
        x, d = (q16(x), q16(d)) if storage == "bf16" else (x.float().double(), d.float().double())
    if storage == "bf16":
        kf = HR.fold_bf16(k)                               # the work copy of a bf16 trunk: fp32 sums rounded to bf16 once
        logits = HR.folded(x, kf, b)
        dx, _ = HR.folded_grads(x, kf, d)
        _, _, dk, db = HR.literal_grads(x, k, b, d)       # the weight gradient does not see the kernel
    else:
        kf = HR.fold(k.float(), torch.float32).double()
        logits, dx, dk, db = HR.literal_grads(x, k, b, d)
    if data == "int":
        assert torch.equal(logits, HR.literal(x, k, b)) and torch.equal(kf, HR.fold(k))
        gmax = 3 + DLOGITS_SHIFT
        X.check_exactness_conditions({"x": (x, storage == "bf16"), "k": (k, False), "folded k": (kf, storage == "bf16"), "bias": (b, False)},
                                     X.conv_abs_bound(16 * C, has_addend=False, w_max=4 * 2), what=f"{tag} fwd")
        X.check_exactness_conditions({"dlogits": (d, storage == "bf16")}, B * 4 * h * w * 3 * gmax, what=f"{tag} wgrad / dbias")
        ties = X.check_exactness_conditions({"dlogits": (d, storage == "bf16")}, 98 * 8 * gmax, dx if storage == "bf16" else None, what=f"{tag} dgrad")
    else:
        ties = 0
    return dict(x=x, k=k, b=b, d=d, kf=kf, logits=logits, dx=dx, dk=dk, db=db, ties=ties)


def embed(t_nchw, ld, c0, dt, fill):
    B, C, H, W = t_nchw.shape
    buf = torch.full((B, H, W, ld), fill, dtype=dt)
    buf[..., c0:c0 + C] = t_nchw.permute(0, 2, 3, 1).to(dt)
    return buf.to(DEV)


class Guarded:
    """A Workspace whose buffer is the first `adv` bytes of a larger allocation filled with a byte pattern."""

    def __init__(self, ops, adv):
        self.big = torch.full((int(adv) + (1 << 16),), CANARY, dtype=torch.uint8, device=DEV)
        self.ws = ops.Workspace(DEV)
        self.ws.buf = self.big[:int(adv)]
        self.adv = int(adv)

    def assert_intact(self, what):
        torch.cuda.synchronize()
        assert self.ws.buf.data_ptr() == self.big.data_ptr() and self.ws.nbytes == self.adv, f"{what}: the wrapper asked for more than the advertised size"
        assert int((self.big[self.adv:] != CANARY).sum()) == 0, f"{what}: bytes behind the advertised workspace size were overwritten"


def run_kernels(ops, r, B, h, w, C, storage):
    """One run of fold, forward, data gradient, weight gradient and bias gradient on poisoned buffers; the weight gradient with exactly
    its advertised workspace in front of a canary."""
    dt, PAD = (torch.float32, 4) if storage == "f32" else (torch.bfloat16, 8)
    xa = ops.Act(embed(r["x"], C + PAD, PAD, dt, 768.0), PAD, C)
    wm = torch.zeros((PAD, 6, 6, C), device=DEV); wm[:2] = r["k"].float().to(DEV)
    bm = torch.zeros(PAD, device=DEV); bm[:2] = r["b"].float().to(DEV)
    wf = torch.full((ops.head_up2_folded_elems(C) + 64,), 11.0, device=DEV)
    ops.head_up2_fold(wm, wf, C, storage == "bf16")
    ya = ops.Act(torch.full((B, 2 * h, 2 * w, 4), 5.0, device=DEV))
    ops.head_up2_fwd(xa, wf, bm, ya)
    dl = ops.Act(embed(r["d"], PAD, 0, dt, 0.0))
    dxa = ops.Act(torch.full((B, h, w, C + PAD), 3.0, dtype=dt, device=DEV), PAD, C)
    ops.head_up2_dgrad(dl, wf, dxa)
    dw = torch.full((PAD, 6, 6, C), 7.0, device=DEV)
    gd = Guarded(ops, ops.head_up2_wgrad_ws_bytes(B, h, w, C))
    ops.head_up2_wgrad(xa, dl, dw, gd.ws)
    gd.assert_intact(f"head_up2_wgrad {B, h, w, C, storage}")
    db = torch.full((PAD,), 9.0, device=DEV)
    ops.colsum(dl, db, ops.Workspace(DEV))
    torch.cuda.synchronize()
    return dict(xa=xa, wm=wm, bm=bm, wf=wf, ya=ya, dl=dl, dxa=dxa, dw=dw, db=db)


@X.parametrize_kinds("B,h,w,C,storage", CASES)
def test_head_up2_kernels(U, B, h, w, C, storage, data):
    ops = U.ops
    assert ops.head_up2_supported(C, storage) == 7
    r = reference(B, h, w, C, storage, data)
    exact = data == "int"
    PAD = 4 if storage == "f32" else 8
    tag = f"head_up2 {B, h, w, C, storage, data}"
    o = run_kernels(ops, r, B, h, w, C, storage)
    nf = ops.head_up2_folded_elems(C)
    # fold: bit for bit in both kinds (fp32 additions in the stated order; bf16: one rounding), nothing behind the copy touched
    X.assert_exact(o["wf"][:nf].view(8, 4, 4, C), r["kf"], tag + " fold")
    assert float(o["wf"][nf:].min()) == 11.0 and float(o["wf"][nf:].max()) == 11.0
    nchw = lambda a: a.permute(0, 3, 1, 2)
    if exact:
        X.note_ties(r["ties"])
        if storage == "bf16" and r["dx"].numel() >= 4096:
            assert r["ties"] > 0, "the integer data gradient has no bf16 tie: the rounding mode is not tested"
        X.assert_exact(nchw(o["ya"].dense()[..., :2]), r["logits"], tag + " logits")
        X.assert_exact(nchw(o["dxa"].dense()), X.expected_bf16(r["dx"]) if storage == "bf16" else r["dx"], tag + " dx")
        X.assert_exact(o["dw"][:2], r["dk"], tag + " dK")
        X.assert_exact(o["db"][:2], r["db"], tag + " dbias")
    else:
        Hf, Wf = 2 * h, 2 * w
        close(nchw(o["ya"].dense()[..., :2]), r["logits"], 2e-6 * math.sqrt(36 * C) + 1e-6 if storage == "f32" else 2e-5, tag + " logits")
        close(nchw(o["dxa"].dense()), r["dx"], 2e-6 * math.sqrt(98) + 1e-6 if storage == "f32" else 1e-2, tag + " dx")
        close(o["dw"][:2], r["dk"], 2e-6 * math.sqrt(B * Hf * Wf) + 1e-6, tag + " dK")
        close(o["db"][:2], r["db"], 2e-6 * math.sqrt(B * Hf * Wf) + 1e-6, tag + " dbias")
    # untouched columns and pad rows keep their fill value
    assert float(o["ya"].dense()[..., 2:].abs().max()) == 0.0                                  # channels 2, 3 of the logits: zeroed, as head6x6_fwd
    side = o["dxa"].base[..., :PAD].float()
    assert float(side.min()) == 3.0 and float(side.max()) == 3.0
    assert float(o["xa"].base[..., :PAD].float().min()) == 768.0
    assert float(o["dw"][2:].min()) == 7.0 and float(o["dw"][2:].max()) == 7.0
    # two runs give identical bits
    o2 = run_kernels(ops, r, B, h, w, C, storage)
    for n in ("wf", "dw"):
        assert torch.equal(o[n], o2[n]), f"{tag}: {n} differs between two runs"
    for n in ("ya", "dxa"):
        assert torch.equal(o[n].base, o2[n].base), f"{tag}: {n} differs between two runs"
    if exact:
        _twin(ops, r, o, B, h, w, C, storage, tag)


def _twin(ops, r, o, B, h, w, C, storage, tag):
    """The literal composition on the device: the up-sampled tensor materialised, the existing 6x6 head kernels at the fine size."""
    dt, PAD = (torch.float32, 4) if storage == "f32" else (torch.bfloat16, 8)
    xup = ops.Act(o["xa"].dense().repeat_interleave(2, dim=1).repeat_interleave(2, dim=2).contiguous())
    ya = ops.Act(torch.full((B, 2 * h, 2 * w, 4), 5.0, device=DEV))
    ops.head6x6_fwd(xup, o["wm"], o["bm"], ya)
    dw = torch.zeros((PAD, 6, 6, C), device=DEV)
    ops.head6x6_wgrad(xup, o["dl"], dw, ops.Workspace(DEV))
    # data gradient of the 6x6 head at the fine size on the tap-table kernel in fp32, then the 2x2 sum (the adjoint of the up-sampling)
    d32 = ops.Act(torch.zeros((B, 2 * h, 2 * w, 4), device=DEV))
    d32.base[..., :2] = o["dl"].dense()[..., :2].float()
    w4 = torch.zeros((4, 6, 6, C), device=DEV); w4[:2] = o["wm"][:2]
    wt = w4.permute(3, 1, 2, 0).contiguous()
    dxf = ops.Act(torch.zeros((B, 2 * h, 2 * w, C), device=DEV))
    ops.conv2d_dgrad(ops.geom(B, 2 * h, 2 * w, C, 4, 6, 1), d32, wt, dxf)
    torch.cuda.synchronize()
    dx = dxf.base.view(B, h, 2, w, 2, C).sum((2, 4))
    assert torch.equal(ya.base, o["ya"].base), tag + ": logits differ from the literal twin"
    assert torch.equal(dw[:2], o["dw"][:2]), tag + ": dK differs from the literal twin"
    assert torch.equal(dx.to(dt), o["dxa"].dense()), tag + ": dx differs from the literal twin"
