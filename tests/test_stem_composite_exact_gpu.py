"""The stem's composite gradient on the device (csrc/stem_composite.hip: head_wgrad_mfma_kernel<5, true>, stem_frame_kernel,
stem_finalize_kernel, stem_contract_kernel) against the two-layer chain in fp64 (tests/stem_composite_ref.py: chain), element by
element with == on the integer data of tests/exact_data.py.

No tolerance: the fp32 partials of the correlation and of the frame sums are sums of integer products of magnitude at most 9 over at
most B H W pixels, exact in any order below 2^24; the fp64 reduction and contraction are exact; the result is below 2^24 (2^23
with reg = 0.5, where it is a multiple of 0.5).  tests/test_stem_composite.py asserts these conditions, and that the chain equals
the S, T, E, F formulas, for every shape used here, on the CPU.  What the device returns is therefore determined: one wrong, missing
or doubled term, a stale ring slot, a partial left out of a strided sum or a value carried through something narrower than fp32 is a
mismatch.

Shapes: stem_composite_ref.EXACT_SHAPES, each with what it reaches - one-pixel and one-line images, one exact tile, ragged second
tiles, three row and three column blocks, the widest admitted image, column lines past one 256-pixel chunk, exactly 512 correlation
blocks and 561 of them (49 workgroups walk a second block), 33 partials for the 16-class strided sums.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exact_data as X  # noqa: E402
import stem_composite_ref as SC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LDG, C0G = 96, 16                     # G lives in channels [16, 80) of a NaN-filled 96-channel buffer
FILL, GUARD = 7.0, 64                 # what the outputs hold before the call; elements behind dW0 that must keep it
PAST_THE_CAP = (33, 272, 2)


@pytest.fixture(scope="module", autouse=True)
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    print("\nexact comparisons of this process so far:", X.STATS)


class _Dev:
    """One shape's inputs on the device.  ldx = 8: x in a zeroed 8-channel buffer; ldx = 2: x alone, no padding channels."""

    def __init__(self, shape, ldx=8):
        from unet_rir_amd import ops
        B, H, W = shape
        c = SC.exact_case(B, H, W)
        t = lambda a: torch.tensor(a)
        self.shape, self.ldx, self.case = shape, ldx, c
        self.x = torch.zeros((B, H, W, ldx), dtype=torch.bfloat16, device=DEV)
        self.x[..., :2] = t(c["x"]).to(torch.bfloat16).to(DEV)
        self.g = ops.Act(torch.full((B, H, W, LDG), float("nan"), dtype=torch.bfloat16, device=DEV), C0G, 64)
        self.g.base[..., C0G:C0G + 64] = t(c["g"]).to(torch.bfloat16).to(DEV)
        self.w1t = t(c["w1"]).permute(3, 1, 2, 0).contiguous().to(torch.bfloat16).to(DEV)       # [co0][t1][co1]
        self.w0 = t(c["w0"])                                                                    # fp64 [64,3,3,8], on the host

    def want(self, ldw=8, reg=0.0):
        """dW0 [64,3,3,ldw] and db0 [64] in fp64: the chain in channels 0 and 1, zero behind them, + reg * w0 in all of them."""
        dw = torch.zeros((64, 3, 3, ldw), dtype=torch.float64)
        dw[..., :2] = torch.tensor(self.case["dw0"])
        return dw + reg * self.w0[..., :ldw], torch.tensor(self.case["db0"])

    def run(self, ldw=8, reg=0.0, ws=None):
        """One call.  Returns dW0 [64,3,3,ldw], db0 [64] and the guard elements behind dW0, on the host."""
        from unet_rir_amd import _lib, ops
        B, H, W = self.shape
        n = 64 * 9 * ldw
        buf = torch.full((n + GUARD,), FILL, device=DEV)
        dw, db = buf[:n].view(64, 3, 3, ldw), torch.full((64,), FILL, device=DEV)
        w0d = self.w0[..., :ldw].contiguous().float().to(DEV)
        ws = ops.Workspace(DEV) if ws is None else ws
        if self.ldx % 8 == 0:
            ops.stem_composite(self.g, ops.Act(self.x), self.w1t, dw, db, ws, reg=reg, w0=w0d)
        else:                             # an Act has 16-byte pixels at least: the C entry point itself
            ws.reserve(ops.stem_composite_ws_bytes(B))
            p = ops._p
            ops.check(_lib.lib().unetrir_stem_composite_bf16(p(self.g), LDG, p(self.x), self.ldx, B, H, W, p(self.w1t), reg,
                                                             p(w0d) if reg else None, p(dw), ldw, p(db), ws.ptr, ws.nbytes, ops._stream()),
                      "stem_composite")
        torch.cuda.synchronize()
        return dw.cpu(), db.cpu(), buf[n:].cpu()

    def poison_intact(self):
        b = self.g.base
        return bool(torch.isnan(b[..., :C0G].float()).all()) and bool(torch.isnan(b[..., C0G + 64:].float()).all())


def _assert_exact(dev, got, ldw=8, reg=0.0, what=""):
    dw, db, guard = got
    want_w, want_b = dev.want(ldw, reg)
    tag = f"stem composite {dev.shape} ldx={dev.ldx} ldw={ldw} reg={reg} {what}"
    X.assert_exact(dw, want_w, tag + " dW0")
    X.assert_exact(db, want_b, tag + " db0")
    assert bool((guard == FILL).all()), tag + ": written behind dW0"


@pytest.mark.parametrize("B,H,W", SC.EXACT_SHAPES)
def test_exact_at_every_shape(B, H, W):
    dev = _Dev((B, H, W))
    got = dev.run()
    _assert_exact(dev, got)
    assert bool((got[0][..., 2:] == 0).all())                 # the padding channels of the 2-channel end
    assert dev.poison_intact()


@pytest.mark.parametrize("B,H,W", SC.REG_SHAPES)
def test_exact_with_weight_decay(B, H, W):
    dev = _Dev((B, H, W))
    plain, reg = dev.run(), dev.run(reg=X.REG)
    _assert_exact(dev, plain)
    _assert_exact(dev, reg, reg=X.REG)
    assert bool((dev.w0[..., 2:] != 0).all())
    X.assert_exact(reg[0][..., 2:], X.REG * dev.w0[..., 2:], "padding channels: reg * w0 as given")
    assert torch.equal(reg[1], plain[1])                      # the bias gradient has no such term


@pytest.mark.parametrize("ldx", [2, 8])
@pytest.mark.parametrize("ldw", [2, 3, 8])
def test_exact_at_other_strides(ldx, ldw):
    """ldw = 2: the contraction's loop over padding channels has no trip; ldw = 3: one channel per tap.  With and without the
    weight-decay term, which is what those channels hold."""
    dev = _Dev((3, 17, 257), ldx)
    assert tuple(dev.x.shape) == (3, 17, 257, ldx)
    _assert_exact(dev, dev.run(ldw=ldw), ldw)
    _assert_exact(dev, dev.run(ldw=ldw, reg=X.REG), ldw, X.REG)
    assert dev.poison_intact()


def test_workspace_contents_do_not_matter():
    """One workspace, every byte 0xFF (NaN as fp32 and as fp64), never refilled: the largest shape first, so that the smaller calls
    behind it find its partials beyond their own nblk and B; the rows of the unused sixth vertical tap are never written at all."""
    from unet_rir_amd import ops
    ws = ops.Workspace(DEV, ops.stem_composite_ws_bytes(33))
    ws.buf.fill_(0xFF)
    ptr = ws.buf.data_ptr()
    for shape in (PAST_THE_CAP, (1, 1, 1), (3, 17, 257)):
        dev = _Dev(shape)
        used, fresh = dev.run(ws=ws), dev.run()
        _assert_exact(dev, used, what="on a used workspace")
        _assert_exact(dev, fresh, what="on a fresh workspace")
        assert torch.equal(used[0], fresh[0]) and torch.equal(used[1], fresh[1])
    assert ws.buf.data_ptr() == ptr                           # the same buffer throughout: no call made it grow


def test_twice_bit_equal_past_the_cap():
    dev = _Dev(PAST_THE_CAP)
    a, b = dev.run(), dev.run()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _assert_exact(dev, a)
