"""The stem's composite gradient on the device (csrc/stem_composite.hip through the C ABI) against the fp64 formulas
(tests/stem_composite_ref.py) on the same bf16 inputs, and against the path it replaces: the 64 -> 64 data gradient, rounded to bf16,
then the stem's weight gradient and a column sum.

Tolerance: none of its own.  Both paths are measured against the fp64 reference (relative L2 per tensor); the composite path, which
never rounds the tensor between the two layers to bf16, must be no worse than 1.25 x the replaced path's error - the margin covers
summation-order scatter only.  That is the statement about real-valued data against the replaced path; the per-element guarantee
(every term, at the shapes where the kernels' loops take further trips) is tests/test_stem_composite_exact_gpu.py, which compares
with == on integer data.

Shapes: the kernel's minimum is a 1 x 1 image; its correlation tile is 16 rows x 256 columns, so 17 x 300 is a non-square image of
two (ragged) tiles per side; 3 x 5 has nothing but border pixels and adjacent corners.
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stem_composite_ref as SC  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL = 10001
SHAPES = [(1, 1), (3, 5), (17, 300)]
LDG, C0G = 96, 16                     # G lives in channels [16, 80) of a poisoned 96-channel buffer


def _inputs(H, W, seed, frame_scale=1.0, B=2):
    from unet_rir_amd import ops
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, H, W, 2), generator=gen).to(torch.bfloat16)
    g = torch.randn((B, H, W, 64), generator=gen)
    if frame_scale != 1.0:
        g[:, 0] *= frame_scale; g[:, -1] *= frame_scale
        g[:, 1:-1, 0] *= frame_scale; g[:, 1:-1, -1] *= frame_scale
    g = (g * 1e-3).to(torch.bfloat16)
    w1 = (torch.randn((64, 3, 3, 64), generator=gen) / 24.0).to(torch.bfloat16)         # [co1][t1][co0], as the bf16 work copy holds it
    w0 = torch.zeros((64, 3, 3, 8))
    w0[..., :2] = torch.randn((64, 3, 3, 2), generator=gen)
    xa = ops.Act(torch.zeros((B, H, W, 8), dtype=torch.bfloat16, device=DEV))
    xa.base[..., :2] = x.to(DEV)
    ga = ops.Act(torch.full((B, H, W, LDG), float("nan"), dtype=torch.bfloat16, device=DEV), C0G, 64)
    ga.base[..., C0G:C0G + 64] = g.to(DEV)
    w1t = w1.permute(3, 1, 2, 0).contiguous().to(DEV)                                    # [co0][t1][co1]
    return x, g, w1, w0, xa, ga, w1t, w0.to(DEV)


def _composite(xa, ga, w1t, w0d, reg):
    from unet_rir_amd import ops
    dw = torch.full((64, 3, 3, 8), 7.0, device=DEV)
    db = torch.full((64,), 7.0, device=DEV)
    ops.stem_composite(ga, xa, w1t, dw, db, ops.Workspace(DEV), reg=reg, w0=w0d)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def _replaced_path(xa, ga, w1t, w0d, reg):
    from unet_rir_amd import ops
    B, H, W = ga.B, ga.H, ga.W
    gd = ops.new_act(B, H, W, 64, DEV, dtype=torch.bfloat16)
    ops.conv2d_dgrad(ops.geom(B, H, W, 64, 64, 3, 1), ga, w1t, gd)
    dw = torch.full((64, 3, 3, 8), 7.0, device=DEV)
    db = torch.full((64,), 7.0, device=DEV)
    ws = ops.Workspace(DEV)
    ops.conv2d_wgrad(ops.geom(B, H, W, 8, 64, 3, 1), xa, gd, dw, ws, reg=reg, w=w0d if reg else None)
    ops.colsum(gd, db, ws)
    torch.cuda.synchronize()
    return dw.cpu(), db.cpu()


def _rel(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def _check(H, W, seed, frame_scale, reg, tag):
    x, g, w1, w0, xa, ga, w1t, w0d = _inputs(H, W, seed, frame_scale)
    want_w, want_b = SC.stem_composite(x.double().numpy(), g.double().numpy(), w1.double().numpy(), reg, w0[..., :2].double().numpy())
    new_w, new_b = _composite(xa, ga, w1t, w0d, reg)
    old_w, old_b = _replaced_path(xa, ga, w1t, w0d, reg)
    e_new = (_rel(new_w[..., :2], want_w), _rel(new_b, want_b))
    e_old = (_rel(old_w[..., :2], want_w), _rel(old_b, want_b))
    print(f"stem_composite {tag} {H}x{W} reg={reg}: rel L2 dW0 new {e_new[0]:.3e} replaced {e_old[0]:.3e}; "
          f"db0 new {e_new[1]:.3e} replaced {e_old[1]:.3e}")
    assert e_new[0] <= 1.25 * e_old[0], (tag, "dW0", e_new[0], e_old[0])
    assert e_new[1] <= 1.25 * e_old[1], (tag, "db0", e_new[1], e_old[1])
    assert float(new_w[..., 2:].abs().max()) == 0.0               # the padding channels of the 2-channel end
    assert bool(torch.isfinite(new_w).all()) and bool(torch.isfinite(new_b).all())
    return new_w, new_b


@pytest.mark.parametrize("H,W", SHAPES)
def test_composite_against_fp64_and_the_replaced_path(H, W):
    _check(H, W, 1000 + H, 1.0, 0.0, "random")


@pytest.mark.parametrize("H,W", SHAPES[1:])
def test_frame_scaled_100x_so_a_wrong_border_term_cannot_hide(H, W):
    _check(H, W, 2000 + H, 100.0, 0.0, "frame x100")


def test_weight_decay_term_and_bit_reproducibility():
    H, W = SHAPES[2]
    x, g, w1, w0, xa, ga, w1t, w0d = _inputs(H, W, 3000)
    reg = 0.05
    w_reg, b_reg = _check(H, W, 3000, 1.0, reg, "reg")
    w_0, b_0 = _composite(xa, ga, w1t, w0d, 0.0)
    # fp32 on the result: (float)sum + reg * w, to one rounding of each term (the compiler may fuse the two operations)
    term = torch.tensor(reg, dtype=torch.float32) * w0
    assert bool(((w_reg - (w_0 + term)).abs() <= 2.0 ** -23 * (w_0.abs() + term.abs())).all())
    assert float(term.abs().max()) > 1e-2 * float(w_0.abs().max())      # the term is not lost in the gradient's own rounding
    assert torch.equal(b_reg, b_0)
    w_again, b_again = _composite(xa, ga, w1t, w0d, reg)
    assert torch.equal(w_again, w_reg) and torch.equal(b_again, b_reg)
    assert bool(torch.isnan(ga.base[..., :C0G].float()).all()) and bool(torch.isnan(ga.base[..., C0G + 64:].float()).all())


def test_rejected_arguments():
    from unet_rir_amd import _lib, ops
    L = _lib.lib()
    H, W = 3, 5
    x, g, w1, w0, xa, ga, w1t, w0d = _inputs(H, W, 4000)
    dw, db = torch.zeros((64, 3, 3, 8), device=DEV), torch.zeros(64, device=DEV)
    ws = ops.Workspace(DEV, ops.stem_composite_ws_bytes(2))
    p = lambda t: C.c_void_p(t.ptr if isinstance(t, ops.Act) else t.data_ptr())

    def call(g_=p(ga), ldg=LDG, x_=p(xa), ldx=8, B=2, H_=H, W_=W, w1_=p(w1t), reg=0.0, w0_=None, dw_=p(dw), ldw=8, db_=p(db), ws_=ws.ptr,
             nb=ws.nbytes):
        return L.unetrir_stem_composite_bf16(g_, ldg, x_, ldx, B, H_, W_, w1_, reg, w0_, dw_, ldw, db_, ws_, nb, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert call(g_=None) == EINVAL and call(x_=None) == EINVAL and call(w1_=None) == EINVAL
    assert call(dw_=None) == EINVAL and call(db_=None) == EINVAL and call(ws_=None) == EINVAL
    assert call(ldg=60) == EINVAL and call(ldg=68) == EINVAL          # fewer than 64 channels; not a multiple of 8
    assert call(ldx=1) == EINVAL and call(ldx=3) == EINVAL
    assert call(ldw=1) == EINVAL
    assert call(B=0) == EINVAL and call(H_=0) == EINVAL and call(W_=0) == EINVAL and call(W_=4097) == EINVAL
    assert call(reg=1e-3, w0_=None) == EINVAL                         # a weight-decay term without the weights
    assert call(nb=ops.stem_composite_ws_bytes(2) - 1) == EINVAL
    assert call(g_=C.c_void_p(ga.ptr + 2)) == EINVAL                  # G rows start on 16-byte boundaries
    assert L.unetrir_stem_composite_supported(2, 32, 32, 64, 64) == 1
    assert L.unetrir_stem_composite_supported(2, 32, 32, 32, 32) == 0 and L.unetrir_stem_composite_supported(2, 32, 32, 64, 128) == 0
    torch.cuda.synchronize()


def test_three_trainer_steps_with_the_composite_path_on_and_off():
    """B = 2, 32 x 32, F0 = 64.  After the first backward every gradient tensor but the stem's two is bit-equal (nothing else reads
    what the composite path replaces); the loss sequences of three optimizer steps agree to the bf16 storage noise recorded for this
    engine: entry "pred" / "rms" of profiles/r04_bf16_noise_trace.json (rms deviation of the bf16 engine's prediction from the fp32
    engine's, 3.4e-3), taken relative to the loss."""
    import unet_rir_amd as U
    bound = json.load(open(os.path.join(ROOT, "profiles", "r04_bf16_noise_trace.json")))["pred"]["rms"]
    B, H, W = 2, 32, 32
    gen = torch.Generator().manual_seed(5)
    spec_in = torch.rand((B, 2, H, W), generator=gen).to(DEV)
    spec_out = torch.rand((B, 2, H, W), generator=gen).to(DEV)
    emb = torch.randint(0, 2000, (B, 2, 16), generator=gen).to(DEV)
    engs, trs = {}, {}
    for on in (True, False):
        eng = U.UNetEngine(H, W, B, F0=64, k=3, device=DEV, dtype="bf16")
        assert eng.stem_composite is True and eng.stem_composite_supported and eng.g_down[1] is None
        eng.stem_composite = on
        eng.reset_parameters(torch.Generator().manual_seed(0))
        engs[on], trs[on] = eng, U.Trainer(eng, lr=1e-4, dropout=False)
    for on, eng in engs.items():
        eng.forward(spec_in, emb, target=spec_out, global_batch=B)
        eng.backward()
    torch.cuda.synchronize()
    assert engs[True].g_down[1] is None and engs[False].g_down[1] is not None
    stem = ("enc1.down.kernel", "enc1.down.bias")
    for n in engs[True].specs:
        a, b = engs[True].g[n], engs[False].g[n]
        if n in stem:
            print(f"{n}: composite vs replaced path rel L2 {_rel(a.cpu(), b.cpu()):.3e}")
            assert bool(torch.isfinite(a).all())
        else:
            assert torch.equal(a, b), n
    losses = {on: [trs[on].step(spec_in, emb, spec_out, return_loss=True) for _ in range(3)] for on in (True, False)}
    print("losses on ", losses[True], "\nlosses off", losses[False])
    assert losses[True][0] == losses[False][0]                        # the first forward pass is the same computation
    for a, b in zip(losses[True], losses[False]):
        assert abs(a - b) <= bound * abs(b), (a, b, bound)
