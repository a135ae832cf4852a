"""The five `linear` entry points (csrc/elementwise.hip with ACT = 2; dl_models/diff_u_net.py:247, diff_vae.py:385) on the GPU by the
criterion of test_aenet_gpu.test_relu1_kernels_element_by_element: every element against an fp64 reference with a bound of its own
(tests/streaming_check.py).  Logits lie in [-1.5, 1.5], so the phase wrap is crossed in both directions; a handful are 0, -0, +/-1 and
a large value.  No element is left out of a comparison."""
import math

import pytest
import torch

import streaming_check as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D64 = torch.float64
TWO_PI_F = float(torch.tensor(6.283185307179586, dtype=torch.float32))
PI_F = float(torch.tensor(3.141592653589793, dtype=torch.float32))
LARGE = 37.5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def linear_loss_ref(z, target, alpha, inv_norm, phase_ref=None, phase_w=None):
    """fp64 reference and per-element bounds of the loss kernel with the linear output, for logits z [B, H, W, 2] (fp32 values) and
    target [B, 2, H, W]:
      pred     p = z: a copy - DETERMINED, bit for bit
      dlogits  g0 = -2.f da alpha inv, da = t0 - p0: one rounding in da, the product with 2 exact, two more products -> 2;
               g1 = -(1.f - alpha) inv 2pi sinf(ph) w: four products -> 4, sinf within 1 ulp (2 * 2^-24), the phase argument's error:
               every fp32 operation 2^-24 of its result, the wrap's |2pi_f - 2pi| per turn (|d| / 2pi + 1 turns: the large logit)
      sums     fp64 accumulation in a fixed order of fp32 addends, then the final conversions."""
    a32 = float(torch.tensor(alpha, dtype=torch.float32)); inv32 = float(torch.tensor(inv_norm, dtype=torch.float32))
    oma32 = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(alpha, dtype=torch.float32))
    W_ = target.shape[3]
    zz = z.double()
    p0, p1 = zz[..., 0], zz[..., 1]
    t0, t1 = target[:, 0].double(), target[:, 1].double()
    e_t1 = torch.zeros_like(t1)
    if phase_ref is not None:
        t1 = t1 - phase_ref[:, 1].double(); e_t1 = S.U32 * t1.abs()
    w = torch.ones_like(t1) if phase_w is None else phase_w.double().view(1, 1, W_).expand_as(t1)
    da = t0 - p0
    e_da = S.U32 * da.abs()
    e_sq = 2 * da.abs() * e_da + S.U32 * da * da
    a1, a2 = t1 * TWO_PI_F, p1 * TWO_PI_F
    yt, yp = a1 - PI_F, a2 - PI_F
    d1 = yt - yp
    dd = d1 + PI_F
    turns = (dd / TWO_PI_F).floor().abs() + 1
    # d / 2pi_f (a division: 1 rounding of a quotient of size turns), floorf, the product with 2pi_f, the two differences
    e_ph = (S.U32 * (a1.abs() + yt.abs() + a2.abs() + yp.abs() + d1.abs() + 3 * dd.abs() + 2 * turns * TWO_PI_F + PI_F) + TWO_PI_F * e_t1
            + turns * abs(TWO_PI_F - 2 * math.pi))
    ph = torch.remainder(dd, TWO_PI_F) - PI_F
    eph = 1 - torch.cos(ph)
    e_eph = e_ph + 2 * S.U32 * torch.cos(ph).abs() + S.U32 * eph.abs()
    e_ephw = w * e_eph + S.U32 * (eph * w).abs()
    N = da.numel()
    sa, sp, spw = (da * da).sum(), eph.sum(), (eph * w).sum()
    d_sa = S.U32 * sa + e_sq.sum() + N * S.U64 * sa
    d_sp = S.U32 * sp + e_eph.sum() + N * S.U64 * sp
    e_spw = e_ephw.sum() + N * S.U64 * spw
    out0 = (a32 * sa + (1 - a32) * spw) * inv32
    d_out0 = S.U32 * abs(out0) + inv32 * (a32 * (e_sq.sum() + N * S.U64 * sa) + (1 - a32) * e_spw)
    c0 = -2 * a32 * inv32
    g0 = c0 * da
    d_g0 = abs(c0) * e_da + 2 * S.U32 * g0.abs()
    c1 = -oma32 * inv32 * TWO_PI_F
    sn = torch.sin(ph)
    g1 = c1 * sn * w
    d_g1 = abs(c1) * w * (e_ph + 2 * S.U32 * sn.abs()) + 4 * S.U32 * g1.abs()
    # an argument within its error of the wrap point may land on either side of it: sin is continuous there (sin(-pi) = sin(pi) = 0)
    # and so is 1 - cos, so the bounds above hold across the wrap
    return dict(v0=g0, d_v0=d_g0, v1=g1, d_v1=d_g1, sums=torch.stack([out0, sa, sp]), d_sums=torch.stack([d_out0, d_sa, d_sp]))


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", ["plain", "phase_ref", "phase_weight", "both"])
@pytest.mark.parametrize("Bq,Hq,Wq,ldl", [(1, 1, 1, 4), (1, 33, 17, 8), (2, 144, 160, 4)])
def test_linear_kernels_element_by_element(U, Bq, Hq, Wq, ldl, mode, dt):
    ops = U.ops
    g = torch.Generator(device=DEV); g.manual_seed(Bq * Hq + Wq + len(mode))
    ur = lambda shape, lo, hi: torch.rand(shape, device=DEV, generator=g) * (hi - lo) + lo
    alpha, inv_norm = 0.9, 1.0 / (2 * Hq * Wq * Bq)
    z = ur((Bq, Hq, Wq, 2), -1.5, 1.5)
    edges = torch.tensor([0.0, -0.0, 1.0, -1.0, LARGE, -LARGE, 1e-45, 0.5], device=DEV)
    pick = torch.randint(0, 64, (Bq, Hq, Wq, 2), device=DEV, generator=g)
    z = torch.where(pick < 8, edges[pick % 8], z)
    if Bq * Hq * Wq == 1:
        z[0, 0, 0, 0], z[0, 0, 0, 1] = -0.0, -1.25            # the single pixel: a negative zero and a negative phase
    target = ur((Bq, 2, Hq, Wq), 0, 1)
    pref = ur((Bq, 2, Hq, Wq), 0, 1) if mode in ("phase_ref", "both") else None
    pw = ur((Wq,), 0, 1) if mode in ("phase_weight", "both") else None
    logits = ops.Act(torch.full((Bq, Hq, Wq, ldl), 777.0, device=DEV), 0, ldl)
    logits.base[..., :2] = z
    ldd = 4 if dt == torch.float32 else 8
    dl = ops.Act(torch.full((Bq, Hq, Wq, ldd), 9.0, dtype=dt, device=DEV))
    pr = torch.full((Bq, 2, Hq, Wq), -7.0, device=DEV)
    out = torch.full((4,), -1.0, device=DEV)
    ws = ops.Workspace(DEV)
    ops.linear_loss(logits, target, alpha, inv_norm, pr, dl, out, ws, phase_ref=pref, phase_weight=pw)
    torch.cuda.synchronize()
    r = linear_loss_ref(z, target, alpha, inv_norm, pref, pw)
    tag = f"{(Bq, Hq, Wq)} {mode}"
    assert torch.equal(_bits(pr), _bits(z.permute(0, 3, 1, 2))), f"pred is the logit bit for bit {tag}"
    if Bq * Hq * Wq > 1:
        assert float(pr.min()) < -1.0 and float(pr.max()) > 1.0                       # neither bounded output could give these
    S.check(dl.base[..., :2], torch.stack([r["v0"], r["v1"]], -1), torch.stack([r["d_v0"], r["d_v1"]], -1), f"dlogits {tag}", "linear_loss dlogits")
    assert float(dl.base[..., 2:].float().abs().max()) == 0.0, "channels 2 ... of dlogits are exact zeros"
    S.check(out[:3], r["sums"], r["d_sums"], f"loss, amplitude sum, phase sum {tag}", "linear_loss sums")
    assert bool(torch.isfinite(out[:3]).all()) and float(out[3]) == -1.0
    assert bool((logits.base[..., 2:] == 777.0).all())
    pr2 = torch.full_like(pr, -7.0)
    ops.linear_nchw(logits, pr2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(pr), _bits(pr2))
    # the bridge: dL/dlogit = dL/dpred, no arithmetic - unchanged in fp32, its rounding in bf16 (S.check with d = 0 decides every element)
    dpred = ur((Bq, 2, Hq, Wq), -1, 1)
    dl2 = ops.Act(torch.full((Bq, Hq, Wq, ldd), 9.0, dtype=dt, device=DEV))
    ops.linear_bwd(pr, dpred, dl2)
    torch.cuda.synchronize()
    if dt == torch.float32:
        assert torch.equal(_bits(dl2.base[..., :2]), _bits(dpred.permute(0, 2, 3, 1)))
    S.check(dl2.base[..., :2], dpred.double().permute(0, 2, 3, 1), 0.0, f"linear_bwd {tag}", "linear_bwd")
    assert float(dl2.base[..., 2:].float().abs().max()) == 0.0
    # a second run gives the same bits: the sums are accumulated in a fixed order
    out2 = torch.full((4,), -1.0, device=DEV)
    ops.linear_loss(logits, target, alpha, inv_norm, pr2, dl2, out2, ws, phase_ref=pref, phase_weight=pw)
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and torch.equal(dl.base, dl2.base)
