"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for what AENet adds to ``unet_rir_amd.ops``: the 2x2 stride-2 entry
points (csrc/conv2x2.hip; the same arithmetic as the generic stand-ins, which are generic in k, under their own names in the
simulated runtime's log) and the clipped-ReLU output kernels.  ``install(monkeypatch, runtime, passes)``: `passes` is what
conv2x2s2_supported answers for a bf16 layer (default: all three), so the product's `_conv2x2` node takes its new branches."""
import math

import torch

import cpu_ops
from cpu_ops import D


class AENetCpuOps:
    C22_FWD, C22_DGRAD, C22_WGRAD = 1, 2, 4

    def __init__(self, rt, base, passes):
        self.rt, self.base, self.passes = rt, base, passes
        self.calls = {}

    def _count(self, what):
        self.calls[what] = self.calls.get(what, 0) + 1

    def conv2x2s2_supported(self, g, x, y, transpose=False):
        ok = g.k == 2 and g.stride == 2 and x.sfx == "bf16" and y.sfx == "bf16" and (transpose or (g.H % 2 == 0 and g.W % 2 == 0))
        return self.passes if ok else 0

    def conv2x2s2_fwd(self, g, x, w, bias, y, addend=None):
        self._count("fwd"); self.base.conv2d_fwd(g, x, w, bias, y, addend)

    def conv2x2s2_dgrad(self, g, dy, wt, dx, addend=None):
        self._count("dgrad"); self.base.conv2d_dgrad(g, dy, wt, dx, addend)

    def conv2x2s2_wgrad(self, g, x, dy, dw, ws, reg=0.0, w=None, defer=None):
        self._count("wgrad"); self.base.conv2d_wgrad(g, x, dy, dw, ws, reg, w, defer)

    def conv2x2s2_transpose_fwd(self, g, x, wt, bias, y):
        self._count("tfwd"); self.base.conv2d_transpose_fwd(g, x, wt, bias, y)

    def conv2x2s2_transpose_dgrad(self, g, dy, w, dx, addend=None):
        self._count("tdgrad"); self.base.conv2d_transpose_dgrad(g, dy, w, dx, addend)

    def conv2x2s2_transpose_wgrad(self, g, x, dy, dw, ws, reg=0.0, w=None, defer=None):
        self._count("twgrad"); self.base.conv2d_transpose_wgrad(g, x, dy, dw, ws, reg, w, defer)

    def relu1_loss(self, logits, target, alpha, inv_norm, pred, dlogits, loss_out, ws, phase_ref=None, phase_weight=None):
        self.rt.touch([logits, target, phase_ref, phase_weight], [pred, dlogits, loss_out, ws], "relu1_loss")
        z = logits.base[..., :2].to(D).permute(0, 3, 1, 2)
        p = torch.clamp(z, 0.0, 1.0).clone().requires_grad_(True)
        t = target.to(D)
        e_amp = (t[:, 0] - p[:, 0]) ** 2
        t1 = t[:, 1] if phase_ref is None else t[:, 1] - phase_ref.to(D)[:, 1]
        ph = torch.remainder((t1 - p[:, 1]) * 2 * math.pi + math.pi, 2 * math.pi) - math.pi
        e_ph = 1.0 - torch.cos(ph)
        e_w = e_ph if phase_weight is None else e_ph * phase_weight.to(D).view(1, 1, -1)
        loss = (alpha * e_amp + (1 - alpha) * e_w).sum() * inv_norm
        (gp,) = torch.autograd.grad(loss, p)
        gz = gp * ((z > 0) & (z < 1))                      # dL/dlogit = dL/dpred where 0 < logit < 1, else 0
        pred.copy_(p.detach().float())
        dlogits.base.zero_()
        dlogits.base[..., :2] = gz.permute(0, 2, 3, 1).to(dlogits.base.dtype)
        loss_out[0] = float(loss.detach()); loss_out[1] = float(e_amp.detach().sum()); loss_out[2] = float(e_ph.detach().sum())

    def relu1_nchw(self, logits, pred):
        self.rt.touch([logits], [pred], "relu1_nchw")
        pred.copy_(torch.clamp(logits.base[..., :2].to(D), 0.0, 1.0).permute(0, 3, 1, 2).float())

    def relu1_bwd(self, pred, dpred, dlogits):
        self.rt.touch([pred, dpred], [dlogits], "relu1_bwd")
        p = pred.to(D)
        dlogits.base.zero_()
        dlogits.base[..., :2] = (dpred.to(D) * ((p > 0) & (p < 1))).permute(0, 2, 3, 1).to(dlogits.base.dtype)


def install(monkeypatch, rt, passes=7):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    a = AENetCpuOps(rt, impl, passes)
    for name in dir(a):
        if not name.startswith("_") and name not in ("rt", "base", "passes", "calls", "C22_FWD", "C22_DGRAD", "C22_WGRAD"):
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(a, name)))
    impl.aenet = a
    return impl
