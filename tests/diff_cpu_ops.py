"""Test infrastructure: fp64 stand-ins for what DiffUNet / DiffVAE add to ``unet_rir_amd.ops`` - the linear output kernels and the 1x1
head (csrc/head1x1.hip) - installed over tests/aenet_cpu_ops.py (DiffUNet: the 2x2 stride-2 layers) or tests/vae_cpu_ops.py (DiffVAE:
the sampling / KL kernels).  ``install(monkeypatch, runtime, family, head_passes, c22_passes)``: `head_passes` is what head1x1_supported
answers (default: both passes), so the product's `_head1x1` node takes its new branches."""
import math

import torch

import cpu_ops
from cpu_ops import D, _flat2, _put2


class DiffCpuOps:
    H1_FWD, H1_BWD = 1, 2

    def __init__(self, rt, head_passes):
        self.rt, self.head_passes = rt, head_passes
        self.calls = {}

    def _count(self, what):
        self.calls[what] = self.calls.get(what, 0) + 1

    # ---- the linear output (dl_models/diff_u_net.py:247, diff_vae.py:385)
    def linear_loss(self, logits, target, alpha, inv_norm, pred, dlogits, loss_out, ws, phase_ref=None, phase_weight=None):
        self.rt.touch([logits, target, phase_ref, phase_weight], [pred, dlogits, loss_out, ws], "linear_loss")
        p = logits.base[..., :2].to(D).permute(0, 3, 1, 2).clone().requires_grad_(True)
        t = target.to(D)
        e_amp = (t[:, 0] - p[:, 0]) ** 2
        t1 = t[:, 1] if phase_ref is None else t[:, 1] - phase_ref.to(D)[:, 1]
        ph = torch.remainder((t1 - p[:, 1]) * 2 * math.pi + math.pi, 2 * math.pi) - math.pi
        e_ph = 1.0 - torch.cos(ph)
        e_w = e_ph if phase_weight is None else e_ph * phase_weight.to(D).view(1, 1, -1)
        loss = (alpha * e_amp + (1 - alpha) * e_w).sum() * inv_norm
        (gp,) = torch.autograd.grad(loss, p)                      # d pred / d logit = 1
        pred.copy_(p.detach().float())
        dlogits.base.zero_()
        dlogits.base[..., :2] = gp.permute(0, 2, 3, 1).to(dlogits.base.dtype)
        loss_out[0] = float(loss.detach()); loss_out[1] = float(e_amp.detach().sum()); loss_out[2] = float(e_ph.detach().sum())

    def linear_nchw(self, logits, pred):
        self.rt.touch([logits], [pred], "linear_nchw")
        pred.copy_(logits.base[..., :2].permute(0, 3, 1, 2).float())

    def linear_bwd(self, pred, dpred, dlogits):
        self.rt.touch([pred, dpred], [dlogits], "linear_bwd")
        dlogits.base.zero_()
        dlogits.base[..., :2] = dpred.permute(0, 2, 3, 1).to(dlogits.base.dtype)

    # ---- Conv2D(2, (1, 1)) on a bf16 trunk
    def head1x1_supported(self, C_):
        return self.head_passes if (C_ % 8 == 0 and 8 <= C_ <= 256) else 0

    def head1x1_bwd_ws_bytes(self, B, H, W, C_):
        return 1 << 12

    def head1x1_fwd(self, x, w, bias, y):
        self._count("fwd")
        self.rt.touch([x, w, bias], [y], "head1x1_fwd")
        wq = w.reshape(-1, x.C)[:2].to(torch.bfloat16).to(D)          # rounded to bf16 on load
        y.base.zero_()
        y.base[..., :2] = (_flat2(x) @ wq.T + bias.to(D)[:2]).reshape(x.B, x.H, x.W, 2).to(y.base.dtype)

    def head1x1_bwd(self, x, dy, w, dx, dw, dbias, ws):
        self._count("bwd")
        self.rt.touch([x, dy, w], [dx, dw, dbias, ws], "head1x1_bwd")
        wq = w.reshape(-1, x.C)[:2].to(torch.bfloat16).to(D)
        g = dy.base[..., :2].reshape(-1, 2).to(D)
        _put2(dx, g @ wq)
        dw.reshape(-1, x.C)[:2] = (g.T @ _flat2(x)).to(dw.dtype)
        dbias[:2] = g.sum(0).to(dbias.dtype)


def install(monkeypatch, rt, family="unet", head_passes=3, c22_passes=7):
    import unet_rir_amd
    if family == "unet":
        import aenet_cpu_ops
        impl = aenet_cpu_ops.install(monkeypatch, rt, c22_passes)
    else:
        import vae_cpu_ops
        impl = vae_cpu_ops.install(monkeypatch, rt)
    d = DiffCpuOps(rt, head_passes)
    for name in dir(d):
        if not name.startswith("_") and name not in ("rt", "head_passes", "calls", "H1_FWD", "H1_BWD"):
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(d, name)))
    impl.diff = d
    return impl
