"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for the entry points of the folded up-sampling head (csrc/head_up2.hip) in
``unet_rir_amd.ops``.  fold / forward / data gradient compute the FOLDED form from the folded work copy the product hands them, the
weight gradient the LITERAL form (tests/head_up2_ref.py): a product that refreshed the copy late, or read the master kernel where the
copy is due, gives other numbers than the restatement the tests compare with.  ``install(monkeypatch, runtime)``."""
import torch

import cpu_ops
import head_up2_ref as HR
from cpu_ops import D, _nchw, _put


class HeadUp2CpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.calls = {}

    def _count(self, what):
        self.calls[what] = self.calls.get(what, 0) + 1

    def head_up2_supported(self, C_, storage="f32"):
        return 7 if C_ > 0 and C_ % 8 == 0 else 0

    def head_up2_folded_elems(self, C_):
        return 128 * int(C_)

    def head_up2_wgrad_ws_bytes(self, B, h, w, C_):
        return 1 << 12

    def head_up2_fold(self, w, wf, C_, round_bf16=False):
        self.rt.touch([w], [wf], "head_up2_fold"); self._count("fold")
        k = w.reshape(-1, 6, 6, C_)[:2]
        kf = HR.fold_bf16(k) if round_bf16 else HR.fold(k.float(), torch.float32)
        wf[:128 * C_] = kf.reshape(-1).float()

    @staticmethod
    def _kf(wf, C_):
        return wf[:128 * C_].view(8, 4, 4, C_).to(D)

    def head_up2_fwd(self, x, wf, bias, y):
        self.rt.touch([x, wf, bias], [y], "head_up2_fwd"); self._count("fwd")
        out = HR.folded(_nchw(x), self._kf(wf, x.C), bias.to(D)[:2])
        y.base.zero_()
        y.base[..., :2] = out.permute(0, 2, 3, 1).to(y.base.dtype)

    def head_up2_dgrad(self, dy, wf, dx):
        self.rt.touch([dy, wf], [dx], "head_up2_dgrad"); self._count("dgrad")
        x0 = torch.zeros((dx.B, dx.C, dx.H, dx.W), dtype=D, requires_grad=True)
        (gx,) = torch.autograd.grad(HR.folded(x0, self._kf(wf, dx.C), None), x0, dy.base[..., :2].to(D).permute(0, 3, 1, 2))
        _put(dx, gx)

    def head_up2_wgrad(self, x, dy, dw, ws):
        self.rt.touch([x, dy], [dw, ws], "head_up2_wgrad"); self._count("wgrad")
        k0 = torch.zeros((2, 6, 6, x.C), dtype=D, requires_grad=True)
        (gk,) = torch.autograd.grad(HR.literal(_nchw(x), k0, None), k0, dy.base[..., :2].to(D).permute(0, 3, 1, 2))
        dw.reshape(-1, 6, 6, x.C)[:2] = gk.to(dw.dtype)


def install(monkeypatch, rt):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    a = HeadUp2CpuOps(rt)
    for name in dir(a):
        if name.startswith("head_up2_"):
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(a, name)))
    impl.head_up2 = a
    return impl
