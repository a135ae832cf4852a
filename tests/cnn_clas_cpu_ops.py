"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for what deep_CNN adds to ``unet_rir_amd.ops`` (csrc/cnn_clas.hip): the
'valid' 3x3 convolution and its gradients, average / global pooling with the folded BatchNorm affine, and the softmax + cross-entropy
+ accuracy output.  Built on the library calls of torch (F.conv2d, F.avg_pool2d, F.log_softmax) and autograd, not on
tests/cnn_clas_ref.py, which the engine is then compared with."""
import torch
import torch.nn.functional as F

import cpu_ops
from cpu_ops import D, _flat2, _nchw, _put


class CnnClasCpuOps:
    def __init__(self, rt):
        self.rt = rt

    def conv3x3_valid_wgrad_ws_bytes(self, g):
        return 1 << 12

    @staticmethod
    def _masked(dy, y, relu):
        g = _nchw(dy)
        return g * (_nchw(y) > 0) if relu else g

    def conv3x3_valid_fwd(self, g, x, w, bias, y, relu=True):
        self.rt.touch([x, w, bias], [y], "conv3x3_valid_fwd")
        out = F.conv2d(_nchw(x), w.reshape(g.Cout, 3, 3, g.Cin).to(D).permute(0, 3, 1, 2), bias.to(D), padding=0)
        _put(y, F.relu(out) if relu else out)

    def conv3x3_valid_dgrad(self, g, dy, y, wt, dx, relu=True):
        self.rt.touch([dy, y if relu else None, wt], [dx], "conv3x3_valid_dgrad")
        w = wt.reshape(g.Cin, 3, 3, g.Cout).to(D).permute(3, 0, 1, 2)             # -> OIHW
        x0 = torch.zeros((g.B, g.Cin, g.H, g.W), dtype=D, requires_grad=True)
        (gx,) = torch.autograd.grad(F.conv2d(x0, w, None, padding=0), x0, self._masked(dy, y, relu))
        _put(dx, gx)

    def conv3x3_valid_wgrad(self, g, x, dy, y, dw, dbias, ws, relu=True):
        self.rt.touch([x, dy, y if relu else None], [dw, dbias, ws], "conv3x3_valid_wgrad")
        w0 = torch.zeros((g.Cout, g.Cin, 3, 3), dtype=D, requires_grad=True)
        gm = self._masked(dy, y, relu)
        (gw,) = torch.autograd.grad(F.conv2d(_nchw(x), w0, None, padding=0), w0, gm)
        dw.reshape(g.Cout, 3, 3, g.Cin).copy_(gw.permute(0, 2, 3, 1).to(dw.dtype))
        dbias.copy_(gm.sum((0, 2, 3)).to(dbias.dtype))

    @staticmethod
    def _affine(v, affine, C_):
        if affine is None:
            return v
        return v * affine[:C_].to(D).view(1, -1, 1, 1) + affine[C_:].to(D).view(1, -1, 1, 1)

    def avgpool2_fwd(self, x, affine, y):
        self.rt.touch([x, affine], [y], "avgpool2_fwd")
        _put(y, self._affine(F.avg_pool2d(_nchw(x), 2), affine, x.C))

    def avgpool2_bwd(self, dy, dx):
        self.rt.touch([dy], [dx], "avgpool2_bwd")
        x0 = torch.zeros((dx.B, dx.C, dx.H, dx.W), dtype=D, requires_grad=True)
        (gx,) = torch.autograd.grad(F.avg_pool2d(x0, 2), x0, _nchw(dy))
        _put(dx, gx)

    def gap_fwd(self, x, affine, y):
        self.rt.touch([x, affine], [y], "gap_fwd")
        _put(y, self._affine(_nchw(x).mean((2, 3), keepdim=True), affine, x.C))

    def gap_bwd(self, dy, dx):
        self.rt.touch([dy], [dx], "gap_bwd")
        _put(dx, (_nchw(dy) / (dx.H * dx.W)).expand(dx.B, dx.C, dx.H, dx.W))

    def softmax_ce(self, logits, classes, target, inv_norm, probs, dlogits, loss_out, acc_out):
        self.rt.touch([logits, target], [probs, dlogits, loss_out, acc_out], "softmax_ce")
        z = _flat2(logits)[:, :classes].clone().requires_grad_(True)
        y = target.to(D)
        ce = -(y * F.log_softmax(z, 1)).sum()
        (gz,) = torch.autograd.grad(ce * inv_norm, z)
        probs.copy_(F.softmax(z.detach(), 1).float())
        dlogits.base.zero_()
        dlogits.base.view(logits.P, -1)[:, :classes] = gz.to(dlogits.base.dtype)
        loss_out[0] = float(ce.detach()) * inv_norm; loss_out[1] = float(ce.detach()); loss_out[2] = 0.0
        acc_out[0] = float((torch.argmax(z.detach(), 1) == torch.argmax(y, 1)).sum())

    def softmax_fwd(self, logits, classes, probs):
        self.rt.touch([logits], [probs], "softmax_fwd")
        probs.copy_(F.softmax(_flat2(logits)[:, :classes], 1).float())

    def softmax_bwd(self, probs, dprobs, classes, dlogits):
        self.rt.touch([probs, dprobs], [dlogits], "softmax_bwd")
        p, g = probs.to(D), dprobs.to(D)
        dlogits.base.zero_()
        dlogits.base.view(p.shape[0], -1)[:, :classes] = (p * (g - (g * p).sum(1, keepdim=True))).to(dlogits.base.dtype)


def install(monkeypatch, rt):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    a = CnnClasCpuOps(rt)
    for name in dir(a):
        if not name.startswith("_") and name != "rt":
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(a, name)))
    impl.cnn_clas = a
    return impl
