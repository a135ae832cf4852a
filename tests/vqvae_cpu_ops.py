"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for the quantiser kernels of csrc/vq.hip behind ``unet_rir_amd.ops``.

``install(monkeypatch, runtime)`` calls ``cpu_ops.install`` and then replaces vq_fwd / vq_bwd / vae_loss_add with restatements in
torch CPU fp64 (tests/vqvae_ref.py) that report what they read and write to the simulated runtime (tests/sim_runtime.py) like the
others.  The product's VQVAEEngine + Trainer then run unmodified on CPU tensors.
"""
import torch

import cpu_ops
import vqvae_ref as Q
from cpu_ops import D, _flat2, _put2


class VqCpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.n_fwd = self.n_bwd = 0
        self.indices = None              # when set: the codes to take instead of searching (tests that pin the index map)

    def vq_fwd(self, x, Dv, E, beta, r, idx, y, vq_out, ws):
        self.rt.touch([x, E, ws], [idx, y, vq_out, ws], "vq_fwd")
        self.n_fwd += 1
        yv, term, S, i = Q.quantize(_flat2(x), E.to(D), beta, r, self.indices)
        _put2(y, yv)
        idx.copy_(i.to(torch.int32))
        vq_out[0], vq_out[1] = float(term), float(S)

    def vq_bwd(self, x, Dv, idx, E, dy, beta, r, dx, dE):
        self.rt.touch([x, idx, E, dy], [dx, dE], "vq_bwd")
        self.n_bwd += 1
        gx, gE = Q.quantize_grads(_flat2(x), E.to(D), idx, _flat2(dy), beta, r)
        _put2(dx, gx)
        dE.copy_(gE.float())

    def vae_loss_add(self, kl_out, loss_out):
        self.rt.touch([kl_out, loss_out], [loss_out], "vae_loss_add")
        loss_out[0] = float(loss_out[0].to(D) + kl_out[0].to(D))


def install(monkeypatch, rt):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    vimpl = VqCpuOps(rt)
    for name in dir(vimpl):
        if not name.startswith("_") and name not in ("rt", "n_fwd", "n_bwd", "indices"):
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, getattr(vimpl, name))
    impl.vq = vimpl
    return impl
