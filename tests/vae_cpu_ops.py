"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for the VAE kernels of csrc/vae.hip behind ``unet_rir_amd.ops``.

``install(monkeypatch, runtime)`` calls ``cpu_ops.install`` and then replaces normal / normal_dev / vae_sample_kl_fwd /
vae_sample_kl_bwd / vae_loss_add with restatements in torch CPU fp64 that report what they read and write to the simulated runtime
(tests/sim_runtime.py) like the others.  The product's VAEEngine + Trainer then run unmodified on CPU tensors.
"""
import torch

import cpu_ops
from cpu_ops import D, _flat2, _put2


class VaeCpuOps:
    def __init__(self, rt):
        self.rt = rt

    def normal(self, out, seed, step):
        """Not the kernel's bits (tests/test_vae_gpu.py restates those): a deterministic function of (seed, step), prefix-stable."""
        self.rt.touch([], [out], "normal")
        gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(step)) ^ 0x4E4F524D)
        out.reshape(-1).copy_(torch.randn(out.numel(), generator=gen, dtype=D).float())

    def normal_dev(self, out, seed, state, offset):
        self.rt.touch([state], [out], "normal_dev")
        gen = torch.Generator().manual_seed((int(seed) * 1000003 + int(state[2]) + int(offset)) ^ 0x4E4F524D)
        out.reshape(-1).copy_(torch.randn(out.numel(), generator=gen, dtype=D).float())

    def vae_sample_kl_fwd(self, mu, log_var, eps, inv_global_batch, z, kl_out):
        self.rt.touch([mu, log_var, eps], [z, kl_out], "vae_sample_kl_fwd")
        m, l, e = _flat2(mu), _flat2(log_var), eps.to(D).reshape(mu.P, mu.C)
        _put2(z, m + torch.exp(0.5 * l) * e)
        raw = float((-0.5 * (1 + l - m * m - torch.exp(l))).sum())
        kl_out[1] = raw
        kl_out[0] = inv_global_batch * raw

    def vae_sample_kl_bwd(self, mu, log_var, eps, dz, inv_global_batch, dmu, dlv):
        self.rt.touch([mu, log_var, eps, dz], [dmu, dlv], "vae_sample_kl_bwd")
        m, l, e, g = _flat2(mu), _flat2(log_var), eps.to(D).reshape(mu.P, mu.C), _flat2(dz)
        _put2(dmu, g + inv_global_batch * m)
        _put2(dlv, g * 0.5 * torch.exp(0.5 * l) * e + inv_global_batch * 0.5 * (torch.exp(l) - 1.0))

    def vae_loss_add(self, kl_out, loss_out):
        self.rt.touch([kl_out, loss_out], [loss_out], "vae_loss_add")
        loss_out[0] = float(loss_out[0].to(D) + kl_out[0].to(D))


def install(monkeypatch, rt):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    vimpl = VaeCpuOps(rt)
    for name in dir(vimpl):
        if not name.startswith("_") and name != "rt":
            if not hasattr(unet_rir_amd.ops, name):
                raise AttributeError(f"unet_rir_amd.ops has no function {name}")
            monkeypatch.setattr(unet_rir_amd.ops, name, getattr(vimpl, name))
    return impl
