"""Test infrastructure: tests/cpu_ops.py plus fp64 stand-ins for what LAMB adds to ``unet_rir_amd.ops`` (csrc/lamb.hip): the segment
table and the two forms of the step.  Values come from tests/lamb_ref.py applied to the variables of the range (their real elements
only: a slot's alignment tail is neither read nor written); every call reports the buffers it reads and writes to the simulated
runtime, so the bucket-wise optimizer stream is race-checked with LAMB on it."""
import torch

import cpu_ops
import lamb_ref


class SimLambTable:
    """Stand-in for ops.LambTable: the same host-side bookkeeping, no device copies."""

    def __init__(self, segments, device):
        self.segments = [tuple(s) for s in segments]
        self.n_seg = len(self.segments)
        self.starts = {int(s[0]): i for i, s in enumerate(self.segments)}
        self.ends = {int(s[0]) + int(s[2]): i + 1 for i, s in enumerate(self.segments)}
        self.begin, self.end = int(self.segments[0][0]), int(self.segments[-1][0]) + int(self.segments[-1][2])
        self.ws = torch.zeros(4 * self.n_seg, dtype=torch.uint8)
        self.calls = []                                  # (lo, hi) of every step call, in issue order

    def is_range(self, lo, hi):
        return lo in self.starts and hi in self.ends and self.starts[lo] < self.ends[hi]

    def ratios(self, ws=None):
        return (self.ws if ws is None else ws).view(torch.float32)


class LambCpuOps:
    def __init__(self, rt):
        self.rt = rt
        self.tables = []

    def make_lamb_table(self, segments, device):
        self.tables.append(SimLambTable(segments, device))
        return self.tables[-1]

    def lamb(self, table, theta, g, m, v, lo, hi, lr, beta1, beta2, eps, weight_decay, corr1, corr2, grad_scale=1.0, ws=None):
        assert table.is_range(lo, hi), "the kernels refuse a range that is not made of whole variables (UNETRIR_EINVAL)"
        sl = slice(lo, hi)
        self.rt.touch([theta[sl], g[sl], m[sl], v[sl]], [theta[sl], m[sl], v[sl], table.ws if ws is None else ws], "lamb")
        table.calls.append((lo, hi))
        segs = table.segments[table.starts[lo]:table.ends[hi]]
        views = [tuple(b[off:off + cnt] for b in (theta, g, m, v)) for off, cnt, _, _, _ in segs]
        out = lamb_ref.step([vw + ((dec, ada),) for vw, (_, _, _, dec, ada) in zip(views, segs)], lr, beta1, beta2, eps, weight_decay,
                            corr1, corr2, grad_scale)
        r = table.ratios(ws)
        for k, ((tw, _, tm, tv), o) in enumerate(zip(views, out)):
            tw.copy_(o["w"].float()); tm.copy_(o["m"].float()); tv.copy_(o["v"].float())
            r[table.starts[lo] + k] = o["r"]

    def lamb_dev(self, table, theta, g, m, v, lo, hi, weight_decay, state, cfg, ws=None):
        self.rt.touch([state, cfg], [], "lamb_dev")
        t = int(state[0])
        lr, b1, b2, eps, gs = (float(x) for x in cfg[:5])
        self.lamb(table, theta, g, m, v, lo, hi, lr, b1, b2, eps, weight_decay, 1.0 - b1 ** t, 1.0 - b2 ** t, gs, ws)


def install(monkeypatch, rt):
    import unet_rir_amd
    impl = cpu_ops.install(monkeypatch, rt)
    a = LambCpuOps(rt)
    for name in ("make_lamb_table", "lamb", "lamb_dev"):
        if not hasattr(unet_rir_amd.ops, name):
            raise AttributeError(f"unet_rir_amd.ops has no function {name}")
        monkeypatch.setattr(unet_rir_amd.ops, name, cpu_ops._with_grad(getattr(a, name)))
    impl.lamb_ops = a
    return impl
