"""tfa.optimizers.LAMB on the device (csrc/lamb.hip; trainer.py:37-38, PARITY UNPINNED - the pin is tests/lamb_ref.py).

Kernel level: a synthetic segment table around the chunk size C the library reports - variables of 2 and 46 elements in 64-float
slots, of 64, C, C + 4 and 3 C + 100 elements, one with w == 0, one with g == 0 and zero moments, one not adapted, one not decayed
under weight_decay 0.01 - at t = 1 and t = 1000 with grad_scale 0.5, every element of m, v and w against the fp64 restatement within
a bound derived from the kernel's own fp32 roundings (tests/streaming_check.py's convention; derivations beside each bound), the
trust ratios to one unit in the last place.  Then: a whole-buffer call equals calls variable by variable bit for bit, two runs are
bit-identical, the device-counter form equals the host form, the advertised workspace is honoured in front of a canary.
Engine level: three Trainer steps against the restatement advanced with the engine's own gradients (both storage types), the graph
step, the launched step with device counters and the launched step with host arguments end bit-identical, the padded kinds of an
AE-family engine stay zero, and a checkpoint resumes bit-exactly."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_ref  # noqa: E402
import streaming_check as S  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = torch.float32
LR, B1, B2, EPS, WD, GS = 1e-2, 0.9, 0.999, 1e-6, 0.01, 0.5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


def f32c(x):
    """x as the fp32 number the kernels hold."""
    return float(torch.tensor(x, dtype=F32))


def one_minus(b):
    """1.f - b in fp32, as the kernels form it."""
    return float(torch.tensor(1.0, dtype=F32) - torch.tensor(b, dtype=F32))


def corrections(t, b1=B1, b2=B2):
    """(float)(1 - beta^t) from the fp32 betas in fp64: what the host passes and what the device form computes."""
    return f32c(1.0 - f32c(b1) ** t), f32c(1.0 - f32c(b2) ** t)


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(U):
    """The synthetic parameter set: (count, (decayed, adapted), data kind) per variable, 64-float slots, built once."""
    Cn = U.ops.lamb_chunk_elems()
    DA = (True, True)
    spec = [(2, DA, "rand"), (46, DA, "rand"), (64, DA, "rand"), (Cn, DA, "rand"), (Cn + 4, DA, "rand"), (3 * Cn + 100, DA, "rand"),
            (300, DA, "w0"), (200, (False, True), "g0"), (1000, (True, False), "rand"), (520, (False, True), "rand")]
    gen = torch.Generator(); gen.manual_seed(17)
    segs, off = [], 0
    for cnt, (dec, ada), _ in spec:
        slot = -(-cnt // 64) * 64
        segs.append((off, cnt, slot, dec, ada))
        off += slot
    n = off
    theta, g, m, v = torch.zeros(n), torch.ones(n), torch.zeros(n), torch.zeros(n)      # tails: theta / m / v zero, g deliberately NOT
    for (o, cnt, _, _, _), (_, _, kind) in zip(segs, spec):
        theta[o:o + cnt] = 0.0 if kind == "w0" else (torch.rand(cnt, generator=gen) * 2 - 1)
        g[o:o + cnt] = 0.0 if kind == "g0" else (torch.rand(cnt, generator=gen) * 2 - 1)
        m[o:o + cnt] = 0.0 if kind == "g0" else (torch.rand(cnt, generator=gen) * 0.2 - 0.1)
        v[o:o + cnt] = 0.0 if kind == "g0" else (torch.rand(cnt, generator=gen) * 0.1)
    table = U.ops.make_lamb_table(segs, DEV)
    assert table.n_chunks == sum(-(-c // Cn) for c, _, _ in spec) and table.end == n
    return dict(C=Cn, spec=spec, segs=segs, n=n, theta=theta, g=g, m=m, v=v, table=table)


def _run(U, case, t, ranges=None, ws=None, dev=False, wd=WD):
    """One LAMB step on fresh copies; ranges: [(lo, hi)] (default: the whole buffer in one call).  Returns theta, m, v, r on the host."""
    tab = case["table"]
    th, g, m, v = (case[k].clone().to(DEV) for k in ("theta", "g", "m", "v"))
    c1, c2 = corrections(t)
    if dev:
        state = torch.tensor([t, 0, 0], dtype=torch.int64, device=DEV)
        cfg = torch.tensor([LR, B1, B2, EPS, GS, 0, 0, 0], dtype=F32, device=DEV)
    for lo, hi in (ranges or [(0, tab.end)]):
        if dev:
            U.ops.lamb_dev(tab, th, g, m, v, lo, hi, wd, state, cfg, ws=ws)
        else:
            U.ops.lamb(tab, th, g, m, v, lo, hi, LR, B1, B2, EPS, wd, c1, c2, grad_scale=GS, ws=ws)
    _sync()
    assert torch.equal(g.cpu(), case["g"]), "the gradient stays readable"
    return th.cpu(), m.cpu(), v.cpu(), tab.ratios(ws).clone().cpu()


def _ulps(a, b):
    """Distance of two positive fp32 numbers in units in the last place."""
    return abs(int(torch.tensor(a, dtype=F32).view(torch.int32)) - int(torch.tensor(b, dtype=F32).view(torch.int32)))


@pytest.mark.parametrize("t", [1, 1000])
def test_kernels_element_by_element(U, case, t):
    th, m, v, r = _run(U, case, t)
    c1, c2 = corrections(t)
    b1, b2, eps, wd, gs, lr = (f32c(x) for x in (B1, B2, EPS, WD, GS, LR))
    T = lambda x: torch.tensor(x, dtype=F32)
    for i, ((o, cnt, slot, dec, ada), (_, _, kind)) in enumerate(zip(case["segs"], case["spec"])):
        what = f"variable {i} ({cnt} elements, {kind}) t={t}"
        sl, tail = slice(o, o + cnt), slice(o + cnt, o + slot)
        w0, g0, m0, v0 = (case[k][sl] for k in ("theta", "g", "m", "v"))
        # the alignment tail of the slot: untouched and still zero, whatever the gradient buffer holds there
        for got in (th, m, v):
            assert float(got[tail].abs().max() if slot > cnt else 0.0) == 0.0, what
        # m' = b1 m + (1.f - b1) gk, gk = g * gs: gk (1), two products (2), the sum (1) -> 4 roundings of at most |b1 m| + |(1 - b1) gk|;
        # v' = b2 v + (1.f - b2) gk gk: gk twice (2), two products (2), the sum (1) -> 5 (a contracted fma only lowers either)
        gk = g0.double() * gs
        a, b = b1 * m0.double(), one_minus(B1) * gk
        c, d = b2 * v0.double(), one_minus(B2) * gk * gk
        S.check(m[sl], a + b, 4 * S.U32 * (a.abs() + b.abs()), f"lamb m {what}", "lamb")
        S.check(v[sl], c + d, 5 * S.U32 * (c.abs() + d.abs()), f"lamb v {what}", "lamb")
        # the trust ratio from the STORED m', v' and the old w.  u is a chain of correctly rounded fp32 operations, none contracted
        # (m' / c1, v' / c2, sqrtf, + eps, the quotient, [wd * w, the sum]), so the fp32 values the kernel squares are reproduced
        # exactly here; what remains free is the order of the fp64 sums: r = (float)(sqrt(sum w^2) / sqrt(sum u^2)) to 1 ulp
        u32 = (m[sl] / T(c1)) / (torch.sqrt(v[sl] / T(c2)) + T(eps))
        if dec:
            u32 = u32 + T(wd) * w0
        nw, nu = float(w0.double().pow(2).sum().sqrt()), float(u32.double().pow(2).sum().sqrt())
        r_want = f32c(nw / nu) if (ada and nw > 0 and nu > 0) else 1.0
        assert _ulps(float(r[i]), r_want) <= 1, (what, float(r[i]), r_want)
        if kind in ("w0", "g0") or not ada:
            assert float(r[i]) == 1.0, what
        # w' = w - (lr r) u from the STORED m', v', r.  q = m^ / (sqrtf(v^) + eps): m' / c1 (a quotient: 2), v' / c2 (2, halved by the
        # root: 1), sqrtf (2), + eps (1), the quotient (2) -> 8 roundings of |q|; the decay term: wd * w (1, of |wd w|) and the sum (1,
        # of |q| + |wd w|); the step: lr * r (1) and its product with u (1) -> 2 of |upd|; the difference: 1 of |w| + |upd|
        q = (m[sl].double() / c1) / (torch.sqrt(v[sl].double() / c2) + eps)
        dq = 8 * S.U32 * q.abs()
        if dec:
            dw_ = wd * w0.double()
            u, du = q + dw_, dq + S.U32 * dw_.abs() + S.U32 * (q.abs() + dw_.abs())
        else:
            u, du = q, dq
        step = lr * float(r[i])
        upd = step * u
        S.check(th[sl], w0.double() - upd, S.U32 * (w0.double().abs() + upd.abs()) + step * du + 2 * S.U32 * upd.abs(), f"lamb theta {what}", "lamb")
        # ... and the whole step against the restatement from the ORIGINAL state: the same bound with the moments' own bounds carried
        # through is what the three checks above compose to; here only the corner cases' exact outcomes are restated
        if kind == "g0":
            assert torch.equal(th[sl], w0) and float(m[sl].abs().max()) == 0.0 and float(v[sl].abs().max()) == 0.0, what
    # ... and r against the restatement from the ORIGINAL state.  |r - r_ref| / r_ref <= ||du|| / ||u|| + 2 roundings (the quotient's, and
    # the conversion's), du the elementwise bound of the kernel's u against the restatement's: the moments' own bounds carried through
    # q = m^ / (sqrt(v^) + eps) - dm' / (c1 (sqrt(v^) + eps)) and, v' being a sum of positive terms, 5 / 2 roundings of |q| under the
    # root - plus the 8 (+ 2 with the decay term) roundings of u itself derived above
    ref = lamb_ref.step([(case["theta"][o:o + cnt], case["g"][o:o + cnt], case["m"][o:o + cnt], case["v"][o:o + cnt], (dec, ada))
                         for o, cnt, _, dec, ada in case["segs"]], lr, b1, b2, eps, wd, c1, c2, gs, one_minus=one_minus)
    for i, ((o, cnt, _, dec, ada), want) in enumerate(zip(case["segs"], ref)):
        nu = float(want["u"].norm())
        if not ada or nu == 0 or float(case["theta"][o:o + cnt].abs().max()) == 0:
            assert float(r[i]) == 1.0 == want["r"], i
            continue
        gk = case["g"][o:o + cnt].double() * gs
        dm = 4 * S.U32 * ((b1 * case["m"][o:o + cnt].double()).abs() + (one_minus(B1) * gk).abs())
        den = torch.sqrt(want["v"] / c2) + eps
        q = (want["m"] / c1) / den
        dwt = (wd * case["theta"][o:o + cnt].double()).abs() if dec else torch.zeros_like(q)
        du = dm / (c1 * den) + (2.5 + 8) * S.U32 * q.abs() + S.U32 * dwt + S.U32 * (q.abs() + dwt)
        assert abs(float(r[i]) - want["r"]) <= want["r"] * (float(du.norm()) / nu + 2 * S.U32), (i, float(r[i]), want["r"])


def test_whole_buffer_equals_range_by_range_bit_for_bit(U, case):
    """A variable's chunks are numbered from its own start, so its reduction order - every bit of r, and with it of w - does not depend
    on what else a call covers; no atomics, so two runs agree; the device-counter form computes the corrections by the same expression."""
    full = _run(U, case, 3)
    again = _run(U, case, 3)
    by_var = _run(U, case, 3, ranges=[(o, o + slot) for o, _, slot, _, _ in case["segs"]])
    mid = case["segs"][5][0]
    halves = _run(U, case, 3, ranges=[(mid, case["n"]), (0, mid)])                   # two buckets, in the order a backward pass ends them
    dev = _run(U, case, 3, dev=True)
    for other, name in ((again, "second run"), (by_var, "variable by variable"), (halves, "two buckets"), (dev, "device counters")):
        for a, b, what in zip(full, other, ("theta", "m", "v", "r")):
            assert torch.equal(a, b), (name, what)
    assert not torch.equal(full[0], case["theta"])


def test_workspace_is_honoured_exactly(U, case):
    """The step runs in exactly unetrir_lamb_ws_bytes bytes (a canary behind them survives) and refuses one byte less."""
    tab = case["table"]
    need = U.ops.lamb_ws_bytes(tab.n_seg, tab.n_chunks)
    assert need == tab.ws_bytes == 16 * tab.n_chunks + 4 * tab.n_seg
    buf = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    got = _run(U, case, 3, ws=buf[:need])
    assert bool((buf[need:] == 0xA5).all())
    for a, b in zip(got, _run(U, case, 3)):
        assert torch.equal(a, b)
    with pytest.raises(U.UnetrirError):
        _run(U, case, 3, ws=buf[:need - 1])
    th = case["theta"].to(DEV)
    with pytest.raises(U.UnetrirError):                     # not a range of whole variables
        U.ops.lamb(tab, th, th.clone(), th.clone(), th.clone(), 64, tab.end - 64, LR, B1, B2, EPS, WD, 0.1, 0.001)
    with pytest.raises(ValueError):                         # buffers shorter than the table
        U.ops.lamb(tab, th[:64], th, th, th, 0, 64, LR, B1, B2, EPS, WD, 0.1, 0.001)


# ----------------------------------------------------------------------------------------------------------------------
# engine level
# ----------------------------------------------------------------------------------------------------------------------
DIMS = {"unet": (32, 48, 2), "ae": (64, 64, 4)}              # H, W, batch


def _engine(U, dtype, overlap=True, kind="unet"):
    H, W, B = DIMS[kind]
    if kind == "unet":
        eng = U.UNetEngine(H, W, B, F0=32, k=3, device=DEV, dtype=dtype, overlap_wgrad=overlap)
    else:
        eng = U.AutoencoderEngine(H, W, B, (8, 16, 32, 64), (3, 3, 3, 3), (2, 2, 2, 2), 32, 64, device=DEV, dtype=dtype, overlap_wgrad=overlap)
    g = torch.Generator(); g.manual_seed(3)
    eng.reset_parameters(g)
    eng.dropout_seed = 77
    return eng


def _batches(n, kind="unet"):
    H, W, B = DIMS[kind]
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((B, 2, H, W), generator=gen).to(DEV), torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV),
             torch.rand((B, 2, H, W), generator=gen).to(DEV)) for _ in range(n)]


class _Ref:
    """The restatement, advanced with the engine's own gradients, and per variable the bound of the engine's distance from it.

    Derived as for the Nadam step test, per step and variable, from the restatement's own values: the moments' 4 resp. 5 roundings of
    at most max(|m|, |g|) resp. max(|v|, g^2); for w the final rounding of at most max|w|, and 32 roundings of the largest update
    lr r max|u| - 8 + 2 of u itself, 3 of the step, 10 through the norm of u into r, and 8 more for what the moments' own
    roundings move u by where u = +-1 (the first steps: m^ / sqrt(v^) of a single gradient), with one to spare.  The bounds add up
    over the steps (the restatement continues from ITS state)."""

    def __init__(self, eng, opt):
        self.eng, self.opt = eng, opt
        self.names = list(eng.specs)
        self.w = [eng.p[n].detach().double().cpu().clone() for n in self.names]
        self.m = [torch.zeros_like(w) for w in self.w]
        self.v = [torch.zeros_like(w) for w in self.w]
        self.tol = [[0.0, 0.0, 0.0] for _ in self.names]
        self.t = 0

    def advance(self, lr):
        eng, o = self.eng, self.opt
        self.t += 1
        g = [eng.g[n].detach().double().cpu() for n in self.names]
        c1, c2 = corrections(self.t, o.beta_1, o.beta_2)
        out = lamb_ref.step([(w, gg, m, v, (o.decayed(n), o.adapted(n))) for n, w, gg, m, v in zip(self.names, self.w, g, self.m, self.v)],
                            f32c(lr), f32c(o.beta_1), f32c(o.beta_2), f32c(o.epsilon), f32c(o.weight_decay), c1, c2, 1.0, one_minus=one_minus)
        for i, r in enumerate(out):
            tol = self.tol[i]
            tol[0] += S.U32 * float(self.w[i].abs().max()) + 32 * S.U32 * f32c(lr) * r["r"] * float(r["u"].abs().max())
            tol[1] += 4 * S.U32 * max(float(self.m[i].abs().max()), float(g[i].abs().max()))
            tol[2] += 5 * S.U32 * max(float(self.v[i].abs().max()), float(g[i].abs().max()) ** 2)
            self.w[i], self.m[i], self.v[i] = r["w"], r["m"], r["v"]

    def check(self):
        eng = self.eng
        for i, n in enumerate(self.names):
            s_ = eng.specs[n]
            sl = slice(s_.offset, s_.offset + s_.numel)
            for buf, want, tol, what in ((eng.theta, self.w[i], self.tol[i][0], "theta"), (eng.adam_m, self.m[i], self.tol[i][1], "m"),
                                         (eng.adam_v, self.v[i], self.tol[i][2], "v")):
                err = float((buf[sl].double().cpu() - want.reshape(-1)).abs().max())
                assert err <= tol + S.TINY, (n, what, err, tol, self.t)


def _padding_is_zero(eng):
    for n, s_ in eng.specs.items():
        for buf in (eng.theta, eng.adam_m, eng.adam_v):
            view = buf[s_.offset:s_.offset + s_.numel].view(s_.shape)
            assert float(buf[s_.offset + s_.numel:s_.end].abs().max() if s_.end > s_.offset + s_.numel else 0.0) == 0.0, n
            if s_.kind in ("conv_padin", "convT_padout"):
                assert float(view[..., 2:].abs().max()) == 0.0, n
            if s_.kind in ("conv_padout", "bias_pad"):
                assert float(view[2:].abs().max()) == 0.0, n


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_three_trainer_steps_against_the_restatement(U, dtype):
    eng = _engine(U, dtype)
    opt = U.LAMB(learning_rate=1e-3)
    tr = U.Trainer(eng, optimizer=opt, bucket_bytes=16 << 10)
    assert eng.optimizer == "lamb" and tr.lr == 1e-3 and tr.bucketer is not None and len(tr.bucketer.bounds) > 3
    ref = _Ref(eng, opt)
    for (a, e, b), lr in zip(_batches(3), (None, None, 5e-4)):
        tr.step(a, e, b, lr=lr)
        _sync()
        ref.advance(1e-3 if lr is None else lr)            # the gradients stay readable after the step
        ref.check()
    assert eng.adam_t == 3
    _padding_is_zero(eng)
    # the trust ratio at work: every adapted variable with a gradient moved by lr ||w|| in the last step, to rounding
    assert float(eng._lamb_table().ratios().min()) > 0


@pytest.mark.parametrize("dtype,overlap", [("bf16", True), ("f32", False)])
def test_graph_and_launched_steps_are_bit_identical(U, dtype, overlap):
    """Three steps, the last with a changed rate, dropout on: the captured graph, the same launches with the counters in device memory,
    and the launches with host arguments (the corrections formed on the host by the same fp64 expression) end in the same bits."""
    data, lrs = _batches(3), (1e-3, 1e-3, 5e-4)
    res = []
    for mode in ("graph", "eager_dev", "eager_host"):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, optimizer=U.LAMB(learning_rate=1e-3), bucket_bytes=16 << 10, graph=(mode == "graph"))
        assert tr.use_graph == (mode == "graph")
        if mode == "eager_dev":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, lr=lr, return_loss=True) for (a, e, b), lr in zip(data, lrs)]
        _sync()
        res.append((losses, eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), eng.adam_t))
    for other, name in ((res[1], "device counters"), (res[2], "host arguments")):
        assert res[0][0] == other[0], name
        for a, b, what in zip(res[0][1:4], other[1:4], ("theta", "m", "v")):
            assert torch.equal(a, b), (name, what)
        assert res[0][4] == other[4] == 3


def test_ae_family_padded_kinds_stay_zero_under_weight_decay(U):
    """conv_padout / convT_padout / bias_pad of an AE-family engine: one step with weight_decay > 0 leaves every padded element of
    theta and of the moments exactly zero, and the step equals the restatement."""
    eng = _engine(U, "bf16", kind="ae")
    kinds = {s_.kind for s_ in eng.specs.values()}
    assert kinds & {"conv_padout", "convT_padout"} and "bias_pad" in kinds
    opt = U.LAMB(learning_rate=1e-3, weight_decay=0.01, exclude_from_weight_decay=["bias"])
    tr = U.Trainer(eng, optimizer=opt)
    ref = _Ref(eng, opt)
    (a, e, b), = _batches(1, "ae")
    tr.step(a, e, b)
    _sync()
    ref.advance(1e-3)
    ref.check()
    _padding_is_zero(eng)


def test_checkpoint_resumes_bit_exactly(U, tmp_path):
    data = _batches(4)

    def trainer():
        eng = _engine(U, "bf16")
        return eng, U.Trainer(eng, optimizer=U.LAMB(learning_rate=1e-3, weight_decay=0.01), bucket_bytes=16 << 10)
    e0, t0 = trainer()
    for a, e, b in data[:2]:
        t0.step(a, e, b)
    path = U.CheckpointManager(t0, str(tmp_path)).save(epoch=0)
    saved = torch.load(path, map_location="cpu", weights_only=True)
    assert saved["optimizer"] == "lamb" and saved["lamb"]["weight_decay"] == 0.01 and saved["adam_t"] == 2
    for a, e, b in data[2:]:
        t0.step(a, e, b)
    e1, t1 = trainer()
    e1.dropout_seed = 5                                   # overwritten by the checkpoint
    U.CheckpointManager(t1, str(tmp_path)).restore(path)
    for a, e, b in data[2:]:
        t1.step(a, e, b)
    _sync()
    assert e0.adam_t == e1.adam_t == 4
    for x, y, what in ((e0.theta, e1.theta, "theta"), (e0.adam_m, e1.adam_m, "m"), (e0.adam_v, e1.adam_v, "v")):
        assert torch.equal(x, y), what
