"""The VAE on the GPU: the kernels of csrc/vae.hip element by element against fp64 (the method of tests/streaming_check.py), the
normal draw against a NumPy restatement of the documented recipe, the whole network against tests/vae_ref.py, the step machinery
(reproducible draws, HIP-graph replay, checkpoint resume) and the module surface.

Bounds (U32 = 2^-24, U64 = 2^-53, as in tests/streaming_check.py: k fp32 roundings of an expression give k * U32 * S with S the sum
of the absolute values of its terms).  The device's expf / logf / cospif are held to the OpenCL full-profile limits (exp 3 ulp,
log 3 ulp, cospi 4 ulp, sqrt 3 ulp - the library documents tighter ones); 1 ulp <= 2^-23 relative = 2 U32.

  z   = mu + e * eps,  e = expf(0.5f * lv) (the argument is exact): 6 U32 |e eps| (exp) + 1 (product) + 1 on |mu| + |e eps| (sum):
        d = U32 (|mu| + 8 |e eps|)
  t   = -0.5f (1 + lv - mu^2 - expf(lv)), S = 1 + |lv| + mu^2 + exp(lv): the sums / the square are 4 roundings of partial results
        <= S, expf 6 U32 exp(lv), the factor 0.5 is exact:  d_t = 0.5 U32 (4 S + 6 exp(lv))
  kl_out[1] = (float) of the fp64 sum of the t (fixed order, P = B L addends):
        d = sum d_t + P U64 sum |t| + U32 (|ref| + sum d_t);   kl_out[0] = inv_gb * kl_out[1] is ONE fp32 product: equality
  dmu = dz + inv_gb mu: 2 roundings (an fma 1):  d = 2 U32 (|dz| + |inv_gb mu|)
  dlv = a + b, a = dz 0.5 e eps, b = inv_gb 0.5 (expf(lv) - 1): a: 6 (exp) + 2 products; b: 6 U32 exp(lv) + 1 on exp(lv) + 1
        (difference), 1 product; the sum 1 on |a| + |b|, |b| <= 0.5 inv_gb (exp(lv) + 1):
        d = U32 (9 |a| + 5 inv_gb (exp(lv) + 1))
  normal: out = s * c, s = sqrtf(-2 logf(u1)), c = cospif(2 u2), u1 and 2 u2 exact: log 6 U32 relative, halved by the root (3),
        the root 6, the cosine 8 (relative: its argument reduction is exact), the product 1: 18 U32 |ref|, taken as 20 to cover the
        second-order terms; plus the fp64 reference's own error in cos(2 pi u2) near its zeros, 16 U64 s.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import streaming_check as SC  # noqa: E402
import vae_ref as V  # noqa: E402
from oracle import detrand, torch_ref as R  # noqa: E402
from streaming_check import U32, U64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = torch.float64


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


# ----------------------------------------------------------------------------------------------------------------------
# the sampling + KL kernels, element by element
# ----------------------------------------------------------------------------------------------------------------------
def _strided(U, x, ld):
    """[B, L] values in an Act with pixel stride ld (the padding holds NaNs: nothing may read or count it)."""
    B, L = x.shape
    base = torch.full((B, 1, 1, ld), float("nan"), dtype=torch.float32, device=DEV)
    base[:, 0, 0, :L] = x.to(DEV)
    return U.ops.Act(base, 0, L)


def _kl_case(name, B, L, zero_eps):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    mu = torch.randn((B, L), generator=g) * 2.0
    lv = torch.rand((B, L), generator=g) * 30.0 - 20.0               # roughly [-20, 10]
    lv[0, :4] = torch.tensor([-20.0, 10.0, 0.0, -0.0])
    eps = torch.randn((B, L), generator=g)
    eps[:, ::5] = 0.0
    if zero_eps:
        eps.zero_()
    dz = torch.randn((B, L), generator=g) * 0.1
    return mu, lv, eps, dz


@pytest.mark.parametrize("B,L,lds,zero_eps", [(2, 8, (8, 8, 8, 8, 8, 8), False), (37, 24, (32, 28, 40, 36, 24, 44), False),
                                              (32, 64, (64, 64, 64, 64, 64, 64), True), (300, 64, (64, 68, 64, 64, 72, 64), False)])
def test_sample_kl_kernels_element_by_element(U, B, L, lds, zero_eps):
    ops = U.ops
    mu, lv, eps, dz = _kl_case(f"kl{B}x{L}", B, L, zero_eps)
    gb = 3 * B
    igb = float(torch.tensor(1.0 / gb, dtype=torch.float32))         # inv_global_batch as the kernel receives it
    a_mu, a_lv, a_dz = _strided(U, mu, lds[0]), _strided(U, lv, lds[1]), _strided(U, dz, lds[3])
    a_z = _strided(U, torch.zeros(B, L), lds[2])
    a_dmu, a_dlv = _strided(U, torch.zeros(B, L), lds[4]), _strided(U, torch.zeros(B, L), lds[5])
    e_dev = eps.to(DEV).contiguous()
    kl = torch.full((4,), -1.0, device=DEV)
    ops.vae_sample_kl_fwd(a_mu, a_lv, e_dev, 1.0 / gb, a_z, kl)
    ops.vae_sample_kl_bwd(a_mu, a_lv, e_dev, a_dz, 1.0 / gb, a_dmu, a_dlv)
    kl2 = torch.full((4,), -2.0, device=DEV)
    a_z2 = _strided(U, torch.zeros(B, L), lds[2])
    ops.vae_sample_kl_fwd(a_mu, a_lv, e_dev, 1.0 / gb, a_z2, kl2)
    torch.cuda.synchronize()
    m, l, e, g = mu.double(), lv.double(), eps.double(), dz.double()
    ee = torch.exp(0.5 * l) * e
    got = lambda a: a.base[:, 0, 0, :L].cpu()
    SC.check(got(a_z), m + ee, U32 * (m.abs() + 8 * ee.abs()), "z", kernel="vae_sample_kl_fwd")
    if zero_eps:
        assert torch.equal(got(a_z), mu)                              # eps = 0: z IS the mean, whatever log_var
    # padding untouched, in every output
    for a in (a_z, a_dmu, a_dlv):
        if a.ld > L:
            assert bool(torch.isnan(a.base[:, 0, 0, L:]).all())
    # KL: the raw sum within the summed bound, the scaled one exactly one product away, two runs bit-identical
    S = 1 + l.abs() + m * m + torch.exp(l)
    t = -0.5 * (1 + l - m * m - torch.exp(l))
    d_t = 0.5 * U32 * (4 * S + 6 * torch.exp(l))
    ref = float(t.sum())
    d_sum = float(d_t.sum()) + B * L * U64 * float(t.abs().sum())
    d_sum += U32 * (abs(ref) + d_sum)
    raw = kl.cpu()
    print(f"kl[{B}x{L}]: got {float(raw[1]):.9g} ref {ref:.12g} bound {d_sum:.3g} |err|/bound {abs(float(raw[1]) - ref) / d_sum:.3f}")
    assert abs(float(raw[1].double()) - ref) <= d_sum, (float(raw[1]), ref, d_sum)
    assert float(raw[0]) == float(torch.tensor(igb, dtype=torch.float32) * raw[1])
    assert torch.equal(kl[:2], kl2[:2]) and torch.equal(a_z.base[:, 0, 0, :L], a_z2.base[:, 0, 0, :L])
    assert float(raw[2]) == -1.0 and float(raw[3]) == -1.0            # two floats are written, no more
    # backward
    bm = igb * m
    SC.check(got(a_dmu), g + bm, 2 * U32 * (g.abs() + bm.abs()), "dmu", kernel="vae_sample_kl_bwd")
    a = g * 0.5 * ee
    b = igb * 0.5 * (torch.exp(l) - 1.0)
    SC.check(got(a_dlv), a + b, U32 * (9 * a.abs() + 5 * igb * (torch.exp(l) + 1.0)), "dlv", kernel="vae_sample_kl_bwd")
    # and the formulas are the gradients of <dz, z> + KL / gb (autograd on the restatement, fp64)
    mq, lq = m.clone().requires_grad_(True), l.clone().requires_grad_(True)
    obj = (V.sample(mq, lq, e) * g).sum() + igb * V.kl_elements(mq, lq).sum()
    gm, gl = torch.autograd.grad(obj, (mq, lq))
    assert float((gm - (g + bm)).abs().max()) <= 1e-12 * float(gm.abs().max())
    assert float((gl - (a + b)).abs().max()) <= 1e-12 * float(gl.abs().max())


def test_loss_add_is_one_fp32_addition(U):
    kl = torch.tensor([0.375, 9.0, 0.0, 0.0], device=DEV)
    loss = torch.tensor([1.25, 2.0, 3.0, 4.0], device=DEV)
    U.ops.vae_loss_add(kl, loss)
    torch.cuda.synchronize()
    assert loss.cpu().tolist() == [1.625, 2.0, 3.0, 4.0]


# ----------------------------------------------------------------------------------------------------------------------
# the normal draw: a fixed function of (seed, draw, index)
# ----------------------------------------------------------------------------------------------------------------------
GOLD = np.uint64(0x9E3779B97F4A7C15)
TAG = np.uint64(0x4E4F524D414C3634)


def mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def normal_bits(n, seed, draw):
    """The recipe of include/unetrir.h (unetrir_normal_f32) in NumPy uint64 arithmetic: the two 24-bit integers of every element."""
    with np.errstate(over="ignore"):
        key = mix64(mix64(np.uint64(seed) * GOLD + np.uint64(draw)) ^ TAG)
        r = mix64(key + GOLD * np.arange(1, n + 1, dtype=np.uint64))
    return (r >> np.uint64(40)).astype(np.int64), ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.int64)


def test_normal_draw_equals_its_restatement(U):
    """The uniforms are those of the restated recipe: every value lies within the fp32 evaluation bound (module docstring) of fp64
    Box-Muller on the restated bits - a band of 20 ulp of a float pins the 24-bit integers - and where the bits decide the value
    outright they do: the sign is the quadrant of u2, a zero of the cosine (u2 = 1/4, 3/4) or u1 = 1 gives exactly 0."""
    ops = U.ops
    n = 2 ** 20
    seen = []
    for seed in (0, 12345, 2 ** 63 + 11):
        for draw in (0, 1, 7):
            out = torch.full((n,), 99.0, device=DEV)
            ops.normal(out, seed, draw)
            state = torch.tensor([0, 0, draw - 1 if draw else 0], dtype=torch.int64, device=DEV)
            dev = torch.full((n,), 99.0, device=DEV)
            ops.normal_dev(dev, seed, state, 1 if draw else 0)          # draw number = state[2] + offset
            short = torch.full((1000 + 3,), 99.0, device=DEV)
            ops.normal(short[:1000], seed, draw)
            torch.cuda.synchronize()
            assert torch.equal(dev, out)                                 # the _dev form is the same draw
            assert torch.equal(short[:1000], out[:1000]) and float(short[1000:].min()) == 99.0       # a prefix, and no more written
            a, b = normal_bits(n, seed, draw)
            u1 = (a + 1).astype(np.float64) / 2.0 ** 24
            u2 = b.astype(np.float64) / 2.0 ** 24
            s = np.sqrt(-2.0 * np.log(u1))
            ref = torch.from_numpy(s * np.cos(2.0 * np.pi * u2))
            d = 20 * U32 * ref.abs() + 16 * U64 * torch.from_numpy(s)
            got = out.cpu()
            SC.check(got, ref, d, f"normal seed {seed} draw {draw}", kernel="normal")
            gn = got.numpy()
            q1, q3 = 2 ** 22, 3 * 2 ** 22
            zero = (b == q1) | (b == q3) | (a + 1 == 2 ** 24)
            assert np.all(gn[zero] == 0.0)
            assert np.all(gn[~zero & ((b < q1) | (b > q3))] > 0) and np.all(gn[~zero & (b > q1) & (b < q3)] < 0)
            # n = 2^20 values: five-sigma sampling bounds of the moments, and the recipe's own ceiling (u1 = 2^-24)
            g64 = gn.astype(np.float64)
            mean, var = g64.mean(), g64.var()
            print(f"normal seed {seed} draw {draw}: mean {mean:+.3e} (bound {5 / math.sqrt(n):.3e}) var-1 {var - 1:+.3e} "
                  f"(bound {5 * math.sqrt(2 / n):.3e}) max|x| {np.abs(g64).max():.4f}")
            assert abs(mean) <= 5 / math.sqrt(n)
            assert abs(var - 1) <= 5 * math.sqrt(2 / n)
            assert np.abs(g64).max() <= math.sqrt(48 * math.log(2)) * (1 + 20 * U32)
            seen.append(gn)
    for i in range(len(seen)):
        for j in range(i):
            assert not np.array_equal(seen[i], seen[j]), "different (seed, draw) pairs give different draws"
    # the key is not the mask's: for the same (seed, draw) the noise's hashes are not the hashes the keep mask is cut from
    with np.errstate(over="ignore"):
        k_mask = mix64(np.uint64(12345) * GOLD + np.uint64(7))
        r_mask = mix64(k_mask + GOLD * np.arange(1, 4097, dtype=np.uint64))
    a, _ = normal_bits(4096, 12345, 7)
    assert float(np.mean((r_mask >> np.uint64(40)).astype(np.int64) == a)) < 0.01
    with pytest.raises(U._lib.UnetrirError):
        ops.normal(torch.zeros(0, device=DEV), 1, 0)


# ----------------------------------------------------------------------------------------------------------------------
# the whole network against tests/vae_ref.py
# ----------------------------------------------------------------------------------------------------------------------
def _net_case(H, W, filters, B, latent, nn, dropout):
    cfg = V.VAEConfig(H, W, filters, (3,) * len(filters), (2,) * len(filters), latent, nn)
    Pn = V.init_params(cfg, randomize_all=True, dtype=np.float64)
    batch = R.synthetic_batch(R.Config(H, W), B)
    h, w, c = cfg.bottleneck_shape()
    eps = np.random.RandomState(7).standard_normal((B, latent))
    md = (detrand.uniform("vae-md", (B, h * w * c)) >= 0.3).astype(np.float64) / 0.7 if dropout else None
    return cfg, Pn, batch, eps, md


@pytest.mark.parametrize("H,W,filters,B,latent,nn,do", [(32, 32, (8, 8, 16, 16), 2, 8, 16, False),
                                                         (64, 48, (8, 16, 32, 64), 2, 32, 64, True)])
def test_vae_forward_backward_vs_vae_ref(U, H, W, filters, B, latent, nn, do):
    """The fp32 criteria of the autoencoder family (tests/test_resae_gpu.py): prediction 1e-4 absolute, loss 1e-5 relative, every
    gradient 1e-3 of its own largest entry plus the floor."""
    cfg, Pn, (spec_in, emb, spec_out), eps, md = _net_case(H, W, filters, B, latent, nn, do)
    inter = {}
    loss, dl, kl, pred, grads = V.loss_and_grads(Pn, spec_in, emb, spec_out, cfg, eps, 0.9, B, md, inter=inter)
    eng = U.VAEEngine(H, W, B, filters, cfg.conv_kernels, cfg.conv_strides, latent, nn, device=DEV)
    eng.load_keras_params(Pn)
    t = lambda a, dt=None: None if a is None else torch.tensor(a, dtype=dt).to(DEV)
    eng.masks["eps"] = t(eps, torch.float32)
    eng.forward(t(spec_in), t(emb), dropout_mask=t(md, torch.float32), target=t(spec_out), global_batch=B)
    eng.backward()
    eng.reg_loss()
    torch.cuda.synchronize()
    assert eng.l2_names == [] and float(eng.reg_out[0]) == 0.0
    assert float((eng.pred.double().cpu() - pred).abs().max()) <= 1e-4
    got = float(eng.loss_out[0]) + float(eng.reg_out[0])
    print(f"vae {H}x{W}: loss {got:.8g} ref {loss:.8g}; kl {float(eng.kl_out[0]):.8g} ref {kl:.8g}; data ref {dl:.8g}")
    assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
    assert abs(float(eng.kl_out[0]) - kl) <= 1e-5 * abs(kl), (float(eng.kl_out[0]), kl)
    assert abs(float(eng.kl_out[1]) - kl * B) <= 1e-5 * abs(kl * B)
    for node, key in ((eng._latent, "z"), (eng._mu, "mu"), (eng._lv, "log_var")):
        ref = inter[key]
        assert float((node.a.base.view(B, latent).double().cpu() - ref).abs().max()) <= 1e-4 * float(ref.abs().max()), key
    kg = eng.export_keras_grads()
    assert set(kg) == set(grads) == set(V.param_shapes(cfg))
    floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
    for n, g_ref in grads.items():
        e = float((kg[n].double() - g_ref).abs().max())
        # biases in front of a BatchNorm: analytically zero gradient (the product writes an exact 0)
        assert e <= 1e-3 * float(g_ref.abs().max()) + floor, (n, e, float(g_ref.abs().max()))
    # ten steps of Adam move the loss down and keep the padded weights at zero
    for _ in range(10):
        eng.adam_step(1e-3)
        eng.forward(t(spec_in), t(emb), dropout_mask=t(md, torch.float32), target=t(spec_out), global_batch=B)
        eng.backward()
    torch.cuda.synchronize()
    assert float(eng.loss_out[0]) < got
    assert float(eng.p["encoder_conv_layer_1.kernel"][..., 2:].abs().max()) == 0.0
    assert float(eng.p[f"decoder_out_{len(filters)}.kernel"][..., 2:].abs().max()) == 0.0


def test_vae_bf16_against_storage_emulation_and_exact_gradients(U):
    """bf16 storage by the criterion of tests/test_graph_bf16_gpu.py: the same product graph on the simulated runtime with the fp64
    stand-ins (tests/vae_cpu_ops.py) IS the storage model; the HIP path must be as close to the exact fp64 result as it is."""
    import vae_cpu_ops
    from sim_runtime import SimRuntime
    H = W = 64
    B = 4
    cfg = V.VAEConfig(H, W, (8, 16, 16, 32), (3, 3, 3, 3), (2, 2, 2, 2), 8, 16)
    params = V.init_params(cfg, randomize_all=True, dtype=np.float64)
    batch = R.synthetic_batch(R.Config(H, W), B)
    eps = np.random.RandomState(9).standard_normal((B, 8)).astype(np.float32)
    make = lambda **kw: U.VAEEngine(H, W, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                                    dtype="bf16", **kw)

    def run(eng, dev):
        eng.load_keras_params(params)
        t = lambda a: torch.tensor(a).to(dev)
        eng.masks["eps"] = t(eps)
        eng.forward(t(batch[0]), t(batch[1]), target=t(batch[2]), global_batch=B)
        eng.backward()
        return (eng.pred.double().cpu().clone(), float(eng.loss_out[0]), float(eng.kl_out[0]),
                {k: v.double() for k, v in eng.export_keras_grads().items()})

    mp = pytest.MonkeyPatch()
    try:
        rt = SimRuntime()
        vae_cpu_ops.install(mp, rt)
        pred_q, loss_q, kl_q, g_q = run(make(device="cpu", runtime=rt), "cpu")
    finally:
        mp.undo()
    pred_h, loss_h, kl_h, g_h = run(make(device=DEV), DEV)
    torch.cuda.synchronize()
    loss_x, _, kl_x, pred_x, g_x = V.loss_and_grads(params, *batch, cfg, eps, 0.9, B)
    nx = float(pred_x.norm())
    e_h, e_q = float((pred_h - pred_x).norm()) / nx, float((pred_q - pred_x).norm()) / nx
    print(f"vae bf16: pred rel L2 error hip {e_h:.2e} emulation {e_q:.2e}; max |hip - emulation| {float((pred_h - pred_q).abs().max()):.2e}; "
          f"loss hip {loss_h:.6f} emulation {loss_q:.6f} exact {loss_x:.6f}; kl hip {kl_h:.6f} emulation {kl_q:.6f} exact {kl_x:.6f}")
    assert e_h <= 2.0 * e_q + 0.01, (e_h, e_q)
    assert float((pred_h - pred_q).abs().max()) <= 0.15
    assert abs(loss_h - loss_x) <= 2.0 * abs(loss_q - loss_x) + 1e-2 * abs(loss_x), (loss_h, loss_q, loss_x)
    assert abs(kl_h - kl_x) <= 2.0 * abs(kl_q - kl_x) + 1e-2 * abs(kl_x), (kl_h, kl_q, kl_x)
    checked = 0
    gmax = max(float(g.abs().max()) for g in g_x.values())
    for n, gx in g_x.items():
        if float(gx.abs().max()) < 1e-6 * gmax:
            continue                               # analytically zero (biases in front of a BatchNorm)
        nx = float(gx.norm()) + 1e-30
        e_h = float((g_h[n] - gx).norm()) / nx
        e_q = float((g_q[n] - gx).norm()) / nx
        assert e_h <= 2.0 * e_q + 0.03, (n, e_h, e_q)
        checked += 1
    assert checked > 20


# ----------------------------------------------------------------------------------------------------------------------
# step machinery: draws, HIP-graph replay, checkpoints
# ----------------------------------------------------------------------------------------------------------------------
HS = WS = 64
BS = 4


def _engine(U, dtype="f32", overlap=False):
    eng = U.VAEEngine(HS, WS, BS, (8, 16, 32, 64), (3, 3, 3, 3), (2, 2, 2, 2), 32, 64, device=DEV, dtype=dtype, overlap_wgrad=overlap)
    g = torch.Generator(); g.manual_seed(3)
    eng.reset_parameters(g)
    eng.dropout_seed = 77
    return eng


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((BS, 2, HS, WS), generator=gen).to(DEV), torch.randint(26, 1282, (BS, 2, 16), generator=gen).to(DEV),
             torch.rand((BS, 2, HS, WS), generator=gen).to(DEV)) for _ in range(n)]


def _state(eng):
    return (eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}, eng.adam_t,
            eng._shared["dropout_step"])


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_eager_step_with_own_draws_is_reproducible(U, dtype, overlap):
    data = _batches(3)
    res = []
    for _ in range(2):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng._latent.a.base.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 3 * 2                        # a mask and an eps per step
    assert all(math.isfinite(x) for x in res[0][0])


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_graph_replay_is_the_same_step(U, dtype, overlap):
    """Three steps: the captured step and the same launches issued one by one (counters in device memory for both) end bit-identical,
    parameter for parameter - so every replay drew the eps and the mask the eager step drew."""
    data = _batches(3)
    res = []
    for mode in ("graph", "eager_dev"):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10, graph=(mode == "graph"))
        if mode == "eager_dev":
            eng.use_device_counters(True)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        if mode == "graph":
            assert set(tr._graphs) == {True}
        res.append((losses, _state(eng), eng._latent.a.base.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2])
    _same(res[0][1], res[1][1])
    for n, s_ in eng.specs.items():                      # parameter for parameter
        sl = slice(s_.offset, s_.offset + s_.numel)
        assert torch.equal(res[0][1][0][sl], res[1][1][0][sl]), n


@pytest.mark.parametrize("graph,dropout", [(True, True), (False, False), (True, False)])
def test_every_step_draws_new_noise(U, graph, dropout):
    """lr = 0 keeps the variables and the batch statistics are the batch's own, so on the SAME inputs the means repeat bit for bit
    while z moves: what changes is eps alone - under replay of one captured graph, and with Dropout switched off in the trainer."""
    (a, e, b), = _batches(1)
    eng = _engine(U)
    tr = U.Trainer(eng, lr=0.0, graph=graph, dropout=dropout)
    zs, mus = [], []
    for _ in range(3):
        tr.step(a, e, b)
        torch.cuda.synchronize()
        zs.append(eng._latent.a.base.clone()); mus.append(eng._mu.a.base.clone())
    if graph:
        assert len(tr._graphs) == 1
    assert torch.equal(mus[0], mus[1]) and torch.equal(mus[1], mus[2])
    assert not torch.equal(zs[0], zs[1]) and not torch.equal(zs[1], zs[2]) and not torch.equal(zs[0], zs[2])
    assert eng._shared["dropout_step"] == 3 * (2 if dropout else 1)


@pytest.mark.parametrize("graph", [False, True])
def test_checkpoint_resumes_the_noise_sequence(U, tmp_path, graph):
    """Four steps == two steps + checkpoint + restore into a fresh engine + two steps, bit for bit."""
    data = _batches(4)
    e0 = _engine(U)
    t0 = U.Trainer(e0, lr=1e-3, graph=graph)
    for a, e, b in data:
        t0.step(a, e, b)
    torch.cuda.synchronize()
    e1 = _engine(U)
    t1 = U.Trainer(e1, lr=1e-3, graph=graph)
    for a, e, b in data[:2]:
        t1.step(a, e, b)
    path = U.CheckpointManager(t1, str(tmp_path)).save(epoch=0)
    e2 = _engine(U)
    e2.dropout_seed = 5          # overwritten by the checkpoint
    t2 = U.Trainer(e2, lr=1e-3, graph=graph)
    U.CheckpointManager(t2, str(tmp_path)).restore(path)
    assert e2._shared["dropout_step"] == 4 and e2.dropout_seed == 77
    for a, e, b in data[2:]:
        t2.step(a, e, b)
    torch.cuda.synchronize()
    _same(_state(e0), _state(e2))
    assert torch.equal(e0._latent.a.base, e2._latent.a.base)


def test_fit_reports_the_kl_metric(U):
    (a, e, b), = _batches(1)
    eng = _engine(U)
    tr = U.Trainer(eng, lr=0.0, dropout=False)
    eng.masks["eps"] = torch.zeros((BS, 32), device=DEV)
    rec = U.fit(tr, lambda ep: [(a, e, b)] * 2, 1, val_batches=lambda ep: [(a, e, b)], log=None)[0]
    torch.cuda.synchronize()
    mu, lv = eng._mu.a.base.view(BS, 32).double().cpu(), eng._lv.a.base.view(BS, 32).double().cpu()
    want = float(V.kl_elements(mu, lv).mean())
    assert abs(rec["train_kl"] - want) <= 1e-5 * want and abs(rec["val_kl"] - want) <= 1e-5 * want


# ----------------------------------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------------------------------
def test_vae_module_surface(U, tmp_path):
    H, W, B, L = 64, 48, 2, 16
    model = U.VAE(input_shape=(H, W, 2), inf_vector_shape=(2, 16), conv_filters=(8, 16, 32, 64), conv_kernels=(3, 3, 3, 3),
                  conv_strides=(2, 2, 2, 2), latent_space_dim=L, n_neurons=32, name="vae", batch_size=B, device=DEV)
    assert model.reconstruction_loss_weight == 100000 and model.name == "vae"
    gen = torch.Generator(); gen.manual_seed(2)
    spec = torch.rand((B, H, W, 2), generator=gen).to(DEV)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV)
    eps = torch.randn((B, L), generator=gen).to(DEV)
    model.engine.masks["eps"] = eps
    z, mean, log_var = model.encoder([spec, emb], training=True)
    torch.cuda.synchronize()
    assert z.shape == mean.shape == log_var.shape == (B, L)
    ref = torch.exp(0.5 * log_var.double()) * eps.double()
    assert float(((z.double() - mean.double()) - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-6 * float(mean.abs().max())
    pred = model.decoder(z)
    assert tuple(pred.shape) == (B, H, W, 2) and bool(torch.isfinite(pred).all())
    with torch.no_grad():
        out = model.model([spec, emb], training=False).clone()
    assert tuple(out.shape) == (B, H, W, 2) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    with pytest.raises(NotImplementedError):
        model.model([spec, emb], training=True)              # grad mode: the bridge cannot carry the KL gradient
    with pytest.raises(NotImplementedError):
        model.compile_and_fit(None, None, None, None, None, None, 2, 1, 1)
    # save / load round trip (parameters.pkl as dl_models/vae.py:229-246 writes it)
    model.save(str(tmp_path))
    import pickle
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [(H, W, 2), (2, 16), (8, 16, 32, 64), (3, 3, 3, 3), (2, 2, 2, 2), L, 32]
    again = U.VAE.load(str(tmp_path), batch_size=B, device=DEV)
    assert torch.equal(again.engine.theta, model.engine.theta)
    again.engine.masks["eps"] = eps
    with torch.no_grad():
        out2 = again.model([spec, emb], training=False)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    # without a supplied eps the generation samples (vae.py:34-39 has no `training` switch)
    model.engine.masks["eps"] = None
    with torch.no_grad():
        o1 = model.model([spec, emb], training=False).clone()
        o2 = model.model([spec, emb], training=False).clone()
    assert not torch.equal(o1, o2)
    # Evaluator needs nothing VAE-specific
    T, H2, W2 = 320, 32, 48
    m2 = U.VAE((H2, W2, 2), (2, 16), (8, 16), (3, 3), (2, 2), 8, 16, batch_size=B, device=DEV, dropout=False)
    ev = U.Evaluator(m2, n50=80, n_fft=32, win_length=16, hop_length=8, des_shape=(17, 41))
    x = torch.rand((B, 2, H2, W2), generator=gen).to(DEV)
    y = torch.rand((B, 2, H2, W2), generator=gen).to(DEV)
    ev.update(x, emb, y, (torch.rand((B, T), generator=gen) * 2e-2 - 1e-2).to(DEV), ["ShoeBoxRoom", "LargeMeetingRoom"])
    res = ev.result()
    assert res["n"][0] == B and all(math.isfinite(res[m][0]) for m in ("mse_spec", "mse_amp", "phase", "mse_wav"))
