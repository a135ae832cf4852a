"""The VQ-VAE on the GPU: the quantiser kernels of csrc/vq.hip against fp64 (indices by margin, everything else GIVEN the kernel's
own indices, by the method of tests/streaming_check.py), integer data with forced ties, the whole network against
tests/vqvae_ref.py, the step machinery (determinism, HIP-graph replay, checkpoint resume, inference) and the module surface.
PARITY UNPINNED: the reference here is a restatement of dl_models/vqvae.py (tests/vqvae_ref.py, pinned by tests/test_vqvae_ref.py).

Bounds (U32 = 2^-24, U64 = 2^-53; k fp32 roundings of an expression give k * U32 * S, S the sum of the absolute values of its terms).

  indices  The kernel minimises dist_k = fl(n_k - 2 s_k) (include/unetrir.h): s_k = x . E_k by D fmas in order (|error| <=
           D U32 sum_d |x_d E_dk| <= D U32 |x| |E_k|, Cauchy-Schwarz), n_k = |E_k|^2 the same way (<= D U32 |E_k|^2), one more
           rounding for the final fma (<= U32 (|E_k|^2 + 2 |x| |E_k|)).  Against the exact |E_k|^2 - 2 x . E_k - which orders
           the codes as the reference's distances do, |x|^2 being the same for every code - the error is at most
           (D + 1) U32 (|E_k|^2 + 2 |x| |E_k|) <= (D + 1) U32 (|x| + |E|max)^2 to first order.
           BOUND = 2 (D + 4) U32 (|x| + |E|max)^2 is more than twice that.  A vector is DECIDED when the fp64 margin between its
           best and second-best code exceeds 2 BOUND: its index must equal the fp64 argmin.  Any vector's chosen code has an fp64
           distance within BOUND of the minimum (two errors of at most BOUND / 2 each).  At most 1 % of a case's vectors may be
           undecided: asserted from the reference alone, before the kernel's indices are looked at.
  y        = fl(x + fl(E[:, idx] - x)): two IEEE operations on given numbers - equality with NumPy fp32.
  S        vq_out[1] = (float) of the fp64 sum of fl(fl(q - x)^2): 3 roundings per addend (the difference enters squared: 2, the
           square: 1), N fp64 additions, one conversion: d = 3 U32 S + N U64 S + U32 (S + 3 U32 S).  vq_out[0] is ONE fp32 product
           of vq_out[1] with (float)(r (1 + beta) / N): equality.
  dx       = fmaf(cdx, fl(x - q), dy): the difference and the fma, the first scaled by cdx: d = U32 (|dy| + 3 |cdx (x - q)|).
  dE[:,k]  = fl(cde * sum_{n_k matches} fl(q - x)): n_k roundings of addends, n_k - 1 fp32 additions in any order (each on a
           partial sum <= sum |addend|), one product: d = |cde| U32 1.01 (2 n_k + 1) sum |q - x|.  Codes nobody chose: exactly 0.
"""
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exact_data as X  # noqa: E402
import streaming_check as SC  # noqa: E402
import vqvae_ref as Q  # noqa: E402
from oracle import detrand, torch_ref as R  # noqa: E402
from streaming_check import U32, U64  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D64 = torch.float64
BETA = Q.BETA
CAP = 0.01


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    return unet_rir_amd


# ----------------------------------------------------------------------------------------------------------------------
# the quantiser kernels
# ----------------------------------------------------------------------------------------------------------------------
def _strided(U, x, ld):
    """[rows, C] values in an Act with pixel stride ld (the padding holds NaNs: nothing may read or count it)."""
    rows, C = x.shape
    base = torch.full((1, 1, rows, ld), float("nan"), dtype=torch.float32, device=DEV)
    base[0, 0, :, :C] = x.to(DEV)
    return U.ops.Act(base, 0, C)


def _data(rows, C, Dv, K):
    g = torch.Generator().manual_seed(1000 * rows + 10 * C + Dv + K)
    x = torch.rand((rows, C), generator=g) * 0.4 - 0.2                  # U(-0.2, 0.2)
    E = torch.rand((Dv, K), generator=g) * 0.1 - 0.05                   # U(-0.05, 0.05): tf.random_uniform_initializer()
    dy = torch.randn((rows, C), generator=g) * 0.1
    return x, E, dy


def _run(U, x, E, dy, ld, Dv, r):
    """One forward + backward of the layer on strided buffers: every output as a CPU tensor, the padding checked."""
    ops = U.ops
    rows, C = x.shape
    a_x, a_dy = _strided(U, x, ld), _strided(U, dy, ld)
    a_y, a_dx = _strided(U, torch.zeros(rows, C), ld), _strided(U, torch.zeros(rows, C), ld)
    E_d = E.to(DEV).contiguous()
    idx = torch.full((rows * C // Dv,), -7, dtype=torch.int32, device=DEV)
    out = torch.full((4,), -1.0, device=DEV)
    dE = torch.full_like(E_d, float("nan"))                            # written, never accumulated
    ws = ops.vq_workspace(DEV)
    ops.vq_fwd(a_x, Dv, E_d, BETA, r, idx, a_y, out, ws)
    ops.vq_bwd(a_x, Dv, idx, E_d, a_dy, BETA, r, a_dx, dE)
    torch.cuda.synchronize()
    for a in (a_y, a_dx):
        if ld > C:
            assert bool(torch.isnan(a.base[0, 0, :, C:]).all())
    assert int(ws[:16].max()) == 0                                     # the arrival counter is left at zero
    assert float(out[2]) == -1.0 and float(out[3]) == -1.0             # two floats are written, no more
    got = lambda a: a.base[0, 0, :, :C].cpu()
    return dict(idx=idx.cpu(), y=got(a_y), vq=out[:2].cpu(), dx=got(a_dx), dE=dE.cpu())


def _check_indices(x, E, idx, Dv, what):
    """The module docstring's index criterion.  x [rows, C] fp32 (CPU), E [D, K] fp32, idx int32.  Returns the undecided share."""
    flat, E64 = x.double().reshape(-1, Dv), E.double()
    dist = Q.distances(flat, E64)
    two = torch.topk(dist, 2, dim=1, largest=False)
    bound = 2 * (Dv + 4) * U32 * (flat.norm(dim=1) + E64.norm(dim=0).max()) ** 2
    decided = (two.values[:, 1] - two.values[:, 0]) > 2 * bound
    share = 1.0 - float(decided.double().mean())
    assert share <= CAP, f"{what}: {share:.3%} of the vectors are undecided (cap {CAP:.0%})"          # from the reference alone
    i = idx.long()
    assert int(i.min()) >= 0 and int(i.max()) < E.shape[1], what
    ref = torch.argmin(dist, dim=1)
    bad = int((decided & (i != ref)).sum())
    chosen = dist.gather(1, i[:, None])[:, 0]
    near = chosen - two.values[:, 0] <= bound
    print(f"{what}: {flat.shape[0]} vectors, undecided {share:.4%}, decided-and-wrong {bad}, not near-optimal {int((~near).sum())}, "
          f"codes used {len(set(i.tolist()))} of {E.shape[1]}, differ from fp64 argmin {int((i != ref).sum())}")
    assert bad == 0, f"{what}: {bad} decided vectors with another index than the fp64 argmin"
    assert bool(near.all()), f"{what}: {int((~near).sum())} vectors whose code is not within the bound of the minimum"
    return share


def _check_given_indices(res, x, E, dy, Dv, r, what):
    """y, vq_out, dx, dE against the formulas evaluated with the kernel's OWN indices."""
    rows, C = x.shape
    N, K = rows * C, E.shape[1]
    i = res["idx"].long()
    q32 = E.t()[i].reshape(rows, C).numpy()                             # fp32 gather
    x32 = x.numpy()
    assert np.array_equal(res["y"].numpy(), x32 + (q32 - x32)), what   # NumPy fp32: two roundings, as the kernel's
    q, xd = torch.from_numpy(q32).double(), x.double()
    S = float(((q - xd) ** 2).sum())
    d_S = 3 * U32 * S + N * U64 * S + U32 * (S + 3 * U32 * S)
    raw = res["vq"]
    print(f"{what}: S {float(raw[1]):.9g} ref {S:.12g} |err|/bound {abs(float(raw[1]) - S) / d_S:.3f}")
    assert abs(float(raw[1].double()) - S) <= d_S, (what, float(raw[1]), S, d_S)
    r32 = float(np.float32(r))
    scale = np.float32(r32 * (1.0 + BETA) / float(N))
    assert float(raw[0]) == float(scale * np.float32(raw[1])), what
    cdx = float(np.float32(2.0 * r32 * BETA / float(N)))
    cde = float(np.float32(2.0 * r32 / float(N)))
    t = cdx * (xd - q)
    SC.check(res["dx"], dy.double() + t, U32 * (dy.double().abs() + 3 * t.abs()), f"{what} dx", kernel="vq_bwd_dx")
    diff = (q - xd).reshape(-1, Dv)
    seg, seg_abs = torch.zeros((K, Dv), dtype=D64), torch.zeros((K, Dv), dtype=D64)
    seg.index_add_(0, i, diff)
    seg_abs.index_add_(0, i, diff.abs())
    n_k = torch.bincount(i, minlength=K).double()
    SC.check(res["dE"], (cde * seg).t(), (abs(cde) * U32 * 1.01 * (2 * n_k[:, None] + 1) * seg_abs).t(), f"{what} dE", kernel="vq_bwd_de")
    unused = n_k == 0
    assert bool((res["dE"][:, unused] == 0).all()), what               # exactly 0
    return int((~unused).sum())


CASES = [(3, 8, 8, 4, 4), (37, 24, 28, 8, 12), (90, 256, 256, 16, 256), (5, 128, 132, 64, 512), (1031, 16, 16, 16, 8),
         (131200, 8, 8, 4, 4),          # 262 400 vectors want 1025 workgroups: the grid is capped at 1024 (a second trip of the grid-stride
                                        # loop) and every combining thread adds four partials
         (65600, 64, 68, 64, 8)]        # 257 workgroups; 1 049 600 float4 units: past the 4096-block cap of vq_bwd_dx


@pytest.mark.parametrize("rows,C,ld,Dv,K", CASES)
@pytest.mark.parametrize("r", [1.0, 0.5])
def test_quantiser_kernels(U, rows, C, ld, Dv, K, r):
    what = f"vq[{rows}x{C}/{ld} D{Dv} K{K} r{r}]"
    x, E, dy = _data(rows, C, Dv, K)
    res = _run(U, x, E, dy, ld, Dv, r)
    _check_indices(x, E, res["idx"], Dv, what)
    used = _check_given_indices(res, x, E, dy, Dv, r, what)
    if K <= 256:
        assert used > K // 2, f"{what}: {used} of {K} codes used - the gradient check would be vacuous"
    again = _run(U, x, E, dy, ld, Dv, r)                               # a second run: bit-identical in all five outputs
    for k in ("idx", "y", "vq", "dx", "dE"):
        assert torch.equal(res[k], again[k]), (what, k)


def test_quantiser_loss_term_off(U):
    """r = 0 (backward(include_reg=False)): dx = dy exactly, dE = 0, vq_out[0] = 0 while S is still reported."""
    x, E, dy = _data(37, 24, 8, 12)
    res = _run(U, x, E, dy, 28, 8, 0.0)
    assert torch.equal(res["dx"], dy) and bool((res["dE"] == 0).all()) and float(res["vq"][0]) == 0.0 and float(res["vq"][1]) > 0


def test_quantiser_integer_data_with_ties(U):
    """Values from tests/exact_data.py's ranges: every product and sum is a small integer, exact in fp32 in any order.  Codebook
    columns are duplicated to force ties: the indices equal the reference's everywhere - the lowest duplicate - and dE is exact
    (N = 1024 and r = 1 make cde = 2^-9)."""
    rows, C, Dv, K = 64, 16, 8, 12
    x = X.acts("vq-int-x", (rows, C)).float()
    E = X.kernels("vq-int-E", (Dv, K)).float()
    E[:, 7] = E[:, 2]; E[:, 11] = E[:, 2]; E[:, 9] = E[:, 0]; E[:, 5] = E[:, 4]
    x[:6, :Dv] = E.t()[[7, 11, 2, 9, 5, 4]]                             # vectors that ARE a duplicated code: distance 0, a tie
    dy = X.acts("vq-int-dy", (rows, C)).float()
    res = _run(U, x, E, dy, C, Dv, 1.0)
    ref = Q.code_indices(x.double().reshape(-1, Dv), E.double())
    dist = Q.distances(x.double().reshape(-1, Dv), E.double())
    ties = int(((dist == dist.min(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
    X.note_ties(ties)
    assert ties >= 6
    assert torch.equal(res["idx"].long(), ref)
    assert not bool(torch.isin(res["idx"], torch.tensor([7, 11, 9, 5], dtype=torch.int32)).any())        # never the higher duplicate
    assert res["idx"][0:12:2].tolist() == [2, 2, 2, 0, 4, 4]                # vector 0 of pixels 0 .. 5 (two vectors per pixel)
    _, dE = Q.quantize_grads(x.double(), E.double(), ref, dy.double(), BETA, 1.0)
    X.assert_exact(res["dE"], dE, "vq integer dE")
    q = E.t()[ref].reshape(rows, C)
    assert torch.equal(res["y"], q) and float(res["vq"][1]) == float(((q - x).double() ** 2).sum())


def test_quantiser_at_the_reference_size(U):
    """dl_models/vqvae.py:522-531 at batch 32: 32 x 10 x 9 pixels of 256 channels = 46 080 vectors, K = 256, D = 16."""
    rows, C, Dv, K = 32 * 10 * 9, 256, 16, 256
    x, E, dy = _data(rows, C, Dv, K)
    res = _run(U, x, E, dy, C, Dv, 1.0)
    _check_indices(x, E, res["idx"], Dv, "vq[reference size]")
    q32, x32 = E.t()[res["idx"].long()].reshape(rows, C).numpy(), x.numpy()
    assert np.array_equal(res["y"].numpy(), x32 + (q32 - x32))
    again = _run(U, x, E, dy, C, Dv, 1.0)
    for k in ("idx", "y", "vq", "dx", "dE"):
        assert torch.equal(res[k], again[k]), k


# ----------------------------------------------------------------------------------------------------------------------
# the whole network against tests/vqvae_ref.py
# ----------------------------------------------------------------------------------------------------------------------
NH, NW, NB = 32, 48, 3
NCFG = Q.VQVAEConfig(NH, NW, (4, 8, 8, 16), (3, 3, 3, 3), (2, 2, 2, 2), 4, 8)
# bf16 storage holds activations in 16-byte channel granules - 8 channels - in every engine of this project (ops.Act refuses
# anything else), so a first level of 4 filters cannot be built in bf16: the bf16 comparison runs at the nearest size it can hold,
# first level 8, everything else as above
NCFG16 = Q.VQVAEConfig(NH, NW, (8, 8, 8, 16), (3, 3, 3, 3), (2, 2, 2, 2), 4, 8)


def _net_case(cfg):
    params = Q.init_params(cfg, randomize_all=True, dtype=np.float64, codebook_scale=8.0)
    spec_in, emb, spec_out = R.synthetic_batch(R.Config(NH, NW), NB)
    h, w, c = cfg.bottleneck_shape()
    mask = (detrand.uniform("vq-mask", (NB, h * w * 2)) >= 0.3).astype(np.float64) / 0.7
    return params, (spec_in, emb % Q.VOCAB, spec_out), mask


@pytest.fixture(scope="module")
def net_case():
    return _net_case(NCFG)


@pytest.fixture(scope="module")
def net_case16():
    return _net_case(NCFG16)


def _make(U, dtype="f32", n_replicas=1, B=NB, cfg=NCFG, **kw):
    return U.VQVAEEngine(NH, NW, B, cfg.conv_filters, cfg.conv_kernels, cfg.conv_strides, cfg.latent_space_dim, cfg.n_neurons,
                         dtype=dtype, n_replicas=n_replicas, **kw)


def _engine_indices(eng, what):
    """The engine's indices after they have passed the near-optimal check against ITS quantiser input: an index flip cannot
    masquerade as a gradient error in what follows."""
    a = eng._vq_in.a
    x = a.base[..., a.c0:a.c0 + a.C].reshape(-1, a.C).float().cpu()
    idx = eng.vq_indices.cpu()
    _check_indices(x, eng.p[Q.CODEBOOK].float().cpu(), idx, NCFG.latent_space_dim, what)
    return idx


@pytest.mark.parametrize("n_replicas", [1, 2])
def test_vqvae_forward_backward_vs_vqvae_ref(U, net_case, n_replicas):
    """The fp32 criteria of tests/test_vae_gpu.py: prediction 1e-4 absolute, loss 1e-5 relative, every gradient 1e-3 of its own
    largest entry plus the floor."""
    params, (spec_in, emb, spec_out), mask = net_case
    gb = NB * n_replicas
    eng = _make(U, n_replicas=n_replicas, device=DEV)
    eng.load_keras_params(params)
    t = lambda a, dt=None: None if a is None else torch.tensor(a, dtype=dt).to(DEV)
    m = t(mask, torch.float32).view(NB, 1, 1, -1)
    eng.forward(t(spec_in), t(emb), dropout_mask=m, target=t(spec_out), global_batch=gb)
    eng.backward()
    eng.reg_loss()
    torch.cuda.synchronize()
    idx = _engine_indices(eng, f"net f32 r{n_replicas}")
    assert len(set(idx.tolist())) > 1
    inter = {}
    loss, dl, term, pred, grads = Q.loss_and_grads(params, spec_in, emb, spec_out, NCFG, 0.9, gb, mask, n_replicas, idx, inter=inter)
    assert eng.l2_names == [] and float(eng.reg_out[0]) == 0.0
    assert float((eng.pred.double().cpu() - pred).abs().max()) <= 1e-4
    got = float(eng.loss_out[0]) + float(eng.reg_out[0])
    print(f"vqvae r{n_replicas}: loss {got:.8g} ref {loss:.8g}; vq {float(eng.vq_out[0]):.8g} ref {term:.8g}; data ref {dl:.8g}")
    assert abs(got - loss) <= 1e-5 * abs(loss), (got, loss)
    assert abs(float(eng.vq_out[0]) - term) <= 1e-5 * abs(term), (float(eng.vq_out[0]), term)
    ref_y = inter["y"]
    assert float((eng._latent.a.base.double().cpu() - ref_y).abs().max()) <= 1e-4 * float(ref_y.abs().max())
    kg = eng.export_keras_grads()
    assert set(kg) == set(grads) == set(Q.param_shapes(NCFG))
    floor = 1e-6 * max(float(g.abs().max()) for g in grads.values())
    for n, g_ref in grads.items():
        e = float((kg[n].double() - g_ref).abs().max())
        assert e <= 1e-3 * float(g_ref.abs().max()) + floor, (n, e, float(g_ref.abs().max()))
    assert float(grads[Q.CODEBOOK].abs().max()) > 0 and float(grads["conv2d.kernel"].abs().max()) > 0
    # include_reg=False leaves the term's gradients out: the codebook's gradient is then exactly 0
    eng.forward(t(spec_in), t(emb), dropout_mask=m, target=t(spec_out), global_batch=gb)
    eng.backward(include_reg=False)
    torch.cuda.synchronize()
    assert float(eng.g[Q.CODEBOOK].abs().max()) == 0.0
    # ten steps of Adam move the loss down and keep the padded weights at zero
    for _ in range(10):
        eng.forward(t(spec_in), t(emb), dropout_mask=m, target=t(spec_out), global_batch=gb)
        eng.backward()
        eng.adam_step(1e-3)
    eng.forward(t(spec_in), t(emb), dropout_mask=m, target=t(spec_out), global_batch=gb)
    torch.cuda.synchronize()
    assert float(eng.loss_out[0]) < got
    assert float(eng.p["encoder_conv_layer_1.kernel"][..., 2:].abs().max()) == 0.0
    assert float(eng.p["conv2d.kernel"][..., 2:].abs().max()) == 0.0


@pytest.mark.parametrize("n_replicas", [1, 2])
def test_vqvae_bf16_against_storage_emulation_and_exact_gradients(U, net_case16, n_replicas):
    """bf16 storage by the criterion of tests/test_vae_gpu.py: the same product graph on the simulated runtime with the fp64
    stand-ins (tests/vqvae_cpu_ops.py) IS the storage model; the HIP path must be as close to the exact fp64 result as it is.
    Both the emulation and the exact reference take the HIP engine's indices (after the near-optimal check)."""
    import vqvae_cpu_ops
    from sim_runtime import SimRuntime
    params, batch, mask = net_case16
    gb = NB * n_replicas

    def run(eng, dev):
        eng.load_keras_params(params)
        t = lambda a: torch.tensor(a).to(dev)
        eng.forward(t(batch[0]), t(batch[1]), dropout_mask=t(mask).float().view(NB, 1, 1, -1), target=t(batch[2]), global_batch=gb)
        eng.backward()
        return (eng.pred.double().cpu().clone(), float(eng.loss_out[0]), float(eng.vq_out[0]),
                {k: v.double() for k, v in eng.export_keras_grads().items()})

    hip = _make(U, "bf16", n_replicas, cfg=NCFG16, device=DEV)
    pred_h, loss_h, vq_h, g_h = run(hip, DEV)
    torch.cuda.synchronize()
    idx = _engine_indices(hip, f"net bf16 r{n_replicas}")
    mp = pytest.MonkeyPatch()
    try:
        rt = SimRuntime()
        impl = vqvae_cpu_ops.install(mp, rt)
        impl.vq.indices = idx
        pred_q, loss_q, vq_q, g_q = run(_make(U, "bf16", n_replicas, cfg=NCFG16, device="cpu", runtime=rt), "cpu")
    finally:
        mp.undo()
    loss_x, _, vq_x, pred_x, g_x = Q.loss_and_grads(params, *batch, NCFG16, 0.9, gb, mask, n_replicas, idx)
    nx = float(pred_x.norm())
    e_h, e_q = float((pred_h - pred_x).norm()) / nx, float((pred_q - pred_x).norm()) / nx
    print(f"vqvae bf16 r{n_replicas}: pred rel L2 error hip {e_h:.2e} emulation {e_q:.2e}; loss hip {loss_h:.6f} emulation {loss_q:.6f} "
          f"exact {loss_x:.6f}; vq hip {vq_h:.6g} emulation {vq_q:.6g} exact {vq_x:.6g}")
    assert e_h <= 2.0 * e_q + 0.01, (e_h, e_q)
    assert float((pred_h - pred_q).abs().max()) <= 0.15
    assert abs(loss_h - loss_x) <= 2.0 * abs(loss_q - loss_x) + 1e-2 * abs(loss_x), (loss_h, loss_q, loss_x)
    assert abs(vq_h - vq_x) <= 2.0 * abs(vq_q - vq_x) + 1e-2 * abs(vq_x), (vq_h, vq_q, vq_x)
    checked = 0
    gmax = max(float(g.abs().max()) for g in g_x.values())
    for n, gx in g_x.items():
        if float(gx.abs().max()) < 1e-6 * gmax:
            continue                               # analytically zero (biases in front of a BatchNorm)
        nrm = float(gx.norm()) + 1e-30
        e_h = float((g_h[n] - gx).norm()) / nrm
        e_q = float((g_q[n] - gx).norm()) / nrm
        assert e_h <= 2.0 * e_q + 0.03, (n, e_h, e_q)
        checked += 1
    assert checked > 20


# ----------------------------------------------------------------------------------------------------------------------
# step machinery: determinism, HIP-graph replay, checkpoints, inference
# ----------------------------------------------------------------------------------------------------------------------
def _engine(U, dtype="f32", overlap=False):
    eng = _make(U, dtype, cfg=NCFG if dtype == "f32" else NCFG16, device=DEV, overlap_wgrad=overlap)
    g = torch.Generator(); g.manual_seed(3)
    eng.reset_parameters(g)
    with torch.no_grad():
        eng.p[Q.CODEBOOK].mul_(8.0)              # codes on the scale of what the random 1x1 convolution produces: several are used
    eng.dropout_seed = 77
    return eng


def _batches(n):
    gen = torch.Generator(); gen.manual_seed(5)
    return [(torch.rand((NB, 2, NH, NW), generator=gen).to(DEV), torch.randint(26, 1282, (NB, 2, 16), generator=gen).to(DEV),
             torch.rand((NB, 2, NH, NW), generator=gen).to(DEV)) for _ in range(n)]


def _state(eng):
    return (eng.theta.clone(), eng.adam_m.clone(), eng.adam_v.clone(), {k: v.clone() for k, v in eng.moving.items()}, eng.adam_t,
            eng._shared["dropout_step"])


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k
    assert a[4] == b[4] and a[5] == b[5]


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_three_steps_twice_from_the_same_seed_are_bit_identical(U, dtype, overlap):
    data = _batches(3)
    res = []
    for _ in range(2):
        eng = _engine(U, dtype, overlap)
        tr = U.Trainer(eng, lr=1e-3, bucket_bytes=16 << 10)
        losses = [tr.step(a, e, b, return_loss=True) for a, e, b in data]
        torch.cuda.synchronize()
        res.append((losses, _state(eng), eng._latent.a.base.clone(), eng.vq_indices.clone(), eng.vq_out.clone()))
    assert res[0][0] == res[1][0] and all(torch.equal(res[0][k], res[1][k]) for k in (2, 3, 4))
    _same(res[0][1], res[1][1])
    assert res[0][1][5] == 3                              # one mask per step
    assert all(math.isfinite(x) for x in res[0][0])
    assert len(set(res[0][3].tolist())) > 1


@pytest.mark.parametrize("dtype,overlap", [("f32", False), ("bf16", True)])
def test_graph_replay_is_the_same_step(U, dtype, overlap):
    """Three steps: the captured step and the same launches issued one by one (counters in device memory for both) end
    bit-identical, parameter for parameter - the codebook and its moments included."""
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
        res.append((losses, _state(eng), eng._latent.a.base.clone(), eng.vq_indices.clone()))
    assert res[0][0] == res[1][0] and torch.equal(res[0][2], res[1][2]) and torch.equal(res[0][3], res[1][3])
    _same(res[0][1], res[1][1])
    s_ = eng.specs[Q.CODEBOOK]
    sl = slice(s_.offset, s_.offset + s_.numel)
    assert torch.equal(res[0][1][0][sl], res[1][1][0][sl]) and float(res[0][1][1][sl].abs().max()) > 0


def test_checkpoint_after_step_2_resumes_to_a_bit_identical_step_3(U, tmp_path):
    data = _batches(3)
    e0 = _engine(U)
    t0 = U.Trainer(e0, lr=1e-3)
    for a, e, b in data:
        t0.step(a, e, b)
    torch.cuda.synchronize()
    e1 = _engine(U)
    t1 = U.Trainer(e1, lr=1e-3)
    for a, e, b in data[:2]:
        t1.step(a, e, b)
    path = U.CheckpointManager(t1, str(tmp_path)).save(epoch=0)
    e2 = _make(U, device=DEV)
    e2.reset_parameters(torch.Generator().manual_seed(99))            # other parameters, another codebook: all overwritten
    e2.dropout_seed = 5
    t2 = U.Trainer(e2, lr=1e-3)
    U.CheckpointManager(t2, str(tmp_path)).restore(path)
    assert e2._shared["dropout_step"] == 2 and e2.dropout_seed == 77
    s_ = e2.specs[Q.CODEBOOK]
    sl = slice(s_.offset, s_.offset + s_.numel)
    assert torch.equal(e2.theta[sl], e1.theta[sl]) and torch.equal(e2.adam_m[sl], e1.adam_m[sl]) and torch.equal(e2.adam_v[sl], e1.adam_v[sl])
    assert float(e2.adam_v[sl].abs().max()) > 0
    t2.step(*data[2])
    torch.cuda.synchronize()
    _same(_state(e0), _state(e2))
    assert torch.equal(e0._latent.a.base, e2._latent.a.base) and torch.equal(e0.vq_indices, e2.vq_indices)


def test_inference_quantises_and_uses_the_moving_statistics(U, net_case):
    params, (spec_in, emb, spec_out), mask = net_case
    eng = _make(U, device=DEV)
    eng.load_keras_params(params)
    g = torch.Generator().manual_seed(4)
    for n, b in eng.moving.items():                                     # moving statistics that are not the batch's
        b.copy_((torch.rand(b.shape, generator=g) * 0.5 + (0.75 if n.endswith("variance") else -0.25)).to(DEV))
    moving = {n: b.double().cpu() for n, b in eng.moving.items()}
    t = lambda a: torch.tensor(a).to(DEV)
    eng.training = False
    pred = eng.forward(t(spec_in), t(emb)).double().cpu()
    torch.cuda.synchronize()
    idx = _engine_indices(eng, "net inference")
    y = eng._latent.a.base.float().cpu()
    q = eng.p[Q.CODEBOOK].float().cpu().t()[idx.long()].reshape(y.shape)
    x = eng._vq_in.a.base.float().cpu()
    assert np.array_equal(y.numpy(), x.numpy() + (q.numpy() - x.numpy()))                 # quantised, training or not
    P = {k: torch.tensor(np.asarray(v), dtype=D64) for k, v in params.items()}
    ref, _ = Q.forward(P, torch.tensor(spec_in, dtype=D64), torch.tensor(emb), NCFG, None, idx.long(), moving=moving)
    assert float((pred - ref).abs().max()) <= 1e-4
    for n, b in eng.moving.items():                                     # and the pass did not move them
        assert torch.equal(b.double().cpu(), moving[n]), n


def test_fit_reports_the_vq_metric(U):
    (a, e, b), = _batches(1)
    eng = _engine(U)
    tr = U.Trainer(eng, lr=0.0, dropout=False)
    rec = U.fit(tr, lambda ep: [(a, e, b)] * 2, 1, val_batches=lambda ep: [(a, e, b)], log=None)[0]
    torch.cuda.synchronize()
    want = float(eng.vq_out[1]) / eng.vq_elems
    assert want > 0 and abs(rec["train_vq"] - want) <= 1e-6 * want and abs(rec["val_vq"] - want) <= 1e-6 * want


# ----------------------------------------------------------------------------------------------------------------------
# the module
# ----------------------------------------------------------------------------------------------------------------------
def test_vqvae_module_surface(U, tmp_path):
    import inspect
    sig = inspect.signature(U.VQVAE.__init__)
    assert list(sig.parameters)[1:9] == ["input_shape", "inf_vector_shape", "conv_filters", "conv_kernels", "conv_strides",
                                         "latent_space_dim", "n_neurons", "name"]
    assert sig.parameters["name"].default == "VAE"                      # dl_models/vqvae.py:115
    assert U.VQVAEEngine.DEFAULTS == ((32, 64, 128, 256), 16, 320)
    H, W, B = NH, NW, 2
    model = U.VQVAE(input_shape=(H, W, 2), inf_vector_shape=(2, 16), conv_filters=(4, 8, 8, 16), conv_kernels=(3, 3, 3, 3),
                    conv_strides=(2, 2, 2, 2), latent_space_dim=4, n_neurons=8, batch_size=B, device=DEV)
    assert model.reconstruction_loss_weight == 100000 and model.name == "VAE"
    with torch.no_grad():
        model.engine.p[Q.CODEBOOK].mul_(8.0)
    gen = torch.Generator(); gen.manual_seed(2)
    spec = torch.rand((B, H, W, 2), generator=gen).to(DEV)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=gen).to(DEV)
    y = model.encoder([spec, emb], training=False)
    torch.cuda.synchronize()
    h, w, c = NCFG.bottleneck_shape()
    assert tuple(y.shape) == (B, h, w, c) and tuple(model._shape_before_bottleneck) == (h, w, c)
    pred = model.decoder(y).clone()
    with torch.no_grad():
        out = model.model([spec, emb], training=False).clone()
    assert tuple(out.shape) == (B, H, W, 2) and float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    assert torch.equal(pred, out)                                       # decoder(encoder(.)) IS model(.)
    assert torch.equal(model.predict_stft([spec, emb]).to(DEV), out)
    with pytest.raises(NotImplementedError):
        model.model([spec, emb], training=True)                         # grad mode: the bridge cannot carry the term's gradient
    with pytest.raises(NotImplementedError):
        model.compile_and_fit(None, None, None, None, None, None, 2, 1, 1)
    assert len(model.get_callbacks()) >= 1
    model.save(str(tmp_path))
    with open(tmp_path / "parameters.pkl", "rb") as f:
        assert pickle.load(f) == [(H, W, 2), (2, 16), (4, 8, 8, 16), (3, 3, 3, 3), (2, 2, 2, 2), 4, 8]
    again = U.VQVAE.load(str(tmp_path), batch_size=B, device=DEV)
    assert torch.equal(again.engine.theta, model.engine.theta)
    with torch.no_grad():
        out2 = again.model([spec, emb], training=False)
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
