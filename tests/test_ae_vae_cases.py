"""The case table of tests/test_fullsize_ae_vae_gpu.py (tests/ae_vae_cases.py) IS the set of launches of the engines: AutoencoderEngine
and VAEEngine are built at main_training.py's geometry on the simulated runtime (tests/sim_runtime.py), in both storage modes, with
every operator replaced by a recorder of (operator, geometry); one Trainer step (forward + backward) must issue exactly
`ae_vae_cases.launches(model, dtype)`.  No GPU, no arithmetic.  A layer added to an engine, or dropped from the table, fails here."""
import pytest
import torch

import ae_vae_cases as T

KEEP = ("_elems", "_supported", "_rows", "_ws_bytes", "_table")       # queries whose simulated answer the engines use


def _recorders(seen):
    def geo(g):
        return (g.B, g.H, g.W, g.Cin, g.Cout, g.k, g.stride)

    def conv(name):
        def rec(g, x, *a, addend=None, **k):
            if name == "conv2d_dgrad" and (addend is not None or (len(a) > 2 and a[2] is not None)):
                seen.add(("conv2d_dgrad_addend", x.sfx) + geo(g))
            else:
                seen.add((name, x.sfx) + geo(g))
        return rec

    def dense_fwd(x, w, bias, y, ws):
        seen.add(("dense_fwd", x.P, x.C, y.C, bias is not None))

    def transpose_weight(w, wt, N, T_, C_):
        seen.add(("transpose_weight", N, T_, C_))

    def colsum(x, out, ws):
        seen.add(("colsum", x.sfx, x.P, x.C))

    def bn_act_add(x, affine, y, act=2, addend=None):
        assert affine is not None and addend is None
        seen.add(("bn_act", x.sfx, x.C, x.P, act))

    def bn_bwd(da, x, gamma, affine, saved, dx, dgamma, dbeta, ws, relu=True):
        seen.add(("bn_bwd", x.sfx, x.C, x.P, int(relu)))

    out = {n: conv(n) for n in ("conv2d_fwd", "conv2d_dgrad", "conv2d_wgrad", "conv2d_transpose_fwd", "conv2d_transpose_dgrad",
                                "conv2d_transpose_wgrad")}
    out.update(dense_fwd=dense_fwd, transpose_weight=transpose_weight, colsum=colsum, bn_act_add=bn_act_add, bn_bwd=bn_bwd)
    return out


def recorded_launches(monkeypatch, model, dtype):
    import unet_rir_amd as U
    import vae_cpu_ops
    from oracle import torch_ref as R
    from sim_runtime import SimRuntime
    rt = SimRuntime()
    impl = vae_cpu_ops.install(monkeypatch, rt)
    seen = set()
    rec = _recorders(seen)
    names = [n for n in dir(impl) + dir(vae_cpu_ops.VaeCpuOps(rt)) if not n.startswith("_") and n != "rt" and not n.endswith(KEEP)]
    for n in names:
        monkeypatch.setattr(U.ops, n, rec.get(n, lambda *a, **k: None))
    cls = U.AutoencoderEngine if model == "ae" else U.VAEEngine
    eng = cls(T.H, T.W, T.B, T.FILTERS, (3, 3, 3, 3), (2, 2, 2, 2), T.LATENT, T.N_NEURONS, device="cpu", runtime=rt, dtype=dtype)
    assert eng.PAD == T.pad(dtype) and eng.shape_before_bottleneck == (9, 10, 512)
    tr = U.Trainer(eng, lr=1e-3)
    spec_in, emb, spec_out = (torch.tensor(a) for a in R.synthetic_batch(R.Config(T.H, T.W, 16, 3), T.B))
    tr.step(spec_in, emb, spec_out)
    return seen


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("model", ["ae", "vae"])
def test_the_case_table_is_the_set_of_launches_of_the_engine(monkeypatch, model, dtype):
    got = recorded_launches(monkeypatch, model, dtype)
    want = T.launches(model, dtype)
    assert got == want, f"launched but not in the table: {sorted(got - want, key=str)}; in the table but never launched: {sorted(want - got, key=str)}"


def test_a_table_without_the_stride_1_transposed_layer_is_rejected(monkeypatch):
    """The comparison above has teeth: the table minus decoder_conv_transpose_layer_0 no longer equals the engine's launches."""
    got = recorded_launches(monkeypatch, "vae", "bf16")
    monkeypatch.setattr(T, "CONVT_LAYERS", [c for c in T.CONVT_LAYERS if c[0] != 1])
    want = T.launches("vae", "bf16")
    assert {n for n, *_ in got - want} == {"conv2d_transpose_fwd", "conv2d_transpose_dgrad", "conv2d_transpose_wgrad"} and not (want - got)


def test_the_batchnorm_pairs_are_cases_of_the_element_by_element_test():
    """The (C, P) pairs of the graph's BatchNorm -> ReLU / LeakyReLU layers run in tests/test_streaming_gpu.py, in both storage types."""
    from test_streaming_gpu import BN_CASES, BF16, F32
    have = {(c, p, t) for c, p, t, _ in BN_CASES}
    assert all((c, p, t) in have for c, p in T.BN_PAIRS for t in (BF16, F32))
