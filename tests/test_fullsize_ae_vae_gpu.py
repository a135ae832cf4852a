"""Oracle parity AT THE LAUNCHED SHAPES of the Autoencoder and the VAE of main_training.py (:118-129, :142-152; the geometry
profiles/vae_step.json times): 144 x 160 input, batch 32, filters (64, 128, 256, 512), strides 2, latent 64, n_neurons 2048, in bf16
AND fp32 storage.  The table of launches is tests/ae_vae_cases.py; tests/test_ae_vae_cases.py asserts (without a GPU) that it is exactly
what the two engines launch.

Every layer is compared over its WHOLE output - forward (+ bias), data gradient, complete weight gradient - in the two data kinds
of tests/test_kernels_gpu.py, one fp64 oracle evaluation per (layer, kind) serving both storage types and every switch set:
  "uniform"  bf16-representable uniform(-1, 1) values: bf16 outputs within 1e-2 of the tensor's scale, fp32 outputs and every weight
             gradient within 2e-6 sqrt(K) + 1e-6 of it (the tolerances of test_kernels_gpu.py / test_fullsize_resae_gpu.py)
  "int"      the integer data of tests/exact_data.py: the exactness conditions are asserted from the oracle's side, then EVERY stored
             element must equal the oracle's (bf16: its round-to-nearest-even), under every switch set of CONV_SWITCH_SETS /
             CONVT_SWITCH_SETS / WGRAD_SETTINGS (fp32 storage reads one switch, conv3x3: defaults and conv3x3 = 0).

  Conv2D 3x3 / 2          2 (stored 8 | 4) -> 64 @ 144 x 160, 64 -> 128 @ 72 x 80, 128 -> 256 @ 36 x 40, 256 -> 512 @ 18 x 20; with the
                          packed kernel copy where the engine makes one.  plan_conv (csrc/api.hip) offers no fused column statistics
                          for 3x3 stride 2 in either direction, so these layers launch conv2d_fwd, as the engines do (asserted)
  Conv2DTranspose 3x3     stride 1 512 -> 512 @ 9 x 10 (fused statistics under every switch set that reports rows), stride 2
                          512 -> 256 @ 9 x 10, 256 -> 128 @ 18 x 20, 128 -> 64 @ 36 x 40, 64 -> 2 (stored 8 | 4) @ 72 x 80
  Dense (fp32)            8192 -> 2048 (32 K slices), 48 128 -> 64 (128 slices: the cap), 64 -> 46 080 (1: the igemm epilogue writes
                          the bias); the three data gradients through dense_fwd on the transpose_weight copy; 46 080 <- 64 also
                          through conv2d_dgrad with an in-place addend (the VAE's second head); weight gradients through
                          conv2d_wgrad on 32 "pixels"; bias gradients through colsum; once with ld > C and poison behind the row and
                          exactly the advertised workspace in front of a canary
The BatchNorm -> ReLU / LeakyReLU pairs of the graph are cases of tests/test_streaming_gpu.py::test_batchnorm_family_element_by_element.
The whole step at this size (oracle-free invariants) is at the end of the file."""
import math

import pytest
import torch

import ae_vae_cases as T
import exact_data as X
from oracle import torch_ref as R
from test_kernels_gpu import CONV_SWITCH_SETS, CONVT_SWITCH_SETS, WGRAD_SETTINGS, q16, rand, set_switches
from test_streaming_gpu import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = T.B
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
POISON = {"bf16": 768.0, "f32": 777.0}
F32_SWITCH_SETS = [{}, dict(conv3x3=0)]          # the one switch plan_conv reads for fp32 storage
RATIO = {}                                       # family -> largest observed error / tolerance on the uniform kind


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    unet_rir_amd._lib.lib()
    yield unet_rir_amd
    set_switches(unet_rir_amd.ops)
    print("\nexact comparisons of this process so far:", X.STATS)
    print("largest error / tolerance on the uniform kind:", {k: round(v, 4) for k, v in sorted(RATIO.items())})


def close(got, want, tol, what, fam):
    """max |got - want| <= tol * max |want| (test_kernels_gpu.close), the ratio kept for the report."""
    w = want.to(got.device).double()
    assert tuple(got.shape) == tuple(w.shape), (what, tuple(got.shape), tuple(w.shape))
    scale = float(w.abs().max()) + 1e-30
    err = float((got.double() - w).abs().max())
    print(f"{what}: max err {err:.3e}, tolerance {tol * scale:.3e}")
    RATIO[fam] = max(RATIO.get(fam, 0.0), err / (tol * scale))
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {tol})"


def act(ops, t_nhwc, dt, stored=None, ld=None, c0=0):
    """fp64 [B,H,W,C] -> Act of `stored` channels (the extra ones zero) at offset c0 of a poisoned buffer with pixel stride ld."""
    C = t_nhwc.shape[-1]
    stored = C if stored is None else stored
    ld = stored if ld is None else ld
    buf = torch.full(tuple(t_nhwc.shape[:3]) + (ld,), POISON[dt], dtype=DT[dt])
    buf[..., c0:c0 + stored] = 0
    buf[..., c0:c0 + C] = t_nhwc.to(DT[dt])
    return ops.Act(buf.to(DEV), c0, stored)


def blank(ops, shape, dt, ld=None, c0=0):
    ld = shape[-1] if ld is None else ld
    return ops.Act(torch.full(tuple(shape[:3]) + (ld,), POISON[dt], dtype=DT[dt], device=DEV), c0, shape[-1])


def poison_intact(a, dt):
    rest = torch.cat([a.base[..., :a.c0], a.base[..., a.c0 + a.C:]], dim=-1)
    return bool((rest.float() == POISON[dt]).all())


def padded(t, dim, n):
    """t zero-padded to n entries along dim."""
    if t.shape[dim] == n:
        return t
    sh = list(t.shape)
    sh[dim] = n - t.shape[dim]
    return torch.cat([t, torch.zeros(sh, dtype=t.dtype)], dim=dim)


def stored(want, dt, exact):
    """What the library stores for an exact fp64 result in this storage type (integer data)."""
    return (X.expected_bf16(want) if dt == "bf16" else want) if exact else want


def kernels(ops, w32, N, C_, dt, packed):
    """The work copies an engine keeps of the fp32 master [N][9][C]: as stored, channel roles swapped [C][9][N], packed or None."""
    if dt == "f32":
        wt = torch.empty((C_, 9, N), device=DEV)
        ops.transpose_weight(w32, wt, N, 9, C_)
        return w32, wt, None
    same = torch.empty((N, 9, C_), dtype=torch.bfloat16, device=DEV)
    tr = torch.empty((C_, 9, N), dtype=torch.bfloat16, device=DEV)
    ne = ops.conv3x3s2_packed_elems(N, C_) if packed else 0
    pk = torch.zeros(ne, dtype=torch.bfloat16, device=DEV) if ne else None
    ops.cast_weights_batched(ops.make_cast_table([(w32, same, tr, N, 9, C_, C_, N, pk)], DEV))       # the engines' launch
    chk_s, chk_t = torch.empty_like(same), torch.empty_like(tr)
    ops.cast_weight_bf16(w32, chk_s, N, 9, C_, C_)
    ops.transpose_cast_weight_bf16(w32, chk_t, N, 9, C_, N)
    torch.cuda.synchronize()
    assert torch.equal(same, chk_s) and torch.equal(tr, chk_t)
    assert torch.equal(tr.float(), w32.view(N, 9, C_).permute(2, 1, 0))          # bf16-representable masters: the copy is the value
    return same, tr, pk


# ------------------------------------------------------------------------------------------------------------------ Conv2D
@X.parametrize_kinds("layer", T.CONV_LAYERS)
def test_conv2d_layers_of_the_encoder_over_the_whole_tensor(U, layer, data):
    ops = U.ops
    exact = data == "int"
    ci, co, h, w = layer
    i = T.CONV_LAYERS.index(layer)
    x = q16(rand(f"aex{layer}", (B, ci, h, w), data)).requires_grad_(True)
    wk = q16(rand(f"aew{layer}", (3, 3, ci, co), data, "kernel")).requires_grad_(True)         # HWIO
    b = rand(f"aeb{layer}", (co,), data, "bias")
    y = R.conv2d_same(x, wk, b, 2)
    Ho, Wo = y.shape[2], y.shape[3]
    gy = q16(rand(f"aeg{layer}", (B, co, Ho, Wo), data))
    (y * gy).sum().backward()
    reg = X.REG if exact else 0.002
    if exact:
        ties = X.check_exactness_conditions({"x": (x.detach(), True), "w": (wk.detach(), True), "bias": (b, False)},
                                            X.conv_abs_bound(9 * ci, has_addend=False), y.detach(), what=f"fwd {layer}")
        ties_d = X.check_exactness_conditions({"dy": (gy, True)}, X.conv_abs_bound(9 * co, has_bias=False, has_addend=False), x.grad,
                                              what=f"dgrad {layer}")
        X.check_exactness_conditions({"w": (wk.detach(), False)}, B * Ho * Wo * 9 + 1, quantum=0.5, what=f"wgrad {layer}")
        assert ties > 0 and (ties_d > 0 or ci == 2), (ties, ties_d)          # the network input has no gradient: nothing is stored
        X.note_ties(ties + ties_d)
        print(f"conv {layer}: {ties} of {y.numel()} forward and {ties_d} of {x.numel()} data-gradient outputs are bf16 ties")
    want_y, want_dx = X.nhwc(y.detach()), X.nhwc(x.grad)
    tag = f"conv 3x3/2 {ci}->{co}@{h}x{w}"
    for dt in ("bf16", "f32"):
        pad = T.pad(dt)
        cs = pad if ci == 2 else ci                           # stored input channels: the network input is zero-padded
        g = ops.geom(*T.conv_geom(layer, dt))
        strided = i == 1                                      # 64 -> 128: input at an offset of a wider buffer, output with poison behind it
        xa = act(ops, X.nhwc(x.detach()), dt, cs, cs + pad if strided else None, pad if strided else 0)
        gya = act(ops, X.nhwc(gy), dt)
        w32 = padded(wk.detach().permute(3, 0, 1, 2), 3, cs).contiguous().float().to(DEV)          # [Co][3][3][cs] fp32 master
        bias = b.float().to(DEV)
        wf, wt, pk = kernels(ops, w32, co, cs, dt, True)
        assert ops.conv2d_colstat_rows(g, 0, xa) == 0          # no fused statistics for 3x3 stride 2: the engines launch conv2d_fwd
        assert (pk is not None) == (dt == "bf16" and ci != 2)
        sets = (CONV_SWITCH_SETS if dt == "bf16" else F32_SWITCH_SETS) if exact else [{}]
        wy, wdx = stored(want_y, dt, exact).to(DEV), stored(want_dx, dt, exact).to(DEV)
        for sw in sets:
            set_switches(ops, sw)
            ya = blank(ops, (B, Ho, Wo, co), dt, co + pad if strided else None)
            ops.conv2d_fwd(g, xa, wf, bias, ya, w_packed=pk)
            dxa = blank(ops, (B, h, w, cs), dt, cs + pad if strided else None)
            if ci != 2:                                       # the network input has no gradient: never launched
                ops.conv2d_dgrad(g, gya, wt, dxa)
            torch.cuda.synchronize()
            assert poison_intact(ya, dt) and poison_intact(dxa, dt) and poison_intact(xa, dt)
            if exact:
                X.assert_exact(ya.dense(), wy, f"{tag} {dt} fwd {sw}", tile=(16, 32))
                if ci != 2:
                    X.assert_exact(dxa.dense(), wdx, f"{tag} {dt} dgrad {sw}", tile=(16, 32))
            else:
                close(ya.dense(), wy, 1e-2 if dt == "bf16" else 2e-6 * math.sqrt(9 * ci) + 1e-6, f"{tag} {dt} fwd", f"conv fwd {dt}")
                if ci != 2:
                    close(dxa.dense(), wdx, 1e-2 if dt == "bf16" else 2e-6 * math.sqrt(9 * co) + 1e-6, f"{tag} {dt} dgrad", f"conv dgrad {dt}")
        set_switches(ops)
        if pk is not None:          # the same layer without the packed copy: the same bits
            y2 = blank(ops, (B, Ho, Wo, co), dt)
            ops.conv2d_fwd(g, xa, wf, bias, y2)
            torch.cuda.synchronize()
            assert torch.equal(y2.dense(), ya.dense())
        want_dw = padded((wk.grad + reg * wk.detach()).permute(3, 0, 1, 2), 3, cs)
        for sw in (WGRAD_SETTINGS if dt == "bf16" and exact else [{}]):
            set_switches(ops, sw)
            ws = ops.Workspace(DEV)
            dw = torch.full((co, 3, 3, cs), 111.0, device=DEV)
            ops.conv2d_wgrad(g, xa, gya, dw, ws, reg=reg, w=w32)
            torch.cuda.synchronize()
            if exact:
                X.assert_exact(dw, want_dw, f"{tag} {dt} wgrad {sw}")
            else:
                close(dw, want_dw, 2e-6 * math.sqrt(B * Ho * Wo) + 1e-6, f"{tag} {dt} wgrad", f"conv wgrad {dt}")
        set_switches(ops)


# --------------------------------------------------------------------------------------------------------- Conv2DTranspose
@X.parametrize_kinds("layer", T.CONVT_LAYERS)
def test_conv2d_transpose_layers_of_the_decoder_over_the_whole_tensor(U, layer, data):
    ops = U.ops
    exact = data == "int"
    s, ci, co, h, w = layer
    i = T.CONVT_LAYERS.index(layer)
    x = q16(rand(f"aetx{layer}", (B, ci, h, w), data)).requires_grad_(True)
    wk = q16(rand(f"aetw{layer}", (3, 3, co, ci), data, "kernel")).requires_grad_(True)        # HWOI
    b = rand(f"aetb{layer}", (co,), data, "bias")
    y = R.conv2d_transpose_same(x, wk, b, s)
    HH, WW = h * s, w * s
    assert tuple(y.shape) == (B, co, HH, WW)
    gy = q16(rand(f"aetg{layer}", tuple(y.shape), data))
    (y * gy).sum().backward()
    reg = X.REG if exact else 0.002
    if exact:
        ties = X.check_exactness_conditions({"x": (x.detach(), True), "w": (wk.detach(), True), "bias": (b, False)},
                                            X.conv_abs_bound(9 * ci, has_addend=False), y.detach(), what=f"convT fwd {layer}")
        ties_d = X.check_exactness_conditions({"dy": (gy, True)}, X.conv_abs_bound(9 * co, has_bias=False, has_addend=False), x.grad,
                                              what=f"convT dgrad {layer}")
        X.check_exactness_conditions({"w": (wk.detach(), False)}, B * h * w * 9 + 1, quantum=0.5, what=f"convT wgrad {layer}")
        # the data gradient of the 2-channel output layer sums 18 terms: |value| <= 108 < 256, every such integer IS a bf16 value
        assert ties > 0 and (ties_d > 0 or X.conv_abs_bound(9 * co, has_bias=False, has_addend=False) < 256), (ties, ties_d)
        X.note_ties(ties + ties_d)
        print(f"convT {layer}: {ties} of {y.numel()} forward and {ties_d} of {x.numel()} data-gradient outputs are bf16 ties")
    tag = f"convT 3x3/{s} {ci}->{co}@{h}x{w}"
    for dt in ("bf16", "f32"):
        pad = T.pad(dt)
        cs = pad if co == 2 else co                           # stored output channels: the 2-channel output layer is zero-padded
        g = ops.geom(*T.convt_geom(layer, dt))
        strided = i == 2                                      # 256 -> 128: output into the upper half of a wider buffer, dy read from one
        want_y, want_dx = padded(X.nhwc(y.detach()), 3, cs), X.nhwc(x.grad)
        wy, wdx = stored(want_y, dt, exact).to(DEV), stored(want_dx, dt, exact).to(DEV)
        xa = act(ops, X.nhwc(x.detach()), dt)
        gya = act(ops, X.nhwc(gy), dt, cs, 2 * cs if strided else None, cs if strided else 0)      # padded channels of dy are zero
        w32 = padded(wk.detach().permute(3, 0, 1, 2), 3, cs).contiguous().float().to(DEV)          # primary [Ci][3][3][cs], padded rows zero
        bias = padded(b, 0, cs).float().to(DEV)
        wprim, wt, pk = kernels(ops, w32, ci, cs, dt, s == 2)
        assert (pk is not None) == (dt == "bf16" and s == 2 and co != 2)
        sets = ((CONV_SWITCH_SETS if s == 1 else CONVT_SWITCH_SETS) if dt == "bf16" else F32_SWITCH_SETS) if exact else [{}]
        with_rows = 0
        for sw in sets:
            set_switches(ops, sw)
            rows = ops.conv2d_transpose_colstat_rows(g, xa)
            if not sw:          # the engines' launch: only the stride-1 layer has BatchNorm statistics from its own epilogue
                assert (rows > 0) == (dt == "bf16" and s == 1), rows
            ya = blank(ops, (B, HH, WW, cs), dt, 2 * cs if strided else None, cs if strided else 0)
            cst = torch.full((max(rows, 1), cs, 2), 7.0, device=DEV)
            if rows:
                ops.conv2d_transpose_fwd_colstat(g, xa, wt, bias, ya, cst)
                with_rows += 1
            else:
                ops.conv2d_transpose_fwd(g, xa, wt, bias, ya)
            dxa = blank(ops, (B, h, w, ci), dt)
            ops.conv2d_transpose_dgrad(g, gya, wprim, dxa, w_packed=pk)
            torch.cuda.synchronize()
            assert poison_intact(ya, dt) and poison_intact(gya, dt)
            if exact:
                X.assert_exact(ya.dense(), wy, f"{tag} {dt} fwd {sw}", tile=(32, 64))
                X.assert_exact(dxa.dense(), wdx, f"{tag} {dt} dgrad {sw}", tile=(16, 32))
            else:
                close(ya.dense(), wy, 1e-2 if dt == "bf16" else 2e-6 * math.sqrt(9 * ci) + 1e-6, f"{tag} {dt} fwd", f"convT fwd {dt}")
                close(dxa.dense(), wdx, 1e-2 if dt == "bf16" else 2e-6 * math.sqrt(9 * co) + 1e-6, f"{tag} {dt} dgrad", f"convT dgrad {dt}")
            if rows:            # per-tile (sum, sum of squares) of the STORED tensor
                yd = ya.dense().double()
                tot = cst.double().sum(dim=0)
                col, sq = yd.sum(dim=(0, 1, 2)), (yd * yd).sum(dim=(0, 1, 2))
                if exact:
                    # the whole column of |stored outputs| stays below 2^24, so every partial sum of any tiling is an exact integer
                    assert torch.equal(wy, wy.round()) and float(wy.abs().sum(dim=(0, 1, 2)).max()) < X.EXACT_LIMIT
                    X.assert_exact(tot[:, 0], col, f"{tag} colstat sums on integer data {sw}")
                else:
                    close(tot[:, 0], col, 2e-6, f"{tag} colstat sum", "colstat")
                close(tot[:, 1], sq, 2e-6, f"{tag} colstat sum of squares {sw}", "colstat")
        set_switches(ops)
        assert with_rows > 0 or not (dt == "bf16" and s == 1)
        if pk is not None:          # the data gradient without the packed copy: the same bits
            d2 = blank(ops, (B, h, w, ci), dt)
            ops.conv2d_transpose_dgrad(g, gya, wprim, d2)
            torch.cuda.synchronize()
            assert torch.equal(d2.dense(), dxa.dense())
        want_dw = padded((wk.grad + reg * wk.detach()).permute(3, 0, 1, 2), 3, cs)                 # padded columns: 0 + reg * 0
        for sw in (WGRAD_SETTINGS if dt == "bf16" and exact else [{}]):
            set_switches(ops, sw)
            ws = ops.Workspace(DEV)
            dw = torch.full((ci, 3, 3, cs), 111.0, device=DEV)
            ops.conv2d_transpose_wgrad(g, xa, gya, dw, ws, reg=reg, w=w32)
            torch.cuda.synchronize()
            if exact:
                X.assert_exact(dw, want_dw, f"{tag} {dt} wgrad {sw}")
            else:
                close(dw, want_dw, 2e-6 * math.sqrt(B * h * w) + 1e-6, f"{tag} {dt} wgrad", f"convT wgrad {dt}")
        set_switches(ops)


# ------------------------------------------------------------------------------------------------------------------- Dense
DENSE_SLICES = {(8192, 2048): 32, (T.N_CAT, 64): 128, (64, T.N_FEAT): 1}          # K slices of dense_ksplit (csrc/igemm.hip), forward
DGRAD_SLICES = {(8192, 2048): 8, (T.N_CAT, 64): 1, (64, T.N_FEAT): 128}           # ... and of the data gradient (K and N swapped)


def cmp32(exact, got, want, K, what, fam):
    if exact:
        X.assert_exact(got, want, what)
    else:
        close(got, want, 2e-6 * math.sqrt(K) + 1e-6, what, fam)


@X.parametrize_kinds("K,N", T.DENSE_LAYERS)
def test_dense_layers_over_the_whole_tensor(U, K, N, data):
    """Each launch twice: dense rows and an ample workspace; then pixel strides larger than the row with poison behind it and exactly
    the advertised workspace in front of a canary."""
    ops, L = U.ops, U._lib.lib()
    exact = data == "int"
    assert L.unetrir_dense_fwd_ws_bytes(B, K, N) == DENSE_SLICES[(K, N)] * B * N * 4          # the K-split plans this test is there for
    assert L.unetrir_dense_fwd_ws_bytes(B, N, K) == DGRAD_SLICES[(K, N)] * B * K * 4
    x = rand(f"aedx{K, N}", (B, K), data)
    w = rand(f"aedw{K, N}", (N, K), data, "kernel") * (1.0 if exact else 0.05)
    w = w.float().double()
    b = rand(f"aedb{K, N}", (N,), data, "bias")
    dy = rand(f"aedg{K, N}", (B, N), data)
    add = rand(f"aeda{K, N}", (B, K), data, "addend")
    reg = X.REG if exact else 0.002
    if exact:
        X.check_exactness_conditions({"x": (x, False), "w": (w, False), "bias": (b, False), "dy": (dy, False), "addend": (add, False)},
                                     X.conv_abs_bound(max(K, N)), what=f"dense {K, N}")
        X.check_exactness_conditions({}, B * 9 + 1, quantum=0.5, what=f"dense wgrad {K, N}")
    wd, bd = w.float().to(DEV), b.float().to(DEV)
    wt = torch.full((K, 1, N), 5.0, device=DEV)
    ops.transpose_weight(wd, wt, N, 1, K)
    torch.cuda.synchronize()
    assert torch.equal(wt.view(K, N), wd.t())                # a copy: compared with ==
    want_y, want_dx = x @ w.t() + b, dy @ w
    want_dw, want_db = dy.t() @ x, dy.sum(0)
    g = ops.geom(B, 1, 1, K, N, 1, 1)
    row = lambda t: t.view(B, 1, 1, -1)
    tag = f"dense {K}->{N}"
    for guarded in (False, True):
        pad = 4 if guarded else 0
        ldk, ldn = K + pad, N + pad

        def workspace(adv, ceiling):
            return Guarded(ops, adv, ceiling + (1 << 20)) if guarded else None

        def run(adv, ceiling, call, what):
            gd = workspace(adv, max(adv, ceiling))
            call(gd.ws if gd else ops.Workspace(DEV, adv + (1 << 20)))
            if gd:
                gd.assert_intact(f"{tag} {what}")
            torch.cuda.synchronize()
        xa, dya = act(ops, row(x), "f32", K, ldk), act(ops, row(dy), "f32", N, ldn)
        ya, dxa = blank(ops, (B, 1, 1, N), "f32", ldn), blank(ops, (B, 1, 1, K), "f32", ldk)
        run(L.unetrir_dense_fwd_ws_bytes(B, K, N), 0, lambda ws: ops.dense_fwd(xa, wd, bd, ya, ws), "fwd")
        cmp32(exact, ya.dense().view(B, N), want_y, K, f"{tag} fwd", "dense fwd")
        run(L.unetrir_dense_fwd_ws_bytes(B, N, K), 0, lambda ws: ops.dense_fwd(dya, wt, None, dxa, ws), "dgrad (dense_fwd on the transposed copy)")
        cmp32(exact, dxa.dense().view(B, K), want_dx, N, f"{tag} dgrad", "dense dgrad")
        assert poison_intact(ya, "f32") and poison_intact(dxa, "f32") and poison_intact(xa, "f32") and poison_intact(dya, "f32")
        if (K, N) == (T.N_CAT, 64):          # the VAE's second head: the data gradient added in place behind the first one's
            acc = act(ops, row(add), "f32", K, ldk)
            ops.conv2d_dgrad(g, dya, wt, acc, addend=acc)
            torch.cuda.synchronize()
            cmp32(exact, acc.dense().view(B, K), want_dx + add, N, f"{tag} dgrad + addend in place (igemm)", "dense dgrad")
            assert poison_intact(acc, "f32")
        r = reg if guarded else 0.0          # the engines launch the Dense weight gradients without an l2 term
        dw = torch.full((N, 1, 1, K), 111.0, device=DEV)
        run(ops.conv2d_wgrad_ws_bytes(g), 0, lambda ws: ops.conv2d_wgrad(g, xa, dya, dw, ws, reg=r, w=wd), "wgrad")
        cmp32(exact, dw.view(N, K), want_dw + r * w, B, f"{tag} wgrad", "dense wgrad")
        db = torch.full((N,), 111.0, device=DEV)
        run(ops.bn_ws_bytes(B, N), min(2048, B) * N * 16 + 8 * N, lambda ws: ops.colsum(dya, db, ws), "colsum")
        cmp32(exact, db, want_db, B, f"{tag} bias gradient", "colsum")


@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_bias_gradient_of_the_output_layer(U, dt):
    """colsum over the 32 x 144 x 160 pixels of the padded 2-channel dL/dlogits (integers: exact; the padded channels sum to zero)."""
    ops = U.ops
    pad = T.pad(dt)
    dy = X.acts(f"aeout{dt}", (B, T.H, T.W, 2))
    X.check_exactness_conditions({"dy": (dy, dt == "bf16")}, B * T.H * T.W * 3, what="output-layer colsum")
    dya = act(ops, dy, dt, pad)
    out = torch.full((pad,), 111.0, device=DEV)
    P = B * T.H * T.W
    gd = Guarded(ops, ops.bn_ws_bytes(P, pad), 2048 * pad * 16 + 8 * pad + (1 << 20))
    ops.colsum(dya, out, gd.ws)
    gd.assert_intact("output-layer colsum")
    X.assert_exact(out, padded(dy.sum(dim=(0, 1, 2)), 0, pad), f"output-layer bias gradient {dt}")


# --------------------------------------------------------------------------------------------------------- the whole step
def _engine(U, model, dt, overlap=False):
    cls = U.AutoencoderEngine if model == "ae" else U.VAEEngine
    eng = cls(T.H, T.W, B, T.FILTERS, (3, 3, 3, 3), (2, 2, 2, 2), T.LATENT, T.N_NEURONS, device=DEV, dtype=dt, overlap_wgrad=overlap)
    gen = torch.Generator()
    gen.manual_seed(0)
    eng.reset_parameters(gen)                      # Keras default initialisers
    eng.dropout_seed = 9
    return eng


def _step(eng, batch, eps=None):
    """Forward + backward from draw 0 of the engine's noise stream (the VAE's eps: its own draw, or the one supplied)."""
    spec_in, emb, spec_out = batch
    eng.training = True
    eng._shared["dropout_step"] = 0
    if "eps" in eng.masks:
        eng.masks["eps"] = eps
    eng.forward(spec_in, emb, target=spec_out, global_batch=B)
    eng.backward()
    torch.cuda.synchronize()
    return eng.pred.clone(), eng.grad.clone(), float(eng.loss_out[0])


def _bn_inputs(eng):
    """(name, node BatchNormalization reads) of the eight BatchNorm layers, from the order _build registers the nodes in."""
    enc = [(f"encoder_bn_{i + 1}", eng.nodes[1 + 2 * i]) for i in range(4)]
    dec = [(f"decoder_bn_{j}", eng.nodes[-9 + 2 * j]) for j in range(4)]
    for (name, n), (C, P) in zip(enc + dec, T.BN_PAIRS + T.BN_PAIRS[::-1]):
        assert name in eng.bn_names and (n.a.C, n.a.P) == (C, P), (name, n.a.C, n.a.P)
    return enc + dec


@pytest.mark.parametrize("model", ["ae", "vae"])
def test_train_step_invariants_at_the_real_geometry(U, model):
    """AutoencoderEngine / VAEEngine, fp32 and bf16 storage on the same variables and the same batch of 32 x [2, 144, 160]."""
    batch = next(U.synthetic_batches(1, B, T.H, T.W, DEV))
    e32 = _engine(U, model, "f32")
    e16 = _engine(U, model, "bf16")
    e16.load_keras_params(e32.export_keras_params())
    assert e32.n_params() == e16.n_params()
    first, eps = {}, None
    for dt, eng in (("f32", e32), ("bf16", e16)):
        pred, grad, loss = _step(eng, batch)
        assert float(pred.min()) >= 0.0 and float(pred.max()) <= 1.0 and math.isfinite(loss) and bool(torch.isfinite(grad).all())
        if dt == "f32":
            # BatchNormalization with batch statistics, fp32 storage: the statistics the layer normalised with are in its moving
            # statistics (first step from (0, 1), momentum 0.99).  Against the fp64 moments of the tensor it read, the output has
            # mean (m - m_used) rstd and variance var / (var_used + eps) instead of var / (var + eps): the bounds of test_fullsize_gpu.py
            for name, node in _bn_inputs(eng):
                xd = node.a.dense().double().view(-1, node.a.C)
                m, v = xd.mean(0), xd.var(0, unbiased=False)
                P = xd.shape[0]
                m_used = eng.moving[name + ".moving_mean"].double() / 0.01
                v_used = (eng.moving[name + ".moving_variance"].double() - 0.99) / 0.01 * (P - 1) / P
                out_mean = (m - m_used) / torch.sqrt(v_used + 1e-3)
                out_var, want_var = v / (v_used + 1e-3), v / (v + 1e-3)
                print(f"{model} {name}: |output mean| {float(out_mean.abs().max()):.2e}, variance off by {float((out_var - want_var).abs().max()):.2e}")
                assert float(out_mean.abs().max()) < 1e-3 and float((out_var - want_var).abs().max()) < 1e-3, name
        if model == "vae":
            eps = eng._eps_buf.clone() if eps is None else eps
            assert torch.equal(eng._eps_buf, eps)               # both engines draw the same noise from the same seed and draw number
            # kl_out[0] = inv_gb * kl_out[1] as ONE fp32 product; kl_out[1] within the bound of tests/test_vae_gpu.py's docstring of the
            # fp64 sum over the engine's own stored mu / log_var
            kl = eng.kl_out.cpu()
            m, l = eng._mu.a.dense().double().cpu().view(B, -1), eng._lv.a.dense().double().cpu().view(B, -1)
            U32, U64 = 2.0 ** -24, 2.0 ** -53
            S = 1 + l.abs() + m * m + torch.exp(l)
            t = -0.5 * (1 + l - m * m - torch.exp(l))
            ref = float(t.sum())
            d_sum = float((0.5 * U32 * (4 * S + 6 * torch.exp(l))).sum()) + t.numel() * U64 * float(t.abs().sum())
            d_sum += U32 * (abs(ref) + d_sum)
            print(f"vae {dt}: kl sum {float(kl[1]):.9g} ref {ref:.12g} bound {d_sum:.3g}")
            assert abs(float(kl[1].double()) - ref) <= d_sum, (float(kl[1]), ref, d_sum)
            assert float(kl[0]) == float(torch.tensor(1.0 / B, dtype=torch.float32) * kl[1])
        # same inputs, same draws: same bits
        pred2, grad2, loss2 = _step(eng, batch)
        assert torch.equal(pred2, pred) and torch.equal(grad2, grad) and loss2 == loss
        first[dt] = (pred, grad, loss)
    # a batch permutation (eps permuted with it, no dropout) permutes the prediction: bit for bit in fp32 storage; in bf16 storage the
    # statistics of the permuted batch are the same sums in another order and a last-bit difference flips bf16 roundings - bounded, as
    # tests/test_fullsize_resae_gpu.py derives it, by half of the bf16 engine's own distance to the fp32 engine, x 1.5, measured here
    pg = torch.Generator(device=DEV)
    pg.manual_seed(3)
    perm = torch.randperm(B, device=DEV, generator=pg)
    pbatch = tuple(t[perm].contiguous() for t in batch)
    peps = eps[perm].contiguous() if model == "vae" else None
    base = {dt: _step(eng, batch, eps)[0] for dt, eng in (("f32", e32), ("bf16", e16))}          # with eps supplied: the same bits as drawn
    assert torch.equal(base["f32"], first["f32"][0]) and torch.equal(base["bf16"], first["bf16"][0])
    p32 = _step(e32, pbatch, peps)[0]
    p16 = _step(e16, pbatch, peps)[0]
    rms = lambda d: float(d.double().pow(2).mean().sqrt())
    dist = (base["bf16"] - base["f32"]).abs()
    move = (p16 - base["bf16"][perm]).abs()
    print(f"{model}: bf16 to fp32 storage: prediction rms {rms(dist):.3e} max {float(dist.max()):.3e}; bf16 under a batch permutation: "
          f"rms {rms(move):.3e} max {float(move.max()):.3e}; fp32 under it: max {float((p32 - base['f32'][perm]).abs().max()):.3e}")
    assert torch.equal(p32, base["f32"][perm])
    assert rms(move) <= 1.5 * 0.5 * rms(dist) and float(move.max()) <= 1.5 * 0.5 * float(dist.max())
    # it trains: ten Adam steps
    for eng in (e32, e16):
        if "eps" in eng.masks:
            eng.masks["eps"] = None
        tr = U.Trainer(eng, lr=1e-4, dropout=False)
        losses = [tr.step(*batch, return_loss=True) for _ in range(10)]
        print(f"{model} {eng.dtype}: loss over ten Adam steps {losses[0]:.6f} -> {losses[-1]:.6f}")
        assert math.isfinite(losses[-1]) and losses[-1] < losses[0]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("model", ["ae", "vae"])
def test_graph_replay_equals_the_launched_step_at_the_real_geometry(U, model, dt):
    """Trainer(graph=True) against the same launches issued one by one, three steps with dropout (and the VAE's own noise):
    bit-identical variables and loss."""
    batch = next(U.synthetic_batches(1, B, T.H, T.W, DEV))
    out = []
    for graph in (True, False):
        eng = _engine(U, model, dt, overlap=True)
        if not graph:
            eng.use_device_counters(True)
        tr = U.Trainer(eng, lr=1e-4, graph=graph)
        for _ in range(3):
            tr.step(*batch)
        torch.cuda.synchronize()
        out.append((eng.theta.clone(), float(eng.loss_out[0])))
        del tr, eng
    assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]
