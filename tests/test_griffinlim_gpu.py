"""GPU tests of the Griffin-Lim reconstruction (csrc/griffinlim.hip through ops.griffinlim, features.GriffinLim and
Evaluator(algorithm='gl')) against the fp64 yardstick tests/griffinlim_ref.py.

Tolerance of the parity test, per sample: |y_dev - y_ref| <= 2^-24 |y_ref| + 1e-9 max|y_ref|.  The device keeps all state and
arithmetic in fp64 and rounds the waveform to fp32 once (the first term); the second is the bound to which two fp64 forms of
the loop with different summation orders are held on the CPU (tests/test_griffinlim.py: they reach ~1e-11 after 32 iterations).
Both take the same fp32 feature values and the same fp32 initial phases."""
import numpy as np
import pytest
import torch

import griffinlim_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


def run(U, name, denormalize, tight, n_iter, momentum, pad_mode, init_phase="given", seed=0, draw=0, ws=None):
    ops = U.ops
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    nb, nf = GC.dims(name)
    feat = torch.tensor(GC.features(name, denormalize, tight)).to(DEV)
    ip = torch.tensor(GC.init_phase(name)).to(DEV) if isinstance(init_phase, str) else init_phase
    wav = torch.full((B, hop * (nf - 1)), float("nan"), dtype=torch.float32, device=DEV)
    ops.griffinlim(feat, wav, nb, nf, n_fft, win, hop, ws if ws is not None else ops.Workspace(DEV), pad_mode=pad_mode,
                   denormalize=denormalize, n_iter=n_iter, momentum=momentum, init_phase=ip, seed=seed, draw=draw)
    return wav


LAYOUTS = [(n, False) for n in GC.GEOMETRIES] + [("rir", True)]      # padded planes everywhere; the reference's size also tight


@pytest.mark.parametrize("denormalize", [True, False], ids=["denorm", "raw"])
@pytest.mark.parametrize("pad_mode", ["reflect", "constant"])
@pytest.mark.parametrize("momentum", [0.99, 0.0])
@pytest.mark.parametrize("n_iter", [0, 1, 2, 32])
@pytest.mark.parametrize("name,tight", LAYOUTS, ids=[n + ("-tight" if t else "") for n, t in LAYOUTS])
def test_parity_per_element(U, name, tight, n_iter, momentum, pad_mode, denormalize):
    ref = GC.reference(name, denormalize, n_iter, momentum, pad_mode)
    got = run(U, name, denormalize, tight, n_iter, momentum, pad_mode).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    assert float(np.abs(ref[0, :ref.shape[1]] - ref[1, :ref.shape[1]]).max()) > 0.01 * float(np.abs(ref).max())     # samples differ
    for b in range(ref.shape[0]):
        peak = float(np.abs(ref[b]).max())
        err = np.abs(got[b] - ref[b])
        bound = 2.0 ** -24 * np.abs(ref[b]) + 1e-9 * peak
        worst = int(np.argmax(err - bound))
        print(f"{name} b={b}: max|dy| = {err.max():.3e} ({err.max() / peak:.3e} of the peak), worst sample {worst}: "
              f"err {err[worst]:.3e} bound {bound[worst]:.3e}")
        assert peak > 0 and bool((err <= bound).all()), (name, b, worst, float(err[worst]), float(bound[worst]))


def test_workspace_is_exactly_the_advertised_size(U):
    """ws_bytes = unetrir_griffinlim_ws_bytes exactly, a canary behind it; one byte less is refused."""
    ops, L = U.ops, U._lib.lib()
    name = "11frames"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    nb, nf = GC.dims(name)
    adv = ops.griffinlim_ws_bytes(B, nb, nf, n_fft)
    assert adv > 0 and adv % 8 == 0
    big = torch.full((adv + (1 << 20),), CANARY, dtype=torch.uint8, device=DEV)
    ws = ops.Workspace(DEV)
    ws.buf = big[:adv]
    got = run(U, name, True, False, 32, 0.99, "reflect", ws=ws)
    torch.cuda.synchronize()
    assert ws.buf.data_ptr() == big.data_ptr() and ws.nbytes == adv            # the wrapper asked for no more
    assert bool((big[adv:] == CANARY).all())
    assert torch.equal(got, run(U, name, True, False, 32, 0.99, "reflect"))
    feat = torch.tensor(GC.features(name, True, False)).to(DEV)
    wav = torch.empty((B, hop * (nf - 1)), dtype=torch.float32, device=DEV)
    args = (feat.data_ptr(), B, feat.shape[2], feat.shape[3], nb, nf, n_fft, win, hop, 0, 1, 2, 0.99, None, 0, 0, wav.data_ptr(),
            big.data_ptr())
    assert L.unetrir_griffinlim_f32(*args, adv - 1, None) == 10001
    assert L.unetrir_griffinlim_f32(*args, adv, None) == 0
    torch.cuda.synchronize()


def test_deterministic_and_capturable(U):
    """Two eager runs are bit-equal; the call captured in a HIP graph and replayed twice gives the eager bits."""
    ops = U.ops
    name = "rir"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    nb, nf = GC.dims(name)
    a = run(U, name, True, False, 32, 0.99, "reflect")
    b = run(U, name, True, False, 32, 0.99, "reflect")
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    feat = torch.tensor(GC.features(name, True, False)).to(DEV)
    ip = torch.tensor(GC.init_phase(name)).to(DEV)
    wav = torch.zeros((B, hop * (nf - 1)), dtype=torch.float32, device=DEV)
    ws = ops.Workspace(DEV, ops.griffinlim_ws_bytes(B, nb, nf, n_fft))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.griffinlim(feat, wav, nb, nf, n_fft, win, hop, ws, init_phase=ip)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.griffinlim(feat, wav, nb, nf, n_fft, win, hop, ws, init_phase=ip)
    for _ in range(2):
        wav.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wav, a)


def test_random_initial_phases(U):
    ops = U.ops
    name = "11frames"
    B = GC.GEOMETRIES[name][0]
    nb, nf = GC.dims(name)
    seed, draw = 7, 3
    u = torch.empty((B, nb, nf), dtype=torch.float32, device=DEV)
    ops.uniform(u, seed, draw)
    drawn = run(U, name, True, False, 32, 0.99, "reflect", init_phase=None, seed=seed, draw=draw)
    assert torch.equal(drawn, run(U, name, True, False, 32, 0.99, "reflect", init_phase=u))
    assert not torch.equal(drawn, run(U, name, True, False, 32, 0.99, "reflect", init_phase=None, seed=seed, draw=draw + 1))
    # the draw itself: [0, 1), mean 0.5 and variance 1/12 over 1e6 values (standard errors 2.9e-4 and 7.5e-5)
    n = 1000000
    big = torch.empty(n, dtype=torch.float32, device=DEV)
    ops.uniform(big, seed, draw)
    assert torch.equal(big[:u.numel()], u.flatten())                            # a shorter draw is a prefix of a longer one
    d = big.double()
    assert float(d.min()) >= 0.0 and float(d.max()) < 1.0
    assert abs(float(d.mean()) - 0.5) <= 0.002 and abs(float(d.var()) - 1.0 / 12.0) <= 0.001
    other = torch.empty(n, dtype=torch.float32, device=DEV)
    ops.uniform(other, seed, draw + 1)
    assert float((other == big).double().mean()) < 1e-3


def test_objects_number_their_draws(U):
    from unet_rir_amd import features as F
    name = "11frames"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    geo = dict(des_shape=GC.dims(name), n_fft=n_fft, win_length=win, hop_length=hop)
    feat = torch.tensor(GC.features(name, True, False)).to(DEV)
    g1, g2 = F.GriffinLim(seed=5), F.GriffinLim(seed=5)
    assert g1.algorithm == "gl"
    a = [g1.post_process(feat, **geo).clone() for _ in range(3)]
    b = [g2.post_process(feat, **geo).clone() for _ in range(3)]
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[0], a[1]) and not torch.equal(a[1], a[2]) and not torch.equal(a[0], a[2])
    assert not torch.equal(a[0], F.GriffinLim(seed=6).post_process(feat, **geo))
    assert g1.waveform is not None and g1.waveform.shape == (B, hop * (GC.dims(name)[1] - 1))


def test_layouts(U):
    """[H, W, 2], [B, H, W, 2] and [B, 2, H, W] give the same waveforms; a single feature gives batch[0]; host tensors raise."""
    from unet_rir_amd import features as F
    name = "11frames"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    geo = dict(des_shape=GC.dims(name), n_fft=n_fft, win_length=win, hop_length=hop)
    nchw = torch.tensor(GC.features(name, True, False)).to(DEV)
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    ip = torch.tensor(GC.init_phase(name)).to(DEV)
    want = torch.tensor(GC.reference(name, True, 32, 0.99, "reflect")).float().to(DEV)
    gl = F.GriffinLim()
    a = gl.post_process(nchw, init_phase=ip, **geo).clone()
    b = gl.post_process(nhwc, init_phase=ip, **geo).clone()
    c = gl.post_process(nhwc.permute(0, 3, 1, 2), init_phase=ip, **geo).clone()     # NCHW view, not contiguous
    one = gl.post_process(nhwc[0], None, init_phase=ip[0], **geo)
    assert a.shape == (B, hop * (GC.dims(name)[1] - 1)) and one.shape == a.shape[1:]
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(one, a[0]) and gl.waveform is one
    assert float((a - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert gl.draws == 0                                                            # given phases do not use up a draw
    with pytest.raises(ValueError):
        gl.post_process(nchw.cpu(), **geo)
    with pytest.raises(ValueError):
        gl.post_process(nchw, init_phase=ip.cpu(), **geo)


def test_evaluator_reconstructs_with_griffinlim(U):
    """Evaluator(algorithm='gl').update == update_scored fed with GriffinLim(seed).post_process(pred); 'ph' is unchanged by the
    new argument; any other algorithm raises."""
    from unet_rir_amd import features as F
    B, T = 2, 9600
    g = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randn((B, T), generator=g) * torch.exp(-torch.arange(T) / 700.0)[None, :]).to(DEV)
    y = (torch.randn((B, T), generator=g) * torch.exp(-torch.arange(T) / 500.0)[None, :]).to(DEV)
    spec_in, spec_out = F.PreProcess()(x), F.PreProcess()(y)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=g, dtype=torch.int32).to(DEV)
    m = U.UNet((144, 160, 2), (2, 16), number_filters_0=8, kernels=3, batch_size=B, device=DEV, dropout=False)
    room = ["ShoeBoxRoom", "LargeMeetingRoom"]
    with pytest.raises(ValueError):
        U.Evaluator(m, algorithm="x")
    for diff_gen in (False, True):
        ev = U.Evaluator(m, diff_gen=diff_gen, algorithm="gl", gl_seed=9)
        want = U.Evaluator(m, diff_gen=diff_gen)
        gl = F.GriffinLim(seed=9)
        for _ in range(2):                                                          # two batches: the draw counter advances in step
            ev.update(spec_in, emb, spec_out, y, room)
            with torch.no_grad():
                pred = m.model([spec_in.permute(0, 2, 3, 1), emb], training=False).clone()
            want.update_scored(pred, spec_in, spec_out, gl.post_process(pred).clone(), y, room)
        got, exp = ev.result(), want.result()
        for k in U.evaluate.METRICS + ("n",):
            assert np.array_equal(np.array(got[k]), np.array(exp[k]), equal_nan=True), k
        assert np.isfinite(got["mse_wav"][0]) and got["n"][0] == 2 * B
        # 'ph' with and without the argument
        e1, e2 = U.Evaluator(m, diff_gen=diff_gen, algorithm="ph"), U.Evaluator(m, diff_gen=diff_gen)
        e1.update(spec_in, emb, spec_out, y, room)
        e2.update(spec_in, emb, spec_out, y, room)
        r1, r2 = e1.result(), e2.result()
        for k in U.evaluate.METRICS + ("n",):
            assert np.array_equal(np.array(r1[k]), np.array(r2[k]), equal_nan=True), k
        assert r1["mse_wav"][0] != got["mse_wav"][0]                                # the two reconstructions are different waveforms
