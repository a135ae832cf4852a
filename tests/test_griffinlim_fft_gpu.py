"""GPU tests of the FFT form of Griffin-Lim (csrc/griffinlim_fft.hip through ops.griffinlim_fft, features.GriffinLim(method="fft") and
Evaluator(algorithm="gl", gl_method="fft")).

The iteration amplifies rounding, so there is no bound per element.  Per row, with e(y) = max_t |y - y64| / max_t |y64| and
sc(y) = || |stft(y)| - S || / || S || (fp64, on the host) against the fp64 yardstick tests/griffinlim_ref.py on the same fp32 inputs, the
device is held to

    e(kernel) <= C e(complex64 restatement on the same data) + 2^-22,     C = 16.5
    |sc(kernel) - sc(y64)| <= SC_TOL sc(y64),                             SC_TOL = 5.3e-5

C is twice the largest factor (8.24) by which two equally good fp32 realisations of the loop differ in e on the CPU over this case table:
the restatement against itself with the overlap-add in descending frame order (8.24), on 3 S scaled back (6.29) and on 0.7 S scaled back
(7.10).  SC_TOL is twice the largest relative distance (2.64e-5) of those four realisations' sc from the yardstick's; it holds the rows
where 32 iterations with momentum have made the per-sample check loose (allowances up to 5 % of the peak).
tests/test_griffinlim_fft_ref.py measures both and shows that every structural mistake misses one of the two checks by a factor of ten
at the least in every row it applies to, typically by four orders of magnitude.  Nothing here is measured on a kernel; what the kernels
then gave on an MI355X over the 352 cases: e 3.6e-8 ... 9.7e-4, at most 0.40 of the allowance, and |sc - sc64| / sc64 at most 1.9e-5
(median 1.4e-8)."""
import numpy as np
import pytest
import torch

import griffinlim_fft_cases as GC
import griffinlim_fft_ref as FR
import griffinlim_ref as GR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 0xA5


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


def geo_of(name):
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    return GC.dims(name) + (n_fft, win, hop)


def run(U, name, n_iter=32, momentum=0.99, pad_mode="reflect", denormalize=True, init_phase="given", seed=0, draw=0, ws=None, rows=None,
        wav=None):
    ops = U.ops
    nb, nf, n_fft, win, hop = geo_of(name)
    feat = torch.tensor(GC.features(name, denormalize))
    ip = torch.tensor(GC.init_phase(name)) if isinstance(init_phase, str) else init_phase
    if rows is not None:
        feat = feat[rows].contiguous()
        ip = ip[rows].contiguous() if ip is not None else None
    if wav is None:
        wav = torch.full((feat.shape[0], hop * (nf - 1)), float("nan"), dtype=torch.float32, device=DEV)
    ops.griffinlim_fft(feat.to(DEV), wav, nb, nf, n_fft, win, hop, ws if ws is not None else ops.Workspace(DEV), pad_mode=pad_mode,
                       denormalize=denormalize, n_iter=n_iter, momentum=momentum, init_phase=ip.to(DEV) if ip is not None else None,
                       seed=seed, draw=draw)
    return wav


@pytest.mark.parametrize("case", GC.CASES, ids=GC.IDS)
def test_every_row_against_fp64(U, case):
    name, n_iter, momentum, pad_mode, denormalize = case
    ref = GC.reference(*case)
    got = run(U, name, n_iter, momentum, pad_mode, denormalize).cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()                           # a NaN left over: a sample not written
    assert float(np.abs(got[0] - got[1]).max()) > 0.01 * float(np.abs(ref).max())      # the rows of a batch differ
    e, e_rs, tol = GC.rel_err(got, ref), GC.rel_err(GC.restated(*case), ref), GC.allowed(case)
    c, c64 = GC.convergence(got, case), GC.reference_convergence(case)
    print(f"{GC.IDS[GC.CASES.index(case)]}: e(kernel) {e} e(restatement) {e_rs} allowed {tol}; |sc - sc64| / sc64 {np.abs(c - c64) / c64}")
    assert (e <= tol).all()
    assert (np.abs(c - c64) <= FR.SC_TOL * c64).all()


@pytest.mark.parametrize("name", ["rir", "18frames"])
def test_reconstruction_quality_is_that_of_the_dft_form(U, name):
    """32 iterations, momentum 0.99: || |stft(y)| - S || / || S ||, in fp64 on the host, of this form's waveform is within 1 % of the DFT
    form's on the same inputs"""
    ops = U.ops
    nb, nf, n_fft, win, hop = geo_of(name)
    fft = run(U, name).cpu().numpy().astype(np.float64)
    feat, ip = torch.tensor(GC.features(name, True)).to(DEV), torch.tensor(GC.init_phase(name)).to(DEV)
    dft = torch.full((feat.shape[0], hop * (nf - 1)), float("nan"), dtype=torch.float32, device=DEV)
    ops.griffinlim(feat, dft, nb, nf, n_fft, win, hop, ops.Workspace(DEV), init_phase=ip)
    dft = dft.cpu().numpy().astype(np.float64)
    S = GC.magnitude(name, True)
    for b in range(S.shape[0]):
        c_fft = GR.spectral_convergence(fft[b], S[b], n_fft, win, hop)
        c_dft = GR.spectral_convergence(dft[b], S[b], n_fft, win, hop)
        print(f"{name} b={b}: spectral convergence fft {c_fft:.6f} dft {c_dft:.6f}")
        assert np.isfinite(c_fft) and abs(c_fft - c_dft) <= 0.01 * c_dft


@pytest.mark.parametrize("name", ["18frames", "fullwin", "n1024", "rir", "n1024x4", "n512x4", "gaps"])
def test_bits_depend_neither_on_the_run_nor_on_the_batch(U, name):
    a = run(U, name)
    assert torch.equal(a, run(U, name)) and bool(torch.isfinite(a).all())
    for b in range(a.shape[0]):
        assert torch.equal(run(U, name, rows=[b])[0], a[b]), b
    rows = [a.shape[0] - 1, 0, a.shape[0] - 1]
    again = run(U, name, rows=rows)
    assert all(torch.equal(again[i], a[r]) for i, r in enumerate(rows))


def test_capturable(U):
    """the call captured in a HIP graph and replayed twice gives the eager bits"""
    ops = U.ops
    name = "rir"
    nb, nf, n_fft, win, hop = geo_of(name)
    B = GC.GEOMETRIES[name][0]
    a = run(U, name)
    feat = torch.tensor(GC.features(name, True)).to(DEV)
    ip = torch.tensor(GC.init_phase(name)).to(DEV)
    wav = torch.zeros((B, hop * (nf - 1)), dtype=torch.float32, device=DEV)
    ws = ops.Workspace(DEV, ops.griffinlim_fft_ws_bytes(B, nb, nf, n_fft, win, hop))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.griffinlim_fft(feat, wav, nb, nf, n_fft, win, hop, ws, init_phase=ip)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.griffinlim_fft(feat, wav, nb, nf, n_fft, win, hop, ws, init_phase=ip)
    for _ in range(2):
        wav.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(wav, a)


def test_random_initial_phases(U):
    ops = U.ops
    name = "18frames"
    B = GC.GEOMETRIES[name][0]
    nb, nf = GC.dims(name)
    seed, draw = 7, 3
    u = torch.empty((B, nb, nf), dtype=torch.float32, device=DEV)
    ops.uniform(u, seed, draw)
    drawn = run(U, name, init_phase=None, seed=seed, draw=draw)
    assert bool(torch.isfinite(drawn).all())
    assert torch.equal(drawn, run(U, name, init_phase=u.cpu()))
    assert not torch.equal(drawn, run(U, name, init_phase=None, seed=seed, draw=draw + 1))
    assert not torch.equal(drawn, run(U, name, init_phase=None, seed=seed + 1, draw=draw))


def test_workspace_is_exactly_the_advertised_size_and_the_waveform_sits_between_canaries(U):
    ops, L = U.ops, U._lib.lib()
    name = "18frames"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    nb, nf = GC.dims(name)
    adv = ops.griffinlim_fft_ws_bytes(B, nb, nf, n_fft, win, hop)
    assert adv == (7 * B * nf * nb * 4 + 7) // 8 * 8
    big = torch.full((adv + (1 << 20),), CANARY, dtype=torch.uint8, device=DEV)
    ws = ops.Workspace(DEV)
    ws.buf = big[:adv]
    n = B * T
    guard = 4096
    flat = torch.full((n + 2 * guard,), float("nan"), dtype=torch.float32, device=DEV)
    flat.view(torch.int32)[:guard] = 0x5A5A5A5A
    flat.view(torch.int32)[guard + n:] = 0x5A5A5A5A
    wav = flat[guard:guard + n].view(B, T)
    got = run(U, name, ws=ws, wav=wav)
    torch.cuda.synchronize()
    assert ws.buf.data_ptr() == big.data_ptr() and ws.nbytes == adv                    # the wrapper asked for no more
    assert bool((big[adv:] == CANARY).all())
    assert bool((flat.view(torch.int32)[:guard] == 0x5A5A5A5A).all()) and bool((flat.view(torch.int32)[guard + n:] == 0x5A5A5A5A).all())
    assert bool(torch.isfinite(got).all()) and torch.equal(got, run(U, name))
    feat = torch.tensor(GC.features(name, True)).to(DEV)
    out = torch.empty((B, T), dtype=torch.float32, device=DEV)
    args = (feat.data_ptr(), B, feat.shape[2], feat.shape[3], nb, nf, n_fft, win, hop, 0, 1, 2, 0.99, None, 0, 0, out.data_ptr(),
            big.data_ptr())
    assert L.unetrir_griffinlim_fft_f32(*args, adv - 1, None) == 10001
    assert L.unetrir_griffinlim_fft_f32(*args, adv, None) == 0
    torch.cuda.synchronize()
    assert bool((big[adv:] == CANARY).all())


def test_griffinlim_object(U):
    """GriffinLim(method="fft"): [H, W, 2], [B, H, W, 2] and [B, 2, H, W] give the same bits, a single feature gives batch[0]; two objects
    with one seed number their draws alike; an unsupported geometry raises and names method="dft"; method="dft" through the new
    argument gives the bits of the object without it"""
    from unet_rir_amd import features as F
    name = "18frames"
    B, T, n_fft, win, hop = GC.GEOMETRIES[name]
    geo = dict(des_shape=GC.dims(name), n_fft=n_fft, win_length=win, hop_length=hop)
    nchw = torch.tensor(GC.features(name, True)).to(DEV)
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    ip = torch.tensor(GC.init_phase(name)).to(DEV)
    gl = F.GriffinLim(method="fft")
    a = gl.post_process(nchw, init_phase=ip, **geo).clone()
    b = gl.post_process(nhwc, init_phase=ip, **geo).clone()
    c = gl.post_process(nhwc.permute(0, 3, 1, 2), init_phase=ip, **geo).clone()         # NCHW view, not contiguous
    one = gl.post_process(nhwc[0], None, init_phase=ip[0], **geo)
    assert a.shape == (B, T) and one.shape == a.shape[1:]
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(one, a[0]) and gl.waveform is one
    assert torch.equal(a, run(U, name)) and gl.draws == 0                               # the op's bits; given phases use up no draw
    mine = torch.full((B, T), float("nan"), dtype=torch.float32, device=DEV)
    assert gl.post_process(nchw, init_phase=ip, out=mine, **geo) is mine and torch.equal(mine, a)
    g1, g2 = F.GriffinLim(seed=5, method="fft"), F.GriffinLim(seed=5, method="fft")
    x = [g1.post_process(nchw, **geo).clone() for _ in range(3)]
    y = [g2.post_process(nchw, **geo).clone() for _ in range(3)]
    assert all(torch.equal(p, q) for p, q in zip(x, y)) and g1.draws == 3
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2]) and not torch.equal(x[0], x[2])
    assert not torch.equal(x[0], F.GriffinLim(seed=6, method="fft").post_process(nchw, **geo))
    assert torch.equal(x[1], run(U, name, init_phase=None, seed=5, draw=1))
    # the same draws feed both forms: the two waveforms are the same reconstruction, not the same bits
    d = [F.GriffinLim(seed=5, **kw).post_process(nchw, **geo).clone() for kw in (dict(), dict(method="dft"))]
    assert torch.equal(d[0], d[1]) and not torch.equal(d[0], x[0])
    small = torch.zeros((1, 2, 48, 16), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match=r'n_fft 64.*method="dft"'):
        F.GriffinLim(method="fft").post_process(small, des_shape=(33, 11), n_fft=64, win_length=32, hop_length=16)
    assert F.GriffinLim().post_process(small, des_shape=(33, 11), n_fft=64, win_length=32, hop_length=16).shape == (1, 160)


def test_evaluator_reconstructs_with_the_fft_form(U):
    """Evaluator(algorithm="gl", gl_method="fft").update == update_scored fed with GriffinLim(seed, method="fft").post_process(pred)"""
    from unet_rir_amd import features as F
    B, T = 2, 9600
    g = torch.Generator(device="cpu").manual_seed(11)
    x = (torch.randn((B, T), generator=g) * torch.exp(-torch.arange(T) / 700.0)[None, :]).to(DEV)
    y = (torch.randn((B, T), generator=g) * torch.exp(-torch.arange(T) / 500.0)[None, :]).to(DEV)
    spec_in, spec_out = F.PreProcess()(x), F.PreProcess()(y)
    emb = torch.randint(26, 1282, (B, 2, 16), generator=g, dtype=torch.int32).to(DEV)
    m = U.UNet((144, 160, 2), (2, 16), number_filters_0=8, kernels=3, batch_size=B, device=DEV, dropout=False)
    room = ["ShoeBoxRoom", "LargeMeetingRoom"]
    ev = U.Evaluator(m, algorithm="gl", gl_seed=9, gl_method="fft")
    want = U.Evaluator(m)
    other = U.Evaluator(m, algorithm="gl", gl_seed=9)
    gl = F.GriffinLim(seed=9, method="fft")
    for _ in range(2):                                                                  # two batches: the draw counter advances in step
        ev.update(spec_in, emb, spec_out, y, room)
        other.update(spec_in, emb, spec_out, y, room)
        with torch.no_grad():
            pred = m.model([spec_in.permute(0, 2, 3, 1), emb], training=False).clone()
        want.update_scored(pred, spec_in, spec_out, gl.post_process(pred).clone(), y, room)
    got, exp, dft = ev.result(), want.result(), other.result()
    for k in U.evaluate.METRICS + ("n",):
        assert np.array_equal(np.array(got[k]), np.array(exp[k]), equal_nan=True), k
    assert np.isfinite(got["mse_wav"][0]) and got["n"][0] == 2 * B
    assert got["mse_wav"][0] != dft["mse_wav"][0]                                       # another kernel, other bits
