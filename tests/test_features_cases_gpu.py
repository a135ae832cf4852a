"""GPU tests of the waveform <-> feature kernels (csrc/features.hip) per element against the fp64 oracle, over the case table of
tests/features_cases.py with the bounds of tests/features_check.py (derived there; measured on the CPU, never on a kernel).

Every test goes through ops.stft_features / ops.istft_features, and again through PreProcess / FeatureExtractor / PostProcess
where those expose the mode: the classes launch the same kernel with the same arguments, so their result is held to the
checked one bit for bit.  Outputs are carved out of a larger buffer with a canary either side."""
import os
import sys

import numpy as np
import pytest
import torch

import features_cases as FC
import features_check as FK
from oracle import features as FO

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_features_golden as MFG  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 1234.5
GUARD = 1024            # floats either side of an output


@pytest.fixture(scope="module")
def U():
    import unet_rir_amd
    return unet_rir_amd


class Guarded:
    """An fp32 output of `shape` filled with NaN (an element the kernel leaves out shows) between two canary regions."""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.big = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.float32, device=DEV)
        self.out = self.big[GUARD:GUARD + n].view(shape)
        self.out.fill_(float("nan"))

    def result(self):
        torch.cuda.synchronize()
        assert bool((self.big[:GUARD] == CANARY).all()) and bool((self.big[GUARD + self.out.numel():] == CANARY).all())
        return self.out


def geometry(name):
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    return dict(n_fft=n_fft, win_length=win, hop_length=hop)


def stft(U, x, name, tight, pad_mode, remove_mean, normalize):
    g = Guarded((x.shape[0], 2) + FC.shape(name, tight))
    U.ops.stft_features(x, g.out, pad_mode=pad_mode, remove_mean=remove_mean, normalize=normalize, **geometry(name))
    return g.result()


def istft(U, feat, name, denormalize):
    nb, nf = FC.dims(name)
    g = Guarded((feat.shape[0], FC.t_out(name)))
    U.ops.istft_features(feat, g.out, nb, nf, denormalize=denormalize, **geometry(name))
    return g.result()


def split(out, name):
    """[B, 2, H, W] device planes -> (amp, phase) fp32 numpy [B, n_bins, n_frames]; the appended rows and columns are zero"""
    nb, nf = FC.dims(name)
    o = out.cpu().numpy()
    assert not o[:, :, nb:, :].any() and not o[:, :, :, nf:].any()
    return np.ascontiguousarray(o[:, 0, :nb, :nf]), np.ascontiguousarray(o[:, 1, :nb, :nf])


MODES = [(True, True), (False, True), (True, False), (False, False)]


@pytest.mark.parametrize("remove_mean,normalize", MODES, ids=["mean-norm", "norm", "mean-raw", "raw"])
@pytest.mark.parametrize("pad_mode", FC.PAD_MODES)
@pytest.mark.parametrize("name,tight", FC.LAYOUTS, ids=FC.LAYOUT_IDS)
def test_analysis_parity_per_element(U, name, tight, pad_mode, remove_mean, normalize):
    from unet_rir_amd import features as F
    S, l1, silent, mirror = FC.analysis(name, "noise", pad_mode, remove_mean)
    x = torch.tensor(FC.waves(name)).to(DEV)
    out = stft(U, x, name, tight, pad_mode, remove_mean, normalize)
    amp, ph = split(out, name)
    FK.check_planes(f"{name} {pad_mode} mean={remove_mean}", amp, ph, S, l1, normalize, silent, mirror)
    geo = tuple(geometry(name).values())
    if normalize:
        g = Guarded(tuple(out.shape))
        got = F.PreProcess(*geo, desired_shape=FC.shape(name, tight), pad_mode=pad_mode, remove_mean=remove_mean)(x, out=g.out)
        assert got is g.out and torch.equal(g.result(), out)
    elif not remove_mean:
        a, p = F.FeatureExtractor(*geo, pad_mode=pad_mode).extract(x)
        assert np.array_equal(a.cpu().numpy(), amp) and np.array_equal(p.cpu().numpy(), ph)


@pytest.mark.parametrize("normalize", [True, False], ids=["norm", "raw"])
@pytest.mark.parametrize("pad_mode", FC.PAD_MODES)
@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_exact_zeros(U, name, pad_mode, normalize):
    """remove_mean=False on a waveform that begins with silence and on an all-zero one: every bin of a silent frame has phase
    exactly 0.5 (0 raw) and an amplitude within the bound; the DC and Nyquist rows equal the oracle's fp32 phases."""
    from unet_rir_amd import features as F
    S, l1, silent, mirror = FC.analysis(name, "zeros", pad_mode, False)
    x = torch.tensor(FC.waves(name, "zeros")).to(DEV)
    out = stft(U, x, name, False, pad_mode, False, normalize)
    amp, ph = split(out, name)
    FK.check_planes(f"{name} {pad_mode} zeros", amp, ph, S, l1, normalize, silent, mirror)
    rest = np.float32(0.5 if normalize else 0.0)
    assert silent[1].all() and (ph[1] == rest).all() and (ph[0][:, silent[0]] == rest).all() and silent[0].any()
    if normalize:
        got = F.PreProcess(*geometry(name).values(), desired_shape=FC.shape(name, False), pad_mode=pad_mode, remove_mean=False)(x)
        assert torch.equal(got, out)


@pytest.mark.parametrize("kind", FC.PLANE_KINDS)
@pytest.mark.parametrize("name,tight", FC.LAYOUTS, ids=FC.LAYOUT_IDS)
def test_synthesis_parity_per_sample(U, name, tight, kind):
    from unet_rir_amd import features as F
    y, A, env = FC.synthesis(name, kind)
    dirty = torch.tensor(FC.planes(name, kind, tight, True)).to(DEV)
    wav = istft(U, dirty, name, kind != "raw")
    FK.check_wave(f"{name} {kind}", wav.cpu().numpy(), y, A, env)
    assert int((env <= FO.TINY32).sum()) == FC.ZERO_ENVELOPE.get(name, 0)
    # un_pad: the rubbish in the appended rows and columns does not reach the waveform
    clean = torch.tensor(FC.planes(name, kind, tight, False)).to(DEV)
    assert torch.equal(istft(U, clean, name, kind != "raw"), wav)
    if kind != "raw":
        g = Guarded(tuple(wav.shape))
        got = F.PostProcess().post_process(dirty, des_shape=FC.dims(name), out=g.out, **geometry(name))
        assert got is g.out and torch.equal(g.result(), wav)


@pytest.mark.parametrize("name", list(FC.GEOMETRIES))
def test_deterministic_and_independent_of_the_batch(U, name):
    """Two runs give the same bits, and row b of a batch equals the same waveform (feature) run alone, from where it lies in the
    batch: for "oddwin" that row starts 812 bytes in, off a 16-byte boundary, and so does its output row."""
    B = FC.GEOMETRIES[name][0]
    x = torch.tensor(FC.waves(name)).to(DEV)
    feat = torch.tensor(FC.planes(name, "range", False, True)).to(DEV)
    a = stft(U, x, name, False, "reflect", True, True)
    w = istft(U, feat, name, True)
    assert torch.equal(a, stft(U, x, name, False, "reflect", True, True)) and torch.equal(w, istft(U, feat, name, True))
    nb, nf = FC.dims(name)
    for b in range(B):
        assert torch.equal(stft(U, x[b:b + 1], name, False, "reflect", True, True), a[b:b + 1])
        g = Guarded((B, FC.t_out(name)))
        U.ops.istft_features(feat[b:b + 1], g.out[b:b + 1], nb, nf, denormalize=True, **geometry(name))
        assert torch.equal(g.result()[b], w[b])
        assert bool(torch.isnan(g.out[:b]).all()) and bool(torch.isnan(g.out[b + 1:]).all())       # the other rows are untouched
    if name == "oddwin":
        assert x[1:2].data_ptr() % 16 != 0


def test_post_process_layouts_give_the_same_bits(U):
    from unet_rir_amd import features as F
    name = "oddwin"
    kw = dict(des_shape=FC.dims(name), **geometry(name))
    nchw = torch.tensor(FC.planes(name, "range", False, True)).to(DEV)
    nhwc = nchw.permute(0, 2, 3, 1).contiguous()
    want = istft(U, nchw, name, True)
    post = F.PostProcess()
    assert torch.equal(post.post_process(nchw, **kw), want)
    assert torch.equal(post.post_process(nhwc, **kw), want)
    for b in range(nchw.shape[0]):
        one = post.post_process(nhwc[b], **kw)
        assert one.shape == (FC.t_out(name),) and torch.equal(one, want[b])


@pytest.mark.parametrize("name", ["oddwin", "hop96"])
def test_round_trip(U, name):
    """istft(stft(x)) == x - mean(x) on the samples whose envelope exceeds 1e-3, independent of the FFT oracle's transforms: the
    allowance is the synthesis bound plus the analysis bounds of the two fp32 planes carried through the absolute-value twin
    of the synthesis sum (their sizes, not the comparison's target, use the oracle's |S|)."""
    B, T, n_fft, win, hop = FC.GEOMETRIES[name]
    S, l1, silent, mirror = FC.analysis(name, "noise", "reflect", True)
    x = torch.tensor(FC.waves(name)).to(DEV)
    feat = stft(U, x, name, False, "reflect", True, True)
    wav = istft(U, feat, name, True).cpu().numpy()
    x64 = FC.waves(name).astype(np.float64)
    want = (x64 - x64.mean(axis=1, keepdims=True))[:, :FC.t_out(name)]
    env = FK.envelope(FC.dims(name)[1], n_fft, win, hop)
    A = np.stack([FK.abs_synthesis(np.abs(S[b]), n_fft, win, hop) for b in range(B)])
    carried = np.stack([FK.abs_synthesis(FK.plane_error_as_complex(S, l1)[b], n_fft, win, hop) for b in range(B)])
    live = env > 1e-3
    assert live.sum() >= 0.9 * live.size
    FK.check_wave(f"{name} round trip", np.ascontiguousarray(wav[:, live]), want[:, live], A[:, live], env[live], carried[:, live])


@pytest.mark.parametrize("name", list(MFG.CASES))
def test_golden_geometries_per_element(U, name):
    """The two geometries of the committed goldens (tests/test_features_gpu.py) through the per-element check as well."""
    B, T, n_fft, win, hop, shape, pad_mode = MFG.CASES[name]
    x32 = MFG.waveforms(name).astype(np.float32)
    x = torch.tensor(x32).to(DEV)
    for remove_mean, normalize in ((True, True), (False, False)):
        S, l1, silent, mirror = [], [], [], []
        for b in range(B):
            y = x32[b].astype(np.float64)
            S.append(FO.stft(y - y.mean() if remove_mean else y, n_fft, win, hop, pad_mode))
            a, s, m = FK.frame_stats(x32[b], n_fft, win, hop, pad_mode, remove_mean)
            l1.append(a), silent.append(s), mirror.append(m)
        out = torch.full((B, 2) + tuple(shape), float("nan"), dtype=torch.float32, device=DEV)
        U.ops.stft_features(x, out, n_fft, win, hop, pad_mode, remove_mean, normalize)
        o = out.cpu().numpy()
        nb, nf = n_fft // 2 + 1, 1 + T // hop
        assert not o[:, :, nb:, :].any() and not o[:, :, :, nf:].any()
        FK.check_planes(f"{name} mean={remove_mean}", np.ascontiguousarray(o[:, 0, :nb, :nf]), np.ascontiguousarray(o[:, 1, :nb, :nf]),
                        np.stack(S), np.stack(l1), normalize, np.stack(silent), np.stack(mirror))
