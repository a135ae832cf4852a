"""csrc/resample.hip on the device, element by element against the fp64 restatement of tests/resample_ref.py.

Geometries: ratios L / M with one residue (1 / 2, 1 / 3: lanes spread over periods; an even M takes the padded window), a few (2, 3, 7:
a period per run of lanes, 256 not a multiple of it), and many (160 / 147, 147 / 160: tiles of 32 residues; 441 / 1280: a partial last
tile of 25, windows that fill the LDS); zeros 1, 2, 16 (T from 2 - tail taps only - to 94: T mod 4 = 2) and 64 for 160 / 147 and 1 / 3
(T = 128 and 384); N = 1, 2, T - 1, T, T + 1 (windows that hang over both ends), 1000, 5000, and 20 000 for 160 / 147 at zeros = 16 (more
periods than one workgroup owns); B = 1 and 3; Nout = full, 1 and full - 1.  Every call writes into the middle of a canary-filled buffer,
`out` off 16-byte alignment.

Integer data (table |h| <= 3, |x| <= 7: every partial sum below 21 T < 2^24) must EQUAL the reference - the kernel does not interpret
the table.  Uniform data through a filter-shaped fp32 table must lie within (terms + 2) 2^-24 sum |h x| of the fp64 sum over the same
table: one rounding per accumulated term, whatever the order."""
import os

import numpy as np
import pytest
import torch

import dataset_tree as DT
import resample_ref as RR

pytestmark = pytest.mark.gpu

RATIOS = [(2, 1), (1, 2), (3, 1), (1, 3), (3, 2), (2, 3), (7, 3), (3, 7), (160, 147), (147, 160), (441, 1280)]
GEOMS = [(L, M, z) for L, M in RATIOS for z in (1, 2, 16)] + [(160, 147, 64), (1, 3, 64)]
IDS = [f"{L}-{M}-z{z}" for L, M, z in GEOMS]
CANARY = 12345.678          # no integer, so no sum of integer data
TONE_LIMIT = {"kaiser_best": 1e-7, "kaiser_fast": 2e-4}         # tests/test_resample_ref.py
TONE_AT = {"kaiser_best": (0.05, 0.5, 0.8), "kaiser_fast": (0.05, 0.5)}


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the cached arrays are read-only


def _lengths(L, M, zeros):
    T = RR.taps(L, M, zeros)
    ns = [1, 2, T - 1, T, T + 1, 1000, 5000] + ([20000] if (L, M, zeros) == (160, 147, 16) else [])
    return sorted({n for n in ns if n >= 1})


def _run(x, table, L, M, Nout, pad=(1, 64)):
    """ops.resample_f32 into the middle of a canary-filled buffer (the front pad also puts `out` off 16-byte alignment); returns the
    result on the host after checking that nothing around it was written."""
    import unet_rir_amd as U
    B = x.shape[0]
    buf = torch.full((pad[0] + B * Nout + pad[1],), CANARY, dtype=torch.float32, device="cuda")
    out = buf[pad[0]:pad[0] + B * Nout].view(B, Nout)
    U.ops.resample_f32(x, table, L, M, out)
    host = buf.cpu().numpy()
    assert np.all(host[:pad[0]] == CANARY) and np.all(host[pad[0] + B * Nout:] == CANARY), "written outside out"
    return host[pad[0]:pad[0] + B * Nout].reshape(B, Nout).copy()


def _variants(L, M, zeros, kind):
    """(name, x, table, Nout, reference triple) for every N, B = 1 and 3, Nout = full, 1 and full - 1"""
    for N in _lengths(L, M, zeros):
        table, x, ref = RR.case(L, M, zeros, N, kind)
        td, xd = _dev(table), _dev(x)
        full = ref[0].shape[1]
        assert full == RR.out_length(N, L, M)
        for B in (1, 3):
            for Nout in sorted({full, 1, max(1, full - 1)}):
                yield f"N={N} B={B} Nout={Nout}", xd[:B], td, Nout, tuple(a[:B, :Nout] for a in ref)


@pytest.mark.parametrize("L,M,zeros", GEOMS, ids=IDS)
def test_integer_data_equals_the_reference(L, M, zeros):
    for name, x, table, Nout, (y, _, _) in _variants(L, M, zeros, "int"):
        got = _run(x, table, L, M, Nout)
        assert not np.any(got == CANARY), name                       # every element written
        bad = np.flatnonzero(got.astype(np.float64) != y)
        assert bad.size == 0, (name, bad[:8], got.ravel()[bad[:8]], y.ravel()[bad[:8]])


@pytest.mark.parametrize("L,M,zeros", GEOMS, ids=IDS)
def test_uniform_data_within_one_rounding_per_term(L, M, zeros):
    worst = 0.0
    for name, x, table, Nout, (y, S, terms) in _variants(L, M, zeros, "uniform"):
        got = _run(x, table, L, M, Nout).astype(np.float64)
        assert np.all(np.isfinite(got)) and not np.any(got == CANARY), name
        err, bound = np.abs(got - y), (terms + 2) * 2.0 ** -24 * S
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (name, bad[:8], err.ravel()[bad[:8]], bound.ravel()[bad[:8]])
    print(f"L={L} M={M} zeros={zeros}: worst error / bound = {worst:.3f}")


def test_the_library_table_is_the_builders():
    """`Resampler` uploads what `ops.resample_table` builds (held to the restatement in tests/test_resample_abi.py)"""
    import unet_rir_amd as U
    r = U.Resampler(44100, 48000)
    assert (r.L, r.M, r.taps) == (160, 147, 128) and r.table.is_cuda and r.table.dtype == torch.float32
    zeros, rolloff, beta = RR.PRESETS["kaiser_best"]
    assert torch.equal(r.table.cpu(), U.ops.resample_table(160, 147, zeros, rolloff, beta))
    assert r.out_length(1000) == 1089
    f = U.Resampler(48000, 16000, "kaiser_fast", zeros=8)
    assert (f.L, f.M, f.taps) == (1, 3, 48)


BITS = [(160, 147, 16, 5000), (160, 147, 16, 20000), (1, 3, 64, 5000), (1, 2, 16, 5000), (3, 1, 16, 1000), (441, 1280, 16, 5000),
        (7, 3, 2, 1000)]


@pytest.mark.parametrize("L,M,zeros,N", BITS, ids=[f"{L}-{M}-z{z}-N{N}" for L, M, z, N in BITS])
def test_bits_do_not_depend_on_run_batch_place_or_length(L, M, zeros, N):
    import unet_rir_amd as U
    table, x, ref = RR.case(L, M, zeros, N, "uniform")
    td, xd = _dev(table), _dev(x)
    full_len = ref[0].shape[1]

    def go(xx, Nout=full_len):
        out = torch.empty((xx.shape[0], Nout), dtype=torch.float32, device="cuda")
        U.ops.resample_f32(xx.contiguous(), td, L, M, out)
        return out

    full = go(xd)
    assert torch.equal(go(xd), full)                                                      # two runs
    for b in range(3):
        assert torch.equal(go(xd[b:b + 1]), full[b:b + 1])                                # a row alone against the batch
    assert torch.equal(go(xd.flip(0)), full.flip(0))                                      # its place in the batch
    for Nout in sorted({1, 2, L - 1, L, L + 1, 31, 1024, full_len - 1}):                  # a truncated Nout = the head of the full result
        if 1 <= Nout <= full_len:
            assert torch.equal(go(xd, Nout), full[:, :Nout]), Nout


def test_graph_capture_replays_the_same_bits():
    import unet_rir_amd as U
    L, M, zeros, N = 160, 147, 16, 5000
    table, x, ref = RR.case(L, M, zeros, N, "uniform")
    td, xd = _dev(table), _dev(x)
    eager = torch.empty((3, ref[0].shape[1]), dtype=torch.float32, device="cuda")
    U.ops.resample_f32(xd, td, L, M, eager)
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        U.ops.resample_f32(xd, td, L, M, out)             # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            U.ops.resample_f32(xd, td, L, M, out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


# ---- end to end ----

@pytest.mark.parametrize("res_type", sorted(RR.PRESETS))
@pytest.mark.parametrize("rate_in,rate_out", [(44100, 48000), (48000, 16000)])
def test_resampler_on_tones(rate_in, rate_out, res_type):
    """The tones of tests/test_resample_ref.py through `Resampler`: within the limits of the definition plus the rounding bound of the
    fp32 sum (one rounding per accumulated term, from the fp64 sum over the library's table)."""
    import unet_rir_amd as U
    r = U.Resampler(rate_in, rate_out, res_type)
    L, M, T = r.L, r.M, r.taps
    N = 3 * T + 400
    m = np.arange(RR.out_length(N, L, M))
    q = m * M // L
    keep = (q - T // 2 + 1 >= 0) & (q + T // 2 <= N - 1)
    fracs = TONE_AT[res_type]
    x = np.stack([RR.tone(rate_in, f * min(rate_in, rate_out) / 2.0, N) for f in fracs]).astype(np.float32)
    got = r(torch.from_numpy(x).cuda())
    assert got.shape == (len(fracs), len(m)) and got.dtype == torch.float32
    _, S, terms = RR.resample_ref(x, r.table.cpu().numpy(), L, M)
    got = got.cpu().numpy().astype(np.float64)
    for k, f in enumerate(fracs):
        err = np.abs(got[k] - RR.tone(rate_out, f * min(rate_in, rate_out) / 2.0, len(m)))
        bound = TONE_LIMIT[res_type] + (terms[k] + 2) * 2.0 ** -24 * S[k]
        print(f"{rate_in} -> {rate_out} {res_type} at {f}: worst error {err[keep].max():.3g}, bound there {bound[keep][np.argmax(err[keep])]:.3g}")
        assert np.all(err[keep] <= bound[keep]), (f, float(err[keep].max()))


def test_resample_equals_resampler_and_equal_rates_return_the_input():
    import unet_rir_amd as U
    x = torch.from_numpy(RR.case(160, 147, 16, 5000, "uniform")[1].copy()).cuda()
    for res_type in sorted(RR.PRESETS):
        want = U.Resampler(44100, 48000, res_type)(x)
        assert torch.equal(U.resample(x, 44100, 48000, res_type), want)
        assert torch.equal(U.resample(x, 44100, 48000, res_type), want)                  # the cached plan
        assert torch.equal(U.resample(x, 88200, 96000, res_type), want)                  # the same reduced ratio
        assert torch.equal(U.resample(x[1], 44100, 48000, res_type), want[1:2])          # [N] is one row
        assert torch.equal(U.resample(x, 44100, 48000, res_type, length=77), want[:, :77])
    assert not torch.equal(U.resample(x, 44100, 48000, "kaiser_fast"), U.resample(x, 44100, 48000, "kaiser_best"))
    custom = U.resample(x, 44100, 48000, "kaiser_fast", zeros=8)
    assert torch.equal(custom, U.Resampler(44100, 48000, "kaiser_fast", zeros=8)(x)) and custom.shape == want.shape
    same = U.resample(x, 48000, 48000)
    assert torch.equal(same, x) and same.data_ptr() != x.data_ptr()                       # equal rates: the input's bits, a copy
    out = torch.empty_like(want)
    assert U.resample(x, 44100, 48000, out=out) is out and torch.equal(out, U.Resampler(44100, 48000)(x))
    with pytest.raises(ValueError, match="length"):
        U.resample(x, 44100, 48000, length=want.shape[1] + 1)
    with pytest.raises(ValueError, match="res_type"):
        U.resample(x, 44100, 48000, "sinc_best")


# ---- read_wav and Dataset ----

def test_read_wav_resamples_a_file_at_another_rate(tmp_path):
    import unet_rir_amd as U
    from unet_rir_amd.auralize import write_wav
    rng = np.random.default_rng(11)
    data = (rng.uniform(-0.5, 0.5, size=(11025, 2)) + 0.01).astype(np.float32)            # 0.25 s at 44.1 kHz, two channels
    p = str(tmp_path / "f441.wav")
    write_wav(p, data, 44100)
    with pytest.raises(ValueError, match="44100 Hz, expected 48000 Hz"):
        U.read_wav(p, 48000, 0.2)
    head = data[:8820]                                                                    # 0.2 s at the file's own rate
    for res_type in sorted(RR.PRESETS):
        mono = torch.from_numpy(head.mean(axis=1, dtype=np.float32)).cuda()
        want = U.resample(mono, 44100, 48000, res_type)[0, :9600].cpu().numpy()
        want = want - np.mean(want)
        got = U.read_wav(p, 48000, 0.2, resample=res_type)
        assert got.dtype == np.float32 and got.shape == (9600,) and np.array_equal(got, want)
        both = U.resample(torch.from_numpy(np.ascontiguousarray(head.T)).cuda(), 44100, 48000, res_type)[:, :9600].cpu().numpy()
        both = both - np.mean(both)
        got2 = U.read_wav(p, 48000, 0.2, mono=False, resample=res_type)
        assert got2.shape == (2, 9600) and np.array_equal(got2, both)
    with pytest.raises(ValueError, match="shorter"):
        U.read_wav(p, 48000, 0.3, resample="kaiser_best")                                 # 0.25 s of audio, whatever the rate


def test_dataset_resamples_the_file_at_another_rate(tmp_path):
    import unet_rir_amd as U
    from unet_rir_amd import features as F
    root, name, room = str(tmp_path), "two", "HemiAnechoicRoom"
    a = os.path.join(root, name, DT.rel_path(room, "A", DT.ARRAYS[0], 1, 1))
    b = os.path.join(root, name, DT.rel_path(room, "A", DT.ARRAYS[0], 1, 2))
    DT.write_wav(a, DT.samples(3, 12000, 1, 48000), 48000)
    DT.write_wav(b, DT.samples(4, 11025, 1, 44100), 44100)
    with pytest.raises(ValueError, match="44100 Hz, expected 48000 Hz"):
        U.Dataset(root, name, room=[room], device="cuda:0")
    ds = U.Dataset(root, name, room=[room], device="cuda:0", keep_waveforms=True, resample="kaiser_best")
    assert len(ds) == 2 and ds.files == [a, b] and ds.resample == "kaiser_best"
    raw = DT.samples(4, 11025, 1, 44100)[:8820, 0].astype(np.float32) * np.float32(2.0 ** -15)
    want = U.resample(torch.from_numpy(raw).cuda(), 44100, 48000, "kaiser_best")[0, :9600].cpu().numpy()
    want = want - np.mean(want)
    assert np.array_equal(ds.waveform(1), want) and np.array_equal(ds.waveform(0), U.read_wav(a, 48000, 0.2))
    assert torch.equal(ds.wav_bank.cpu(), torch.from_numpy(np.stack([ds.waveform(0), want])))
    rows = F.PreProcess(remove_mean=False)(torch.from_numpy(np.stack([ds.waveform(0), want])).cuda())
    assert torch.equal(ds.bank, rows)
