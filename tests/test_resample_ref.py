"""The fp64 restatement of the resampler's definition (tests/resample_ref.py) pinned on the CPU: against scipy.signal.upfirdn, by the
figures a resampler is judged by (a tone comes out as the same tone, the rows of the table sum to 1, a tone above the new Nyquist
frequency is gone) and by librosa's length rule; and four one-line mutations of it, each of which fails a check named here.  Neither
librosa nor resampy is a dependency: the presets carry resampy's parameters, the definition is the one written down in
include/unetrir.h.  No GPU, no library: tests/test_resample_abi.py and tests/test_resample_gpu.py hold the code to this restatement."""
import numpy as np
import pytest

import resample_ref as RR

RATIOS = [(2, 1), (1, 2), (3, 2), (2, 3), (7, 3), (3, 7), (160, 147), (147, 160)]
RATES = [(44100, 48000), (48000, 44100), (48000, 16000), (16000, 48000)]
TONE_LIMIT = {"kaiser_best": 1e-7, "kaiser_fast": 2e-4}
TONE_AT = {"kaiser_best": (0.05, 0.5, 0.8), "kaiser_fast": (0.05, 0.5)}           # 0.8 lies in kaiser_fast's transition band
ROW_SUM_LIMIT = {"kaiser_best": 1e-7, "kaiser_fast": 2e-4}
LEAK = {"kaiser_best": (1.1, 2e-8), "kaiser_fast": (1.35, 2e-5)}                  # (multiple of the new Nyquist frequency, limit)


def _reduced(rate_in, rate_out):
    g = np.gcd(rate_in, rate_out)
    return rate_out // g, rate_in // g


def _inner(N, L, M, T):
    """The outputs whose whole window lies inside the signal"""
    m = np.arange(RR.out_length(N, L, M))
    q = m * M // L
    return (q - T // 2 + 1 >= 0) & (q + T // 2 <= N - 1)


# ---- the checks, each usable with a mutation of the restatement ----

def check_upfirdn(L, M, res_type, mutation=None):
    """y[m] = sum_n g[m M - n L] x[n]: scipy's upfirdn with g[k] = h(k / L) for |k| < C, zeros in front so that the centre of g is a
    multiple of M (c M): then y[m] = upfirdn[m + c]."""
    from scipy.signal import upfirdn
    zeros, rolloff, beta = RR.PRESETS[res_type]
    C = zeros * max(L, M)
    k = np.arange(-(C - 1), C)
    g = RR.h_ref(k, L, M, zeros, rolloff, beta)
    c = -(-(C - 1) // M)
    g = np.concatenate([np.zeros(c * M - (C - 1)), g])
    x = np.random.default_rng([L, M]).uniform(-1.0, 1.0, size=211)
    want = upfirdn(g, x, up=L, down=M)
    Nout = RR.out_length(len(x), L, M)
    want = np.concatenate([want, np.zeros(max(0, c + Nout - len(want)))])[c:c + Nout]
    got = RR.resample_def(x, L, M, zeros, rolloff, beta, mutation)
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-13, (L, M, res_type, float(np.max(np.abs(got - want))))


def check_tones(rate_in, rate_out, res_type, mutation=None):
    L, M = _reduced(rate_in, rate_out)
    zeros, rolloff, beta = RR.PRESETS[res_type]
    T = RR.taps(L, M, zeros)
    N = 3 * T + 400
    keep = _inner(N, L, M, T)
    table = RR.table_ref(L, M, zeros, rolloff, beta, mutation)
    for frac in TONE_AT[res_type]:
        f = frac * min(rate_in, rate_out) / 2.0
        y = RR.resample_ref(RR.tone(rate_in, f, N), table, L, M, mutation)[0]
        err = float(np.max(np.abs(y - RR.tone(rate_out, f, len(y)))[keep]))
        assert err <= TONE_LIMIT[res_type], (rate_in, rate_out, res_type, frac, err)


def check_row_sums(L, M, res_type, mutation=None):
    zeros, rolloff, beta = RR.PRESETS[res_type]
    dev = float(np.max(np.abs(RR.table_ref(L, M, zeros, rolloff, beta, mutation).sum(axis=1) - 1.0)))
    assert dev <= ROW_SUM_LIMIT[res_type], (L, M, res_type, dev)


def check_leak(res_type, mutation=None):
    """48000 -> 16000: a tone above the new Nyquist frequency of 8 kHz, past the transition band, is gone"""
    L, M = 1, 3
    zeros, rolloff, beta = RR.PRESETS[res_type]
    T = RR.taps(L, M, zeros)
    N = 3 * T + 400
    mult, limit = LEAK[res_type]
    y = RR.resample_ref(RR.tone(48000, mult * 8000.0, N), RR.table_ref(L, M, zeros, rolloff, beta, mutation), L, M, mutation)[0]
    left = float(np.max(np.abs(y)[_inner(N, L, M, T)]))
    assert left <= limit, (res_type, left)


# ---- the restatement passes them ----

@pytest.mark.parametrize("res_type", sorted(RR.PRESETS))
@pytest.mark.parametrize("L,M", RATIOS, ids=[f"{L}-{M}" for L, M in RATIOS])
def test_restatement_equals_upfirdn(L, M, res_type):
    pytest.importorskip("scipy.signal")
    check_upfirdn(L, M, res_type)


@pytest.mark.parametrize("res_type", sorted(RR.PRESETS))
@pytest.mark.parametrize("rate_in,rate_out", RATES, ids=[f"{a}-{b}" for a, b in RATES])
def test_a_tone_comes_out_as_the_same_tone(rate_in, rate_out, res_type):
    check_tones(rate_in, rate_out, res_type)


@pytest.mark.parametrize("res_type", sorted(RR.PRESETS))
@pytest.mark.parametrize("L,M", RATIOS, ids=[f"{L}-{M}" for L, M in RATIOS])
def test_rows_of_the_table_sum_to_one(L, M, res_type):
    check_row_sums(L, M, res_type)


@pytest.mark.parametrize("res_type", sorted(RR.PRESETS))
def test_a_tone_above_the_new_nyquist_frequency_is_gone(res_type):
    check_leak(res_type)


@pytest.mark.parametrize("N", [1, 2, 146, 147, 148, 1000])
def test_output_length_is_librosas(N):
    """librosa.resample: n_samples = int(np.ceil(y.shape[axis] * ratio)) with ratio = float(target_sr) / orig_sr"""
    for rate_in, rate_out in RATES + [(7, 3), (3, 7)]:
        L, M = _reduced(rate_in, rate_out)
        want = int(np.ceil(N * rate_out / rate_in))
        assert RR.out_length(N, L, M) == want
        y = RR.resample_ref(np.ones(N), np.ones((L, 2)), L, M)[0]
        assert y.shape == (want,)


def test_the_table_is_zero_outside_the_support_and_symmetric():
    for L, M in RATIOS:
        zeros, rolloff, beta = RR.PRESETS["kaiser_fast"]
        t = RR.table_ref(L, M, zeros, rolloff, beta)
        T, D, C = t.shape[1], t.shape[1] // 2, zeros * max(L, M)
        k = np.arange(L)[:, None] - (np.arange(T)[None, :] - D + 1) * L
        assert np.all(t[np.abs(k) >= C] == 0.0) and np.all(t[np.abs(k) < C - 1] != 0.0)
        assert abs(t[0, D - 1] - rolloff * min(1.0, L / M)) <= 4e-16    # h(0) = s
        assert np.array_equal(RR.h_ref(np.arange(1, C), L, M, zeros, rolloff, beta), RR.h_ref(-np.arange(1, C), L, M, zeros, rolloff, beta))


# ---- and sees what it is there to see: every mutation fails the check named beside it ----

def test_mutation_phase_from_mL_fails_upfirdn_and_tones():
    pytest.importorskip("scipy.signal")
    for L, M in ((3, 2), (2, 3), (160, 147)):
        with pytest.raises(AssertionError):
            check_upfirdn(L, M, "kaiser_fast", "phase_from_mL")
    with pytest.raises(AssertionError):
        check_tones(44100, 48000, "kaiser_fast", "phase_from_mL")


def test_mutation_window_a_tap_late_fails_upfirdn_and_tones():
    pytest.importorskip("scipy.signal")
    for L, M in RATIOS:
        with pytest.raises(AssertionError):
            check_upfirdn(L, M, "kaiser_fast", "window_a_tap_late")
    with pytest.raises(AssertionError):
        check_tones(48000, 16000, "kaiser_best", "window_a_tap_late")


def test_mutation_no_downsampling_gain_fails_row_sums_and_tones():
    for L, M in ((1, 2), (2, 3), (3, 7), (147, 160)):
        with pytest.raises(AssertionError):
            check_row_sums(L, M, "kaiser_best", "no_downsampling_gain")
    with pytest.raises(AssertionError):
        check_tones(48000, 16000, "kaiser_best", "no_downsampling_gain")
    check_row_sums(3, 2, "kaiser_best", "no_downsampling_gain")        # upsampling has no such gain: the mutation changes nothing


def test_mutation_support_closed_a_tap_wide_fails_upfirdn():
    pytest.importorskip("scipy.signal")
    for L, M in RATIOS:
        for res_type in sorted(RR.PRESETS):
            with pytest.raises(AssertionError):
                check_upfirdn(L, M, res_type, "support_closed_a_tap_wide")


def test_all_mutations_are_covered():
    covered = {n[len("test_mutation_"):].split("_fails_")[0] for n in globals() if n.startswith("test_mutation_")}
    assert covered == set(RR.MUTATIONS)
