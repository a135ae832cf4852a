"""CPU tests of what the FFT form of Griffin-Lim is held to (tests/griffinlim_fft_ref.py): the complex64 restatement against the fp64
yardstick, the margin C of the per-sample check and the tolerance SC_TOL of the convergence check, and the mutations those checks must
catch - over the whole case table of tests/griffinlim_fft_cases.py (11 geometries x n_iter 0, 1, 2, 32 x momentum 0.99, 0 x both pad
modes x both denormalize settings = 352 cases).

Measured here, per row (the restatement is the same bits on every machine), e = max_t |y - y64| / max_t |y64| and
sc = || |stft(y)| - S || / || S ||:

    e(restatement)           2.5e-8 ... 5.8e-5, median 2.1e-7, without momentum or with at most 2 iterations;
                             2.1e-7 ... 3.4e-3, median 5.7e-6, at 32 iterations with momentum 0.99 (largest: rir, raw magnitudes, row 0)
    e(variant) / e(restatement), largest and smallest over all cases and rows
        overlap-add in descending frame order     8.24   0.023     (n128-it32-m0.99-constant-raw)
        the loop on 3 S, scaled back              6.29   0.063
        the loop on 0.7 S, scaled back            7.10   0.10
    C = 16.5 >= 2 x 8.243
    |sc - sc64| / sc64 of the restatement and the three variants, largest: 2.64e-5 (rir-it32-m0.99-reflect-raw)
    SC_TOL = 5.3e-5 >= 2 x 2.64e-5

    what a mutation exceeds the checks by, least over the cases it applies to and their rows: the per-sample check alone, and the
    larger of the two checks (least, median)
        nyquist 0.19 | 11.8  7.0e3      nofold 19.9 | 1.0e4  8.1e4     shift 10.6 | 154  1.1e4
        notprev 14.4 | 803  9.4e3       noenv  14.9 | 506  1.2e5       nohalo 17.7 | 1470  1.2e5

The per-sample check alone lets a dropped bin N/2 pass in a chaotic row (0.19: n1024x4-it32-m0.99-reflect-raw row 1, where the
restatement's own e is 7.9e-4) and is missed by 4.8 only in another; with the convergence check, which does not amplify, every mutation
misses one of the two by a factor of ten at the least in every row, and typically by four orders of magnitude."""
import numpy as np
import pytest

import griffinlim_fft_cases as GC
import griffinlim_fft_ref as FR
import griffinlim_ref as GR

BY_GEOMETRY = {name: [c for c in GC.CASES if c[0] == name] for name in GC.GEOMETRIES}


def test_the_case_table():
    assert len(GC.CASES) == 11 * 4 * 2 * 2 * 2 == len(set(GC.IDS))
    for name, (B, T, n_fft, win, hop) in GC.GEOMETRIES.items():
        nb, nf = GC.dims(name)
        assert hop * (nf - 1) > n_fft // 2 and 4 * hop >= win and hop * nf + n_fft < 2 ** 31 and nb == n_fft // 2 + 1 and nf == 1 + T // hop
        assert GC.features(name, True).shape[2] % 16 == 0 and GC.features(name, True).shape[3] % 16 == 0


@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_restatement_against_fp64(name):
    """the restatement is an fp32 form of the yardstick's loop: exact data flow, rounding apart - e stays at rounding level without
    iterations and within 1e-4 without momentum or with at most 2 iterations, finite, rows different from each other"""
    for case in BY_GEOMETRY[name]:
        ref, y = GC.reference(*case), GC.restated(*case)
        assert y.dtype == np.float32 and y.shape == ref.shape and np.isfinite(y).all()
        assert float(np.abs(ref[0] - ref[1]).max()) > 0.01 * float(np.abs(ref).max())
        e = GC.rel_err(y, ref)
        print(case, e)
        assert (e <= (2e-6 if case[1] == 0 else 1e-4 if case[1] <= 2 or case[2] == 0 else 1e-2)).all() and (e > 0).all(), (case, e)


@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_the_margin_covers_twice_the_spread_of_equally_good_realisations(name):
    worst = 0.0
    for case in BY_GEOMETRY[name]:
        ref = GC.reference(*case)
        e0 = GC.rel_err(GC.restated(*case), ref)
        for v in FR.VARIANTS:
            r = GC.rel_err(GC.restated(*case, variant=v), ref) / e0
            worst = max(worst, float(r.max()))
    print(name, "largest e(variant) / e(restatement)", worst)
    assert 2.0 * worst <= FR.C


@pytest.mark.parametrize("mutation", FR.MUTATIONS)
@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_every_mutation_fails_the_device_checks_on_every_case_it_applies_to(name, mutation):
    """in every row one of the two checks is missed by a factor of ten at the least"""
    least, n = np.inf, 0
    for case in BY_GEOMETRY[name]:
        if not FR.applies(mutation, *case[1:], overlap=GC.overlaps(name)):
            continue
        n += 1
        by_sample, by_convergence = GC.excess(GC.restated(*case, variant=mutation), case)
        least = min(least, float(np.maximum(by_sample, by_convergence).min()))
    print(name, mutation, n, "cases, least excess over what the checks allow", least)
    assert (n > 0 or (mutation == "nohalo" and not GC.overlaps(name))) and least > 10.0


@pytest.mark.parametrize("name", list(GC.GEOMETRIES))
def test_the_convergence_tolerance_covers_twice_the_spread_of_equally_good_realisations(name):
    worst = 0.0
    for case in BY_GEOMETRY[name]:
        for v in (None,) + FR.VARIANTS:
            worst = max(worst, float(GC.excess(GC.restated(*case, variant=v), case)[1].max()) * FR.SC_TOL)
    print(name, "largest |sc - sc64| / sc64 of the four fp32 realisations", worst)
    assert 2.0 * worst <= FR.SC_TOL


def test_spectral_convergence_of_the_two_precisions_agrees():
    """fp32 costs no reconstruction quality: || |stft(y)| - S || / || S || of the complex64 result is that of the fp64 result to 1 %
    (measured: equal to four decimals)"""
    for name in ("rir", "18frames"):
        B, T, n_fft, win, hop = GC.GEOMETRIES[name]
        case = (name, 32, 0.99, "reflect", True)
        S = GC.magnitude(name, True)
        for b in range(B):
            c64 = GR.spectral_convergence(GC.reference(*case)[b], S[b], n_fft, win, hop)
            c32 = GR.spectral_convergence(GC.restated(*case)[b].astype(np.float64), S[b], n_fft, win, hop)
            print(name, b, c64, c32)
            assert abs(c32 - c64) <= 0.01 * c64
