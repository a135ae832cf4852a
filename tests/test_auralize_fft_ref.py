"""tests/auralize_fft_ref.py - the partitioned overlap-save formulation restated with torch's CPU FFTs - against the fp64 double sum of
tests/auralize_ref.py, and two guards against a bound that checks nothing: integer data must round to the exact result at EVERY
element, and each deliberate mutation of the restatement must break the bound somewhere."""
import numpy as np
import pytest

from auralize_fft_ref import MUTATIONS, bound, ols_ref
from auralize_ref import case

GEOMS = [(9600, 5000), (1025, 17000), (16384, 3000), (33, 1000), (2049, 2047)]
BLOCKS = (2048, 4096)
IDS = [f"K{K}-N{N}" for K, N in GEOMS]


def _layouts(K, N, kind):
    """(name, h, x, reference y) for x per row and x shared"""
    h, x, rows, shared = case(K, N, kind)
    return (("rows", h, x, rows[0]), ("shared", h, x[0], shared[0]))


@pytest.mark.parametrize("P", BLOCKS)
@pytest.mark.parametrize("K,N", GEOMS, ids=IDS)
def test_restatement_within_the_bound_on_uniform_data(K, N, P):
    for name, h, x, y in _layouts(K, N, "uniform"):
        got = ols_ref(h, x, P).astype(np.float64)
        err, lim = np.abs(got - y), bound(h, x, P)
        assert got.shape == y.shape and np.all(lim > 0)
        print(f"K={K} N={N} P={P} {name}: max error {err.max():.3g}, worst error / bound {np.max(err / lim):.3g}")
        bad = np.flatnonzero(err > lim)
        assert bad.size == 0, (name, bad[:8], err.ravel()[bad[:8]], lim.ravel()[bad[:8]])


@pytest.mark.parametrize("P", BLOCKS)
@pytest.mark.parametrize("K,N", GEOMS, ids=IDS)
def test_integer_data_rounds_to_the_exact_result_everywhere(K, N, P):
    for name, h, x, y in _layouts(K, N, "int"):
        got = ols_ref(h, x, P).astype(np.float64)
        print(f"K={K} N={N} P={P} {name}: max error {np.abs(got - y).max():.3g}")
        bad = np.flatnonzero(np.rint(got) != y)
        assert bad.size == 0, (name, bad[:8], got.ravel()[bad[:8]], y.ravel()[bad[:8]])


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("K,N", GEOMS, ids=IDS)
def test_every_mutation_breaks_the_bound(K, N, mutation):
    P = 2048
    for name, h, x, y in _layouts(K, N, "uniform"):
        err = np.abs(ols_ref(h, x, P, mutate=mutation).astype(np.float64) - y)
        assert np.any(err > bound(h, x, P)), (name, mutation)


def test_a_truncated_length_is_the_head_of_the_full_result_and_of_its_bound():
    h, x, _, _ = case(2049, 2047, "uniform")
    full, lim = ols_ref(h, x, 2048), bound(h, x, 2048)
    for L in (1, 2047, 2048, 2049, 4095):
        assert np.array_equal(ols_ref(h, x, 2048, L=L), full[:, :L]) and np.array_equal(bound(h, x, 2048, L=L), lim[:, :L])
