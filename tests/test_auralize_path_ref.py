"""tests/auralize_path_ref.py against itself, without a GPU: the gains sum to 1, the fp32 restatement of the kernel's algorithm passes
every check tests/test_auralize_path_gpu.py applies to the kernel, the integer cases meet the condition under which check 3 may be
asked of an fp32 FFT (the restatement's own error times D at most 1 / 8), and every one-line mutation of the restatement misses at
least one check by a factor of 10 or more on every case it applies to."""
import numpy as np
import pytest

from auralize_path_ref import (CASES, INT_CASES, MUTATIONS, P, block_nodes, bound, bound_figure, case, gain32, gains64, int_figure,
                               nodes_ols, path_ols_ref, sharp_figure, single_node)

NAMES = sorted(CASES)


def _layouts(name, kind):
    """(layout, h, x, nodes64, path_ref64) for x per row and x shared"""
    h, x, times, rows, shared = case(name, kind)
    return (("rows", h, x) + rows, ("shared", h, x[0]) + shared)


@pytest.mark.parametrize("name", NAMES)
def test_the_gains_sum_to_one_and_the_kernels_are_their_roundings(name):
    R, K, N, times = CASES[name]
    L = N + K - 1
    g = gains64(times, L)
    assert np.all(np.abs(g.sum(axis=0) - 1.0) <= 2.0 ** -52) and np.all(g >= 0) and np.all((g != 0).sum(axis=0) <= 2)
    n = np.arange(L, dtype=np.int64)
    g32 = np.stack([gain32(n, r, np.asarray(times, dtype=np.int64)) for r in range(R)])
    assert np.all(np.abs(g32 - g) <= 2.0 ** -24) and np.array_equal(g32 == 0, g == 0) and np.array_equal(g32 == 1, g == 1)
    for j in range(-(-L // P)):                                   # no node outside r_lo ... r_hi has a gain in block j
        r_lo, r_hi = block_nodes(times, j)
        blk = g[:, j * P:(j + 1) * P]
        assert not blk[:r_lo].any() and not blk[r_hi + 1:].any(), j
        assert r_hi - r_lo + 1 <= 66


@pytest.mark.parametrize("name", NAMES)
def test_the_restatement_passes_the_checks_of_the_gpu_test(name):
    R, K, N, times = CASES[name]
    for layout, h, x, nodes, ref in _layouts(name, "uniform"):
        got = path_ols_ref(h, x, times)
        assert got.dtype == np.float32 and got.shape == ref.shape
        f1 = bound_figure(got, ref, bound(h, x, times, nodes))
        print(f"case {name} {layout}: error / bound = {f1:.3g}")
        assert f1 <= 1.0
        assert sharp_figure(got, ref, got) <= 1.0                 # of itself: the figure is at most 1 / 4
        y = nodes_ols(h, x)
        for r, idx in single_node(times, N + K - 1):              # check 4: the stationary form's bits where one node has gain 1
            assert np.array_equal(got[:, idx], y[:, r, idx]), (layout, r)
        for L in (1, P + 1):                                      # a truncated L: the head, to the rounding of torch's batched FFTs
            assert np.allclose(path_ols_ref(h, x, times, L=L), got[:, :L], rtol=0, atol=1e-4), L


@pytest.mark.parametrize("name", sorted(INT_CASES))
def test_the_integer_cases_meet_their_condition(name):
    """round(D out) == D y may be asked of the kernel only where the restatement's own error times D is at most 1 / 8."""
    amp, D = INT_CASES[name]
    R, K, N, times = CASES[name]
    assert all(b - a == D for a, b in zip(times, times[1:]))
    for layout, h, x, nodes, ref in _layouts(name, "int"):
        got = path_ols_ref(h, x, times)
        f3 = int_figure(got, ref, D)
        print(f"case {name} {layout}, |h|, |x| <= {amp}: restatement's error times D = {f3 / 2:.3g}")
        assert f3 / 2 <= 0.125
        assert np.array_equal(np.rint(D * got.astype(np.float64)), D * ref)


def _applies(mutation, name):
    R, K, N, times = CASES[name]
    if R == 1:
        return False
    if mutation == "block_anchor":                                # a no-op where the nodes are on block edges; needs distinct anchors
        anchors = [t // P * P for t in times]
        return anchors != list(times) and all(b > a for a, b in zip(anchors, anchors[1:]))
    if mutation == "tail_from_r_minus_2":
        return times[-1] < N + K - 1
    return True


@pytest.mark.parametrize("mutation", MUTATIONS)
@pytest.mark.parametrize("name", NAMES)
def test_every_mutation_misses_a_check_by_a_factor_of_ten(name, mutation):
    if not _applies(mutation, name):
        return
    R, K, N, times = CASES[name]
    for layout, h, x, nodes, ref in _layouts(name, "uniform"):
        good, bad = path_ols_ref(h, x, times), path_ols_ref(h, x, times, mutate=mutation)
        figures = {"bound": bound_figure(bad, ref, bound(h, x, times, nodes)), "sharp": sharp_figure(bad, ref, good)}
        if name in INT_CASES:
            hi, xi, _, rows, shared = case(name, "int")
            xi, refi = (xi, rows[1]) if layout == "rows" else (xi[0], shared[1])
            figures["int"] = int_figure(path_ols_ref(hi, xi, times, mutate=mutation), refi, INT_CASES[name][1])
        print(f"case {name} {layout} {mutation}: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
        assert max(figures.values()) >= 10.0, figures


def test_every_mutation_applies_somewhere():
    assert all(sum(_applies(m, n) for n in NAMES) >= 2 for m in MUTATIONS)
