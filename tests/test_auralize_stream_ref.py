"""tests/auralize_stream_ref.py against the one-shot restatements, without a GPU.

The streaming restatement (ring with i mod S, carry, counter, fade on the first block of a push) is held
- in fp64 to the definition: the plain convolution of the concatenated input (tests/auralize_ref.convolve_ref) and, with updates,
  tests/auralize_path_ref.path_ref64 piecewise, within 2^-40 of the row's peak (fp64 FFTs of 4096 points: some 2^-48);
- in fp32 to tests/auralize_fft_ref.ols_ref and tests/auralize_path_ref.path_ols_ref piecewise with ==: the same transforms of the same
  windows, the same products in the same order.
Every mutation of MUTATIONS must miss BOTH: it changes bits, and its fp64 error is beyond the tolerance by the factor printed.

Factors by which the mutations fail (fp64 error over the 2^-40 tolerance; the unmutated restatement is at 0.0042),
K = 4097, B = 2, max_blocks = 3, pushes of 3, 1, 2 blocks, updates at blocks 3 and 4:
    ring_short 1.9e10    stale_carry 6.9e11    fade_second_block 1.3e12    early_switch 1.5e12
and 4096, 32008, 8190 and 8192 of the 45056 fp32 samples lose their bits
(all are errors of the size of the signal itself: a wrong spectrum, wrong samples, or the wrong response for a whole block)."""
import functools

import numpy as np
import pytest

from auralize_fft_ref import ols_ref
from auralize_path_ref import path_ols_ref, path_ref64
from auralize_ref import convolve_ref
from auralize_stream_ref import MUTATIONS, P, piecewise, run

TOL = 2.0 ** -40


@pytest.fixture(autouse=True)
def one_thread():
    """torch divides a large elementwise product among its threads at arbitrary elements, and the vector body and the scalar tail of
    each share round a complex product differently in rare elements: the bits of ols_ref depend on the thread count.  On one thread
    every row of P + 1 bins is walked alike, by ols_ref and by the streaming restatement."""
    import torch
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _data(K, blocks, B=2, seed=0):
    rng = np.random.default_rng([11, K, blocks, seed])
    return (rng.uniform(-1, 1, size=(B, K)).astype(np.float32), rng.uniform(-1, 1, size=(B, blocks * P)).astype(np.float32))


def _rel(got, ref):
    return float(np.max(np.abs(got.astype(np.float64) - ref).max(axis=1) / np.abs(ref).max(axis=1)))


# K, max_blocks, pushes: total blocks 2 S + 1, so the ring wraps twice
STATIONARY = [(1, 1, (1,)), (2047, 2, (2, 1)), (2049, 2, (1, 2)), (4097, 3, (3, 1, 2)), (9600, 2, (2, 2, 1))]


@pytest.mark.parametrize("K, mb, pushes", STATIONARY)
@pytest.mark.parametrize("rows", ("shared", "rows"))
def test_the_stationary_stream_is_the_one_shot_form(K, mb, pushes, rows):
    Q = -(-K // P)
    S = Q + mb - 1
    total = 2 * S + 1
    h, x = _data(K, total)
    xs = x if rows == "rows" else x[0]
    nrows = 2 if rows == "rows" else 1
    L = total * P + K - 1
    flush = -(-(K - 1) // P)
    got32 = run(h, xs, nrows, mb, pushes, flush_blocks=flush)[:, :L]
    assert got32.dtype == np.float32
    assert np.array_equal(got32, ols_ref(h, xs, P)), "fp32: not the bits of ols_ref"
    got64 = run(h, xs, nrows, mb, pushes, dtype=np.float64, flush_blocks=flush)[:, :L]
    e = _rel(got64, convolve_ref(h, xs)[0])
    print(f"K={K} {rows}: fp64 error / peak = {e:.3g}")
    assert e <= TOL


# the update cases of the GPU test, in blocks: (max_blocks, pushes, total blocks, update blocks)
UPDATES = {
    "before_the_first_push": (2, (2, 1), 6, (0,)),
    "adjacent_blocks": (3, (3, 1, 2), 9, (3, 4)),
    "mid_sequence": (3, (2,), 9, (4,)),
    "during_the_first_Q_blocks": (2, (1,), 7, (1, 2)),
}


@functools.lru_cache(maxsize=None)
def _update_case(name, K=4097, B=2):
    mb, pushes, total, at = UPDATES[name]
    rng = np.random.default_rng([13, sorted(UPDATES).index(name)])
    hs = rng.uniform(-1, 1, size=(len(at) + 1, B, K)).astype(np.float32)
    x = rng.uniform(-1, 1, size=(total * P,)).astype(np.float32)
    return mb, pushes, total, at, hs, x


@pytest.mark.parametrize("name", sorted(UPDATES))
def test_updates_are_the_path_form_piecewise(name):
    mb, pushes, total, at, hs, x = _update_case(name)
    K = hs.shape[-1]
    L = total * P + K - 1
    flush = -(-(K - 1) // P)
    ups = tuple((j, hs[u + 1]) for u, j in enumerate(at))
    got32 = run(hs[0], x, 1, mb, pushes, ups, flush_blocks=flush)[:, :L]
    want32 = piecewise(hs, x, at, total, L, lambda h, xx: ols_ref(h, xx, P), path_ols_ref)
    assert got32.shape == want32.shape and np.array_equal(got32, want32), "fp32: not the bits of ols_ref / path_ols_ref piecewise"
    got64 = run(hs[0], x, 1, mb, pushes, ups, dtype=np.float64, flush_blocks=flush)[:, :L]
    want64 = piecewise(hs, x, at, total, L, lambda h, xx: convolve_ref(h, xx)[0], path_ref64)
    e = _rel(got64, want64)
    print(f"{name}: fp64 error / peak = {e:.3g}")
    assert e <= TOL


def test_the_last_of_two_updates_wins():
    mb, pushes, total, at, hs, x = _update_case("mid_sequence")
    lost = np.ones_like(hs[1])
    a = run(hs[0], x, 1, mb, pushes, ((at[0], lost), (at[0], hs[1])))
    assert np.array_equal(a, run(hs[0], x, 1, mb, pushes, ((at[0], hs[1]),)))


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_every_mutation_fails_both_checks(mutation):
    mb, pushes, total, at, hs, x = _update_case("adjacent_blocks")
    K = hs.shape[-1]
    L = total * P + K - 1
    flush = -(-(K - 1) // P)
    ups = tuple((j, hs[u + 1]) for u, j in enumerate(at))
    want32 = piecewise(hs, x, at, total, L, lambda h, xx: ols_ref(h, xx, P), path_ols_ref)
    want64 = piecewise(hs, x, at, total, L, lambda h, xx: convolve_ref(h, xx)[0], path_ref64)
    bad32 = run(hs[0], x, 1, mb, pushes, ups, mutate=mutation, flush_blocks=flush)[:, :L]
    bad64 = run(hs[0], x, 1, mb, pushes, ups, dtype=np.float64, mutate=mutation, flush_blocks=flush)[:, :L]
    good = _rel(run(hs[0], x, 1, mb, pushes, ups, dtype=np.float64, flush_blocks=flush)[:, :L], want64) / TOL
    factor = _rel(bad64, want64) / TOL
    print(f"{mutation}: fp64 error over the tolerance = {factor:.3g} (unmutated: {good:.3g}); "
          f"{int((bad32 != want32).sum())} of {want32.size} fp32 samples differ")
    assert not np.array_equal(bad32, want32)
    assert factor >= 10.0 and good <= 1.0
