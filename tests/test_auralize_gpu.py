"""csrc/auralize.hip on the device, element by element against the fp64 restatement of tests/auralize_ref.py.

Geometries: K around the 32-wide MFMA tile (1, 31, 32, 33), 100, 1025 (just above the 1024-tap chunk of h: two chunks, the second nearly
empty) and 9600 once; N = 1, 31, 33, 1000 (N < K and N > K both occur) and 5000 (two of a workgroup's four waves own outputs, the
second a partial tile); 17 000 samples (more than the 16 384 outputs of a workgroup: the block index has to be split into row and tile).
Every geometry runs with B = 1 and 3, x shared and per row, L = full, N and 1.

Integer data (|h| <= 3, |x| <= 7: every partial sum below 21 K <= 201 600 < 2^24) must EQUAL the reference.  Uniform data in [-1, 1]
(no subnormals) must lie within (terms + 2) 2^-24 sum_k |h[k] x[n - k]| of it: one rounding per accumulated term."""
import numpy as np
import pytest
import torch

from auralize_ref import case

pytestmark = pytest.mark.gpu

KS = (1, 31, 32, 33, 100, 1025)
NS = (1, 31, 33, 1000, 5000)
GEOMS = [(K, N) for K in KS for N in NS] + [(33, 17000), (1025, 17000), (9600, 1000)]
CANARY = 12345.678          # no integer, so no sum of integer data


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the cached arrays are read-only


def _run(h, x, L, pad=(1, 64)):
    """auralize into the middle of a canary-filled buffer (the front pad also puts `out` off 16-byte alignment); returns the result on the
    host after checking that nothing around it was written."""
    import unet_rir_amd as U
    B = h.shape[0]
    buf = torch.full((pad[0] + B * L + pad[1],), CANARY, dtype=torch.float32, device="cuda")
    out = buf[pad[0]:pad[0] + B * L].view(B, L)
    got = U.auralize(h, x, length=L, out=out)
    assert got is out
    host = buf.cpu().numpy()
    assert np.all(host[:pad[0]] == CANARY) and np.all(host[pad[0] + B * L:] == CANARY), "written outside out"
    return host[pad[0]:pad[0] + B * L].reshape(B, L).copy()


def _variants(K, N, kind):
    """(name, h, x, L, reference triple) for B = 1 and 3, x shared and per row, L = full, N and 1"""
    h, x, rows, shared = case(K, N, kind)
    hd, xd = _dev(h), _dev(x)
    for B in (1, 3):
        for mode, xs, ref in (("shared", xd[0], shared), ("rows", xd[:B], rows)):
            for L in (N + K - 1, N, 1):
                yield f"B={B} {mode} L={L}", hd[:B], xs, L, tuple(a[:B, :L] for a in ref)


@pytest.mark.parametrize("K,N", GEOMS, ids=[f"K{K}-N{N}" for K, N in GEOMS])
def test_integer_data_equals_the_reference(K, N):
    for name, h, x, L, (y, _, _) in _variants(K, N, "int"):
        got = _run(h, x, L)
        assert not np.any(got == CANARY), name                       # every element written
        bad = np.flatnonzero(got.astype(np.float64) != y)
        assert bad.size == 0, (name, bad[:8], got.ravel()[bad[:8]], y.ravel()[bad[:8]])


@pytest.mark.parametrize("K,N", GEOMS, ids=[f"K{K}-N{N}" for K, N in GEOMS])
def test_uniform_data_within_one_rounding_per_term(K, N):
    worst = 0.0
    for name, h, x, L, (y, S, terms) in _variants(K, N, "uniform"):
        got = _run(h, x, L).astype(np.float64)
        assert np.all(np.isfinite(got)), name
        err, bound = np.abs(got - y), (terms + 2) * 2.0 ** -24 * S
        worst = max(worst, float(np.max(err / bound)))
        bad = np.flatnonzero(err > bound)
        assert bad.size == 0, (name, bad[:8], err.ravel()[bad[:8]], bound.ravel()[bad[:8]])
    print(f"K={K} N={N}: worst error / bound = {worst:.3f}")


@pytest.mark.parametrize("K,N", [(33, 1000), (1025, 5000), (100, 17000), (9600, 1000)])
def test_bits_do_not_depend_on_run_batch_layout_or_length(K, N):
    import unet_rir_amd as U
    h, x, _, _ = case(K, N, "uniform")
    hd, xd = _dev(h), _dev(x)
    full = U.auralize(hd, xd)
    assert full.shape == (3, N + K - 1) and full.dtype == torch.float32
    assert torch.equal(U.auralize(hd, xd), full)                                          # two runs
    for b in range(3):                                                                    # a row alone, [K] and [1, K]
        assert torch.equal(U.auralize(hd[b], xd[b]), full[b:b + 1]) and torch.equal(U.auralize(hd[b:b + 1], xd[b:b + 1]), full[b:b + 1])
    assert torch.equal(U.auralize(hd.flip(0).contiguous(), xd.flip(0).contiguous()), full.flip(0))       # its place in the batch
    sh = U.auralize(hd, xd[1])
    assert torch.equal(sh, U.auralize(hd, xd[1].repeat(3, 1)))                            # shared x = x repeated per row
    assert torch.equal(sh[1], full[1])
    same = U.auralize(hd, xd, length="same")
    assert same.shape == (3, N) and torch.equal(same, full[:, :N])                        # a truncated L = the head of the full result
    for L in (1, 31, 1024, N + K - 2):
        if L <= N + K - 1:
            assert torch.equal(U.auralize(hd, xd, length=L), full[:, :L]), L


def test_graph_capture_replays_the_same_bits():
    import unet_rir_amd as U
    K, N = 1025, 5000
    h, x, _, _ = case(K, N, "uniform")
    hd, xd = _dev(h), _dev(x[0])
    eager = U.auralize(hd, xd)
    out = torch.zeros_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        U.auralize(hd, xd, out=out)                      # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            U.auralize(hd, xd, out=out)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_the_largest_supported_response():
    """K = 16384: the LDS budget at its limit (143 620 bytes), 17 chunks; integer data, one row, exact."""
    import unet_rir_amd as U
    h, x, _, shared = case(16384, 300, "int")
    got = U.auralize(_dev(h[:1]), _dev(x[0])).cpu().numpy().astype(np.float64)
    assert np.array_equal(got, shared[0][:1])
    with pytest.raises(ValueError, match="supported"):
        U.auralize(torch.zeros(1, 16385, device="cuda"), _dev(x[0]))
