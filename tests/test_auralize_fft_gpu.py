"""csrc/auralize_fft.hip on the device, element by element against the fp64 double sum of tests/auralize_ref.py.

With P = ops.auralize_fft_block(K) (2048): K around the partition edge (1, P - 1, P, P + 1, 2P + 1), 9600 and the largest, 16384; every K
against at least three N around a block edge (1, P - 1, P, P + 1, 2P + 5, 5000).  Every geometry runs with B = 1 and 3, x shared and
per row, L = full, N, 1, P and P + 1 (where N + K - 1 allows), into the middle of a canary-filled buffer.

Uniform data in [-1, 1] must lie within the bound of include/unetrir.h (tests/auralize_fft_ref.bound) - which is loose, so integer data
(|h| <= 3, |x| <= 7) must in addition ROUND to the exact result at every element, and on uniform data every block of P output samples
must be as close to fp64 in rms as twice the complex64 restatement of the same pipeline (tests/auralize_fft_ref.ols_ref), which is
4e3 to 3e4 times tighter than the bound: an error of the FFT itself that the bound cannot see."""
import ctypes as C

import numpy as np
import pytest
import torch

from auralize_fft_ref import bound, ols_ref
from auralize_ref import case

pytestmark = pytest.mark.gpu

P = 2048
GEOMS = ([(1, N) for N in (1, P - 1, P, P + 1, 2 * P + 5)] + [(P - 1, N) for N in (1, P, P + 1, 5000)] +
         [(P, N) for N in (P - 1, P, P + 1)] + [(P + 1, N) for N in (P - 1, P, P + 1, 2 * P + 5)] +
         [(2 * P + 1, N) for N in (P - 1, P + 1, 2 * P + 5)] + [(9600, N) for N in (P - 1, P, P + 1, 5000)] +
         [(16384, N) for N in (1, P - 1, P, P + 1)])
IDS = [f"K{K}-N{N}" for K, N in GEOMS]
CANARY = 12345.678          # no integer, so no sum of integer data


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the cached arrays are read-only


def _run(h, x, L, pad=(1, 64)):
    """method="fft" into the middle of a canary-filled buffer (the front pad also puts `out` off 8-byte alignment); returns the result on
    the host after checking that nothing around it was written."""
    import unet_rir_amd as U
    B = h.shape[0]
    buf = torch.full((pad[0] + B * L + pad[1],), CANARY, dtype=torch.float32, device="cuda")
    out = buf[pad[0]:pad[0] + B * L].view(B, L)
    got = U.auralize(h, x, length=L, out=out, method="fft")
    assert got is out
    host = buf.cpu().numpy()
    assert np.all(host[:pad[0]] == CANARY) and np.all(host[pad[0] + B * L:] == CANARY), "written outside out"
    return host[pad[0]:pad[0] + B * L].reshape(B, L).copy()


def _variants(K, N, kind):
    """(name, device h, device x, host h, host x, L, reference y) for B = 1 and 3, x shared and per row, L = full, N, 1, P and P + 1"""
    h, x, rows, shared = case(K, N, kind)
    hd, xd = _dev(h), _dev(x)
    for B in (1, 3):
        for mode, xs, xh, ref in (("shared", xd[0], x[0], shared), ("rows", xd[:B], x[:B], rows)):
            for L in sorted({N + K - 1, N, 1, P, P + 1}):
                if L <= N + K - 1:
                    yield f"B={B} {mode} L={L}", hd[:B], xs, h[:B], xh, L, ref[0][:B, :L]


def _block_rms(v, y):
    """rms of v - y over each block of P samples [B, J] (the last one may be short) and over each whole row [B]"""
    d2 = (v - y) ** 2
    B, L = d2.shape
    J = -(-L // P)
    pad = np.zeros((B, J * P))
    pad[:, :L] = d2
    return np.sqrt(pad.reshape(B, J, P).sum(axis=2) / np.minimum(P, L - P * np.arange(J))), np.sqrt(d2.mean(axis=1))


def test_the_block_is_the_documented_one():
    import unet_rir_amd as U
    assert all(U.ops.auralize_fft_block(K) == P for K, _ in GEOMS)


@pytest.mark.parametrize("K,N", GEOMS, ids=IDS)
def test_uniform_data_within_the_bound(K, N):
    """Every element within the bound; and where there is at least one whole block (N + K - 1 >= P), on the full-length variants, the
    rms error r_j of every block j of every row at most twice that of the complex64 restatement rs of the same pipeline in that block,
    or over the row (the floor for a ragged last block of a few samples): r_j(kernel) <= 2 max(r_j(rs), r_row(rs)).  The margin 2 is
    that of C1 in tests/fft_lds_ref.py, for the same reason: both are fp32 FFTs with correctly rounded twiddles.  The shorter L are the
    head of the full result bit for bit (test_bits_do_not_depend_on...)."""
    worst, worst_blk = 0.0, 0.0
    for name, hd, xd, h, x, L, y in _variants(K, N, "uniform"):
        got = _run(hd, xd, L).astype(np.float64)
        assert np.all(np.isfinite(got)) and not np.any(got == np.float32(CANARY)), name
        err, lim = np.abs(got - y), bound(h, x, P, L=L)
        worst = max(worst, float(np.max(err / lim)))
        bad = np.flatnonzero(err > lim)
        assert bad.size == 0, (name, bad[:8], err.ravel()[bad[:8]], lim.ravel()[bad[:8]])
        if L == N + K - 1 and L >= P:
            rs_blk, rs_row = _block_rms(ols_ref(h, x, P).astype(np.float64), y)
            assert np.all(rs_row > 0), name                           # from the restatement alone
            blk, _ = _block_rms(got, y)
            ratio = blk / np.maximum(rs_blk, rs_row[:, None])
            worst_blk = max(worst_blk, float(ratio.max()))
            assert np.all(ratio <= 2.0), (name, np.argwhere(ratio > 2.0)[:8], ratio[ratio > 2.0][:8])
    print(f"K={K} N={N}: worst error / bound = {worst:.3g}" + (f", worst block rms / restatement's = {worst_blk:.3g}" if worst_blk else ""))


@pytest.mark.parametrize("K,N", GEOMS, ids=IDS)
def test_integer_data_rounds_to_the_exact_result_everywhere(K, N):
    worst = 0.0
    for name, hd, xd, h, x, L, y in _variants(K, N, "int"):
        got = _run(hd, xd, L).astype(np.float64)
        assert not np.any(got == np.float32(CANARY)), name           # every element written
        worst = max(worst, float(np.max(np.abs(got - y))))
        bad = np.flatnonzero(np.rint(got) != y)
        assert bad.size == 0, (name, bad[:8], got.ravel()[bad[:8]], y.ravel()[bad[:8]])
    print(f"K={K} N={N}: largest error on integer data = {worst:.3g}")


@pytest.mark.parametrize("dry_rows", (0, 1), ids=("shared", "rows"))
def test_exactly_the_advertised_workspace_is_used(dry_rows):
    """The C entry point with a workspace of exactly ws_bytes in front of a canary, and one byte less refused."""
    import unet_rir_amd as U
    K, N, B = P + 1, 2 * P + 5, 3
    L = N + K - 1
    h, x, rows, shared = case(K, N, "int")
    hd, xd = _dev(h), _dev(x if dry_rows else x[0])
    stride = N if dry_rows else 0
    need = U.ops.auralize_fft_ws_bytes(B, K, N, stride, L)
    assert need == 16384 * (B * 2 + (B if dry_rows else 1) * 4)
    ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.empty((B, L), dtype=torch.float32, device="cuda")
    lib = U._lib.lib()
    args = (C.c_void_p(hd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), B, K, N, stride, L)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.unetrir_auralize_fft_f32(*args, C.c_void_p(ws.data_ptr()), need - 1, stream) == 10001
    assert lib.unetrir_auralize_fft_f32(*args, C.c_void_p(ws.data_ptr() + 8), need, stream) == 10001
    assert lib.unetrir_auralize_fft_f32(*args, C.c_void_p(ws.data_ptr()), need, stream) == 0
    torch.cuda.synchronize()
    assert torch.all(ws[need:] == 0xA5), "written beyond the advertised workspace"
    y = (rows if dry_rows else shared)[0]
    assert np.array_equal(np.rint(out.cpu().numpy().astype(np.float64)), y)


@pytest.mark.parametrize("K,N", [(33, 1000), (P + 1, 2 * P + 5), (9600, 5000)])
def test_bits_do_not_depend_on_run_batch_layout_length_or_workspace(K, N):
    import unet_rir_amd as U
    h, x, _, _ = case(K, N, "uniform")
    hd, xd = _dev(h), _dev(x)
    f = lambda *a, **kw: U.auralize(*a, method="fft", **kw)
    full = f(hd, xd)
    assert full.shape == (3, N + K - 1) and full.dtype == torch.float32
    assert torch.equal(f(hd, xd), full)                                                   # two runs
    for b in range(3):                                                                    # a row alone, [K] and [1, K]
        assert torch.equal(f(hd[b], xd[b]), full[b:b + 1]) and torch.equal(f(hd[b:b + 1], xd[b:b + 1]), full[b:b + 1])
    assert torch.equal(f(hd.flip(0).contiguous(), xd.flip(0).contiguous()), full.flip(0))               # its place in the batch
    sh = f(hd, xd[1])
    assert torch.equal(sh, f(hd, xd[1].repeat(3, 1)))                                     # shared x = x repeated per row
    assert torch.equal(sh[1], full[1])
    same = f(hd, xd, length="same")
    assert same.shape == (3, N) and torch.equal(same, full[:, :N])                        # a truncated L = the head of the full result
    for L in (1, 31, P - 1, P, P + 1, N + K - 2):
        if L <= N + K - 1:
            assert torch.equal(f(hd, xd, length=L), full[:, :L]), L
    padded = torch.cat([xd, torch.zeros(3, P + 7, device="cuda")], dim=1)                 # N beyond the samples themselves
    assert torch.equal(f(hd, padded, length=N + K - 1), full)
    ws = U.ops.Workspace(hd.device)                                                       # a caller's workspace, grown by the call
    out = torch.empty_like(full)
    U.ops.auralize_fft_f32(hd, xd, out, ws=ws)
    assert ws.nbytes >= U.ops.auralize_fft_ws_bytes(3, K, N, N, N + K - 1) and torch.equal(out, full)


def test_graph_capture_replays_the_same_bits():
    import unet_rir_amd as U
    K, N = P + 1, 5000
    h, x, _, _ = case(K, N, "uniform")
    hd, xd = _dev(h), _dev(x[0])
    eager = U.auralize(hd, xd, method="fft")
    out = torch.zeros_like(eager)
    ws = U.ops.Workspace(hd.device, U.ops.auralize_fft_ws_bytes(3, K, N, 0, N + K - 1))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        U.ops.auralize_fft_f32(hd, xd, out, ws=ws)       # on the side stream, outside the capture
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            U.ops.auralize_fft_f32(hd, xd, out, ws=ws)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(CANARY)
        ws.buf.fill_(0xA5)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_fft_and_direct_agree_within_the_sum_of_their_bounds():
    import unet_rir_amd as U
    K, N = 9600, 5000
    h, x, rows, _ = case(K, N, "uniform")
    hd, xd = _dev(h), _dev(x)
    fft = U.auralize(hd, xd, method="fft").cpu().numpy().astype(np.float64)
    direct = U.auralize(hd, xd, method="direct").cpu().numpy().astype(np.float64)
    assert torch.equal(U.auralize(hd, xd), U.auralize(hd, xd, method="direct"))           # the default is the direct form
    _, S, terms = rows
    lim = bound(h, x, P) + (terms + 2) * 2.0 ** -24 * S
    diff = np.abs(fft - direct)
    print(f"largest |fft - direct| = {diff.max():.3g}, worst / bound = {np.max(diff / lim):.3g}")
    assert np.all(diff <= lim)


def test_the_largest_supported_response_and_the_first_unsupported():
    import unet_rir_amd as U
    with pytest.raises(ValueError, match="supported"):
        U.auralize(torch.zeros(1, 16385, device="cuda"), torch.zeros(300, device="cuda"), method="fft")
