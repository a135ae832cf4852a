"""`AuralizeStream` (csrc/auralize_fft.hip) restated with torch's CPU FFTs: the streaming algorithm, not the one-shot one.

    state: H[2] (the spectra of the current response and of the one being faded in), a ring X[rows][S] of the last spectra of x,
           S = Q + max_blocks - 1, X_i in slot i mod S; the carry (the last P dry samples); count c, cur, pending
    push(new [rows, blocks P]):   X_{c+i} = rfft(carry | new) for i = 0, rfft(new[(i-1)P ... (i+1)P)) beyond -> slot (c + i) mod S
                                  Y_j = sum_{q <= min(j, Q-1)} H_q X_{j-q} through the ring, ascending q; the last P samples of irfft(Y_j)
                                  with a fade pending, block c through the old and the new response, blended as auralize_path blends
                                  two nodes at cP and (c+1)P; every later block through the new response
                                  then carry = the last P samples, c += blocks, the new response current
    update(h):                    spectra into the slot that is not current, pending = 1

The transforms, the products and the blend are those of tests/auralize_fft_ref.ols_ref and tests/auralize_path_ref.path_ols_ref (their
helpers imported, not edited), so in fp32 the stream equals them bit for bit, piecewise; in fp64 it is held to the definition.
(torch's elementwise complex product runs a vector body and a scalar tail whose roundings differ in rare elements, and where the two
meet depends on the row length and on how a large tensor is divided among threads: the products here are formed one row of P + 1 bins
at a time, which is how a single-threaded ols_ref walks its tensors - tests/test_auralize_stream_ref.py runs both on one thread.)
`mutate` selects one of MUTATIONS, deliberately wrong variants of one line each:
    ring_short         the ring one slot short (S - 1): a push of max_blocks blocks overwrites a spectrum it still needs
    stale_carry        the carry not refreshed after a push: the first window of the next push starts with old samples
    fade_second_block  the fade applied to the second block of the push instead of the first
    early_switch       the new response made current a block early: the fade block is rendered through the new response alone"""
import numpy as np
import torch

from auralize_path_ref import gain32

P = 2048
MUTATIONS = ("ring_short", "stale_carry", "fade_second_block", "early_switch")


class StreamRef:
    def __init__(self, h, rows, max_blocks, dtype=np.float32, mutate=None):
        """h [B, K]; rows: 1 (shared dry) or B; dtype float32 (complex64 spectra) or float64 (complex128)"""
        assert mutate is None or mutate in MUTATIONS
        self.B, self.K = h.shape
        assert rows in (1, self.B) and max_blocks >= 1
        self.rows, self.max_blocks, self.dtype, self.mutate = rows, max_blocks, np.dtype(dtype), mutate
        self.Q = -(-self.K // P)
        self.S = self.Q + max_blocks - 1 - (1 if mutate == "ring_short" else 0)
        assert self.S >= 1
        cdtype = torch.complex64 if self.dtype == np.float32 else torch.complex128
        self.H = [self._spectra(h), torch.zeros((self.B, self.Q, P + 1), dtype=cdtype)]
        self.X = torch.zeros((rows, self.S, P + 1), dtype=cdtype)
        self.carry = np.zeros((rows, P), dtype=self.dtype)
        self.count, self.cur, self.pending = 0, 0, False

    def _spectra(self, h):
        hp = np.zeros((self.B, self.Q, 2 * P), dtype=self.dtype)
        flat = np.zeros((self.B, self.Q * P), dtype=self.dtype)
        flat[:, :self.K] = h
        hp[:, :, :P] = flat.reshape(self.B, self.Q, P)
        return torch.fft.rfft(torch.from_numpy(hp))

    def update(self, h):
        self.H[1 - self.cur] = self._spectra(h)
        self.pending = True

    def _block(self, H, j):
        """the last P samples of irfft(sum_q H_q X_{j-q}), [B, P]"""
        Y = torch.zeros((self.B, P + 1), dtype=H.dtype)
        for q in range(min(j, self.Q - 1) + 1):                               # ascending q
            for b in range(self.B):                                            # row by row: see the note on torch's products above
                Y[b] += H[b, q] * self.X[b if self.rows > 1 else 0, (j - q) % self.S]
        y = torch.fft.irfft(Y, n=2 * P)[:, P:].numpy()
        assert y.dtype == self.dtype
        return y

    def push(self, new):
        """new [rows, blocks P] or None (zeros, one block) -> [B, blocks P]"""
        new = np.zeros((self.rows, P), dtype=self.dtype) if new is None else np.asarray(new, dtype=self.dtype).reshape(self.rows, -1)
        blocks = new.shape[1] // P
        assert 1 <= blocks <= self.max_blocks and new.shape[1] == blocks * P
        ext = np.concatenate([self.carry, new], axis=1)
        for i in range(blocks):
            self.X[:, (self.count + i) % self.S] = torch.fft.rfft(torch.from_numpy(ext[:, i * P:(i + 2) * P].copy()))
        fade_at = (1 if self.mutate == "fade_second_block" and blocks > 1 else 0) if self.pending else -1
        old, fresh = self.H[self.cur], self.H[1 - self.cur]
        out = np.zeros((self.B, blocks * P), dtype=self.dtype)
        for i in range(blocks):
            j = self.count + i
            if i == fade_at:
                out[:, i * P:(i + 1) * P] = self._fade(fresh if self.mutate == "early_switch" else old, fresh, j)
            else:
                out[:, i * P:(i + 1) * P] = self._block(fresh if self.pending and i > fade_at else old, j)
        if self.mutate != "stale_carry":
            self.carry = new[:, -P:].copy()
        self.count += blocks
        if self.pending:
            self.cur, self.pending = 1 - self.cur, False
        return out

    def _fade(self, old, fresh, j):
        """block j of auralize_path with the nodes (old at jP, fresh at (j+1)P): the blend of path_ols_ref, or its fp64 definition"""
        n = np.arange(j * P, (j + 1) * P, dtype=np.int64)
        tau = np.array([j * P, (j + 1) * P], dtype=np.int64)
        y = [self._block(old, j), self._block(fresh, j)]
        if self.dtype == np.float64:
            a = (n - tau[0]) / float(P)
            return (1.0 - a)[None] * y[0] + a[None] * y[1]
        acc = np.zeros((self.B, P), dtype=np.float32)
        have = np.zeros(P, dtype=bool)
        for r in range(2):                                                     # path_ols_ref's blend, line for line
            g = gain32(n, r, tau)
            first = g[None] * y[r]
            fused = (g[None].astype(np.float64) * y[r].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
            use = g != 0
            acc = np.where(use[None], np.where(have[None], fused, first), acc)
            have |= use
        return acc


def run(h0, x, rows, max_blocks, pushes, updates=(), dtype=np.float32, mutate=None, flush_blocks=0):
    """The stream over x [N] or [rows, N] (N a whole number of blocks) cut into pushes of `pushes` blocks (cycled), with
    updates = ((block index, h), ...) applied before the push that starts at that block; then flush_blocks blocks of zeros.
    -> [B, N + flush_blocks P]"""
    x2 = np.asarray(x).reshape(rows, -1)
    total = x2.shape[1] // P
    assert x2.shape[1] == total * P
    s = StreamRef(np.asarray(h0), rows, max_blocks, dtype, mutate)
    todo = sorted(updates, key=lambda u: u[0])
    out, at, k = [], 0, 0
    while at < total + flush_blocks:
        while todo and todo[0][0] <= at:
            assert todo[0][0] == at, "an update must fall on a push boundary"
            s.update(todo.pop(0)[1])
        nb = pushes[k % len(pushes)]
        k += 1
        if at < total:
            nb = min(nb, total - at)
            if todo:
                nb = min(nb, todo[0][0] - at)
            out.append(s.push(x2[:, at * P:(at + nb) * P]))
        else:
            nb = 1
            out.append(s.push(None))
        at += nb
    return np.concatenate(out, axis=1)


def piecewise(hs, x, at, total, L, one_shot, path):
    """The yardstick of a stream with updates at blocks `at`: blocks [0, at_0) of one_shot(h_0, x); blocks [at_u, at_{u+1}) of
    path(stack(h_u, h_{u+1}), x, times = [at_u P, (at_u + 1) P]).  A single path over all nodes is not it: between two nodes that
    carry the same response it blends (1 - a) y + a y, which is not y bit for bit."""
    edges = list(at) + [total + 64]
    parts = [one_shot(hs[0], x)[:, :min(at[0] * P, L)]]
    for u, j in enumerate(at):
        y = path(np.stack([hs[u], hs[u + 1]], axis=1), x, [j * P, (j + 1) * P])
        parts.append(y[:, j * P:min(edges[u + 1] * P, L)])
    return np.concatenate(parts, axis=1)
