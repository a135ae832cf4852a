"""References and criteria for the code between the convolutions and the optimiser: the fixed-order split-K reductions of
csrc/splitk_reduce.hip and the weight work copies of csrc/weights.hip.  CPU only (torch / NumPy), importable without the product;
tests/test_reduction_ref.py proves on emulated kernels that the criteria accept the true result and reject each of ten mutants.

  reductions   out[i] = sum_s part[s][i] + reg * w[i].  Integer data: every partial sum of any grouping is exact in fp32, the
               output is determined - equality (tests/exact_data.py).  Uniform data: reduce_ref's bound, element by element
               (tests/streaming_check.py).
  work copies  one rounding to bf16 (nearest, ties to even), zero pad, the layouts restated from include/unetrir.h - compared
               BIT for bit (assert_bits: the sign of a zero and a canary NaN count), so no tolerance appears anywhere.
"""
import functools

import numpy as np
import torch

import exact_data as X
import streaming_check as S
from oracle import detrand

U32 = S.U32
EINVAL = 10001               # UNETRIR_EINVAL (include/unetrir.h)


# ----------------------------------------------------------------------------------------------------------------------
# the weight-slab reduction
# ----------------------------------------------------------------------------------------------------------------------
def reduce_ref(part64, reg, w64):
    """(sum, bound) of out = sum_s part[s] + reg * w for part64 [nsplit, n] and w64 [n] (None: no reg term), both fp64; reg is
    the fp32 number the kernel is given.

    Bound, to first order: the kernel performs nsplit - 1 fp32 additions of slab values (in ANY grouping: every group starts from
    its first slab, which is exact, and G group sums take G - 1 additions to combine), one product reg * w and one more addition.
    That is nsplit + 1 roundings, each of relative size 2^-24 on a partial result that is no larger than the sum of the absolute
    values of all terms, S = sum_s |part[s]| + |reg * w|.  By the project's "k roundings give k * U32 * S" rule:
        bound = (nsplit + 1) * 2^-24 * S.
    A fused multiply-add for the last step only lowers the count."""
    nsplit = part64.shape[0]
    total, S_abs = part64.sum(0), part64.abs().sum(0)
    if w64 is not None:
        total, S_abs = total + reg * w64, S_abs + (reg * w64).abs()
    return total, (nsplit + 1) * U32 * S_abs


NSPLITS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 56, 57, 58, 64, 65, 224, 225, 257, 300)
NS = (1, 3, 4, 5, 63, 64, 252, 255, 256, 257, 260, 1000, 4100)
LARGE = ((32, 32512), (33, 32512), (32, 32516), (33, 32516))      # the last n that takes the wide form and the first that does not
CASES = tuple((s, n) for s in NSPLITS for n in NS) + LARGE
VARIANTS = ("noreg", "reg", "offset")      # reg = 0 and w = NULL; reg != 0 with w; the latter with part, out and w one float off
INT_RANGE = 1000
POOL = max(s * (n + 1) for s, n in CASES) + 1024     # floats; every case reads its slabs from ONE pool (room for the n + 1 mutant)


def pool_offset(i, misaligned):
    """Where case i's slabs begin in the pool: 16-byte aligned positions that differ from case to case, + 1 float when misaligned."""
    return 4 * ((37 * i) % 64) + (1 if misaligned else 0)


def reg_of(data, variant):
    """The l2 coefficient as the fp32 number that travels through the ABI."""
    if variant == "noreg":
        return 0.0
    return X.REG if data == "int" else float(np.float32(2e-3))


@functools.lru_cache(maxsize=None)
def pool(data):
    """(slab pool [POOL], w pool [max n + 8]) as fp32 tensors.  "int": integers in [-1000, 1000].  "uniform": uniform(-1, 1) times
    2^k, k in [-8, 8] per element, so that addends of very different size meet and rounding matters."""
    nw = max(n for _, n in CASES) + 8
    if data == "int":
        p, w = X.ints("rr-pool-int", (POOL,), -INT_RANGE, INT_RANGE), X.ints("rr-w-int", (nw,), -INT_RANGE, INT_RANGE)
    else:
        def scaled(tag, m):
            u = torch.tensor(detrand.uniform(f"rr-{tag}-u", (m,), -1, 1, np.float64))
            k = torch.tensor(detrand.randint(f"rr-{tag}-k", (m,), 0, 17) - 8, dtype=torch.float64)
            return u * 2.0 ** k
        p, w = scaled("pool", POOL), scaled("w", nw)
    assert torch.equal(p.float().double(), p) and torch.equal(w.float().double(), w)          # fp32 holds them exactly
    return p.float(), w.float()


def slabs(data, i, misaligned, stride=None):
    """Case i's slabs [nsplit, n] as a view of the pool (stride: the distance between slabs, n unless a mutant asks otherwise)."""
    nsplit, n = CASES[i]
    off = pool_offset(i, misaligned)
    return pool(data)[0][off:].as_strided((nsplit, n), (n if stride is None else stride, 1))


@functools.lru_cache(maxsize=None)
def slab_sums(data, misaligned):
    """Per case: (sum_s part[s], sum_s |part[s]|) in fp64 - the part of the reference that does not depend on reg."""
    out = []
    for i in range(len(CASES)):
        p = slabs(data, i, misaligned).double()
        out.append((p.sum(0), p.abs().sum(0)))
    return out


def case_ref(data, variant, i):
    """(reference, bound) of case i in fp64 - reduce_ref's result, assembled from the shared slab sums."""
    nsplit, n = CASES[i]
    mis = variant == "offset"
    total, S_abs = slab_sums(data, mis)[i]
    reg = reg_of(data, variant)
    if reg != 0.0:
        t = reg * pool(data)[1][(1 if mis else 0):][:n].double()
        total, S_abs = total + t, S_abs + t.abs()
    return total, (nsplit + 1) * U32 * S_abs, S_abs


def check_reduction(got, data, variant, i, what, kernel=None):
    """The criterion of the GPU sweep for one case.  "int": the exactness condition from the reference alone, then equality;
    "uniform": every element within reduce_ref's bound."""
    ref, bound, S_abs = case_ref(data, variant, i)
    if data == "int":
        assert float(S_abs.max()) < X.EXACT_LIMIT * X.REG, f"{what}: sum of absolute terms {float(S_abs.max()):.4g} is not below 2^24 * 0.5"
        X.assert_exact(got, ref, what)
    else:
        S.check(got, ref, bound, what, kernel=kernel or "splitk_reduce")


def expected_kind(nsplit, n, part_addr, out_addr, w_addr):
    """reduce_kind's rule (csrc/splitk_reduce.hip), restated: 0 = the wide form - n a multiple of 4, at least 32 slabs, fewer than
    128 narrow workgroups (64 float4 outputs each) and every pointer on a 16-byte boundary (a NULL w counts as aligned) - else the
    narrow form with 8 / 4 / 2 / 1 slab groups: the largest of those that nsplit reaches."""
    narrow_blocks = -(-(-(-n // 4)) // 64)
    if n % 4 == 0 and nsplit >= 32 and narrow_blocks < 128 and (part_addr | out_addr | (w_addr or 0)) % 16 == 0:
        return 0
    return 8 if nsplit >= 8 else 4 if nsplit >= 4 else 2 if nsplit >= 2 else 1


def assert_every_form_is_entered(kinds, wide=True):
    """kinds: [(kind, n)] of a sweep.  Every form occurs with n % 4 zero and non-zero, except wide, which requires zero (wide=False:
    a sweep over misaligned pointers, where the wide form must not occur at all)."""
    seen = {(k, n % 4 == 0) for k, n in kinds}
    want = {(k, z) for k in (1, 2, 4, 8) for z in (True, False)} | ({(0, True)} if wide else set())
    assert seen == want, sorted(want ^ seen)


def emulate(flat, nsplit, n, stride, reg, w, kind, acc=torch.float32):
    """The reduction as the kernels perform it, in fp32 torch arithmetic: G slab groups (32 in the wide form), group g adds slabs
    g, g + G, ... in order from zero, the group sums are added in order, then + reg * w.  flat: the pool from the case's first
    element on; stride: the distance between slabs; acc: the type that holds a partial sum (a mutant narrows it)."""
    G = 32 if kind == 0 else kind
    part = flat.as_strided((nsplit, n), (stride, 1))
    groups = []
    for g in range(min(G, nsplit)):
        s = torch.zeros(n, dtype=acc)
        for k in range(g, nsplit, G):
            s = (s + part[k].to(acc)).to(acc)
        groups.append(s)
    s = groups[0]
    for g in groups[1:]:
        s = (s + g).to(acc)
    s = s.float()
    if reg != 0.0:
        s = s + torch.tensor(reg, dtype=torch.float32) * w
    return s


# ----------------------------------------------------------------------------------------------------------------------
# the weight work copies
# ----------------------------------------------------------------------------------------------------------------------
def work_copy_ref(w, Cp, Np):
    """fp32 master [N][T][C] -> (same [N][T][Cp], transposed [C][T][Np]) in bf16: ONE rounding to nearest, ties to even
    (S.bf16_rne, from the bits: independent of any library's conversion), zero pad."""
    N, T, C = w.shape
    h = S.bf16_rne(w.double()).to(torch.bfloat16)             # exact: the values are bf16 numbers already
    assert torch.equal(h.double(), S.bf16_rne(w.double()))
    same = torch.zeros((N, T, Cp), dtype=torch.bfloat16)
    same[:, :, :C] = h
    tr = torch.zeros((C, T, Np), dtype=torch.bfloat16)
    tr[:, :, :N] = h.permute(2, 1, 0)
    return same, tr


def packed_elems(N, C):
    """Size of the packed copy by the header's prose: [N / 128 rounded up][C / 16][9][4][64][8]."""
    return -(-N // 128) * (C // 16) * 9 * 4 * 64 * 8


def packed_index(N, C):
    """Destination [N, 9, C] (int64) of every element of a [N][9][C] kernel in the packed stride-2 order, from the prose of
    include/unetrir.h: [N / 128][C / 16][9 taps][4 blocks of 32 channels][64 lanes][8 values]; lane = row + 32 * (8-channel half
    of the chunk); row = the position of the channel in its 32-block with bits 2 and 3 exchanged."""
    n = torch.arange(N).view(N, 1, 1)
    t = torch.arange(9).view(1, 9, 1)
    c = torch.arange(C).view(1, 1, C)
    group, chunk, block = n // 128, c // 16, (n // 32) % 4
    m = n % 32
    a, b, c2, d = m // 16, (m // 8) % 2, (m // 4) % 2, m % 4
    row = 16 * a + 8 * c2 + 4 * b + d
    lane = row + 32 * ((c // 8) % 2)
    value = c % 8
    dims = ((group, -(-N // 128)), (chunk, C // 16), (t, 9), (block, 4), (lane, 64), (value, 8))
    idx = torch.zeros((N, 9, C), dtype=torch.int64)
    for coord, size in dims:                                   # every dimension contiguous inside the one before it
        assert int(coord.min()) >= 0 and int(coord.max()) < size
        idx = idx * size + coord
    return idx


def packed_ref(w, N, C):
    """The packed stride-2 copy of the fp32 master w [N][9][C]: bf16 (one rounding), zero where no channel maps."""
    assert tuple(w.shape) == (N, 9, C) and C % 16 == 0
    out = torch.zeros(packed_elems(N, C), dtype=torch.bfloat16)
    out[packed_index(N, C).reshape(-1)] = S.bf16_rne(w.double()).to(torch.bfloat16).reshape(-1)
    return out


def assert_bits(got, want, what):
    """Bit equality of two tensors of one 2- or 4-byte type (the sign of a zero and NaN canaries included), through
    X.assert_exact so that the comparison is counted and a failure names its first elements."""
    assert got.dtype == want.dtype and got.element_size() in (2, 4), (what, got.dtype, want.dtype)
    it = torch.int16 if got.element_size() == 2 else torch.int32
    X.assert_exact(got.contiguous().view(it).double(), want.to(got.device).contiguous().view(it).double(), what)


def accepts(fn, *args):
    """An asserting check as a predicate (tests/test_reduction_ref.py)."""
    try:
        fn(*args)
    except AssertionError:
        return False
    return True


TIE_SLICE = 520          # the first elements of every master are overwritten by special_values()


def special_values():
    """fp32 values for the start of a master: exact bf16 ties - a bf16 number plus half its spacing - whose lower neighbour has
    an even (rounds down) and an odd (rounds up) last bit, in both signs and at four exponents; +-0; 2^-130 (an fp32 subnormal
    that bf16 holds); 3.0e38 (finite in bf16: the largest bf16 number is 3.39e38)."""
    v = []
    for e in (-20, -1, 0, 9):
        for j in range(0, 128, 2):                              # j and j + 1: both parities
            for jj in (j, j + 1):
                v.append(((128 + jj) / 128.0 + 2.0 ** -8) * 2.0 ** e * (-1.0 if (j // 2) % 2 else 1.0))
    v += [0.0, -0.0, 2.0 ** -130, -2.0 ** -130, 3.0e38, -3.0e38, 0.0, -0.0]
    t = torch.tensor(v, dtype=torch.float64)
    assert t.numel() == TIE_SLICE and torch.equal(t[:-8].float().double(), t[:-8])
    return t.float()


@functools.lru_cache(maxsize=None)
def master(N, T, C):
    """The fp32 master [N][T][C] of one shape: detrand.uniform(-1, 1) with special_values() over its first elements (as many as
    fit).  Returns (w, number of exact bf16 ties in it)."""
    w = torch.tensor(detrand.uniform(f"wc{N, T, C}", (N, T, C), -1, 1)).reshape(-1)
    sv = special_values()
    if w.numel() < sv.numel():
        sv = torch.cat([sv[:w.numel() - 8], sv[-8:]]) if w.numel() >= 8 else sv[:w.numel()]
    w[:sv.numel()] = sv
    return w.view(N, T, C), int(X.is_tie(w.double()).sum())
