"""Integer-valued test data for exact (tolerance-free) comparisons of convolution kernels with the fp64 oracle.

With integer inputs every product and every partial sum of a convolution is an integer; while all of them stay below 2^24 an
fp32 accumulation is exact IN ANY ORDER, the fp64 oracle is exact too, and what a correct kernel stores is fully determined:
the exact value for fp32 outputs, its bf16 rounding (to nearest, ties to even) for bf16 outputs.  A comparison then needs no
tolerance, does not depend on which kernel the dispatch chose, and sees every single wrong term, a truncating store, a
sub-fp32 intermediate or a missing bias.  Many outputs are exact ties between two bf16 neighbours (odd integers in [256, 512),
2 mod 4 in [512, 1024), ...), so the rounding mode is tested as well.

ONE data set serves every test:
  activations and output gradients  integers in {-1 .. 3}
  kernels                           integers in {-1 .. 2}  (signed, positive mean: partial sums grow with K, so an intermediate
                                                            narrower than fp32 loses bits)
  bias                              integers in [-300, 300]
  bf16 addends                      4 * integers in [-60, 60]  (multiples of 4 up to 240: bf16-representable)
  l2 coefficient                    reg = 0.5  (weight gradients are then multiples of 0.5)
"""
import torch

from oracle import detrand

ACT = (-1, 3)
KERNEL = (-1, 2)
BIAS = (-300, 300)
ADDEND = (-60, 60)          # times ADDEND_STEP
ADDEND_STEP = 4
REG = 0.5
EXACT_LIMIT = float(1 << 24)
# what the exact comparisons of this process have covered so far (assert_exact / note_ties keep it; test modules print it)
STATS = dict(comparisons=0, elements=0, ties=0)


def note_ties(n):
    STATS["ties"] += int(n)


def ints(name, shape, lo, hi):
    """Integers in [lo, hi] (both ends included) from oracle.detrand, as an fp64 torch tensor."""
    return torch.tensor(detrand.randint(name, tuple(shape), 0, hi - lo + 1) + lo, dtype=torch.float64)


def acts(name, shape):
    return ints(name, shape, *ACT)


def kernels(name, shape):
    return ints(name, shape, *KERNEL)


def biases(name, shape):
    return ints(name, shape, *BIAS)


def addends(name, shape):
    return ADDEND_STEP * ints(name, shape, *ADDEND)


def bf16(t):
    """Round to bfloat16 (nearest, ties to even), returned as fp64.  The values here are fp32-representable, so going through
    fp32 rounds once."""
    return t.float().to(torch.bfloat16).double()


def expected_bf16(conv_plus_bias_fp64, addend=None):
    """What the library stores for a bf16 output.  Without an addend: bf16(conv + bias).  With one, TWO roundings:
    bf16(bf16(conv + bias) + addend) - every bf16 epilogue rounds the convolution result to the storage type first and adds the
    addend to that (conv3x3g.hip:349-387, conv3x3p.hip:392, igemm_bf16.hip:217, pw1x1.hip:182, ...): what storing the convolution
    and adding afterwards would give."""
    y = bf16(conv_plus_bias_fp64)
    return y if addend is None else bf16(y + addend)


def is_tie(v):
    """Elements of the exact fp64 tensor v that lie exactly half way between two neighbouring bf16 values."""
    m, e = torch.frexp(v.abs())                      # |v| = m * 2^e, m in [0.5, 1): bf16 keeps 8 bits of m
    q = torch.ldexp(m, torch.full_like(e, 9))        # m * 2^9: an odd integer <=> the ninth bit is the last one set
    return (v != 0) & (q == q.round()) & (q % 2 == 1)


def count_ties(conv_plus_bias_fp64, addend=None):
    """Outputs for which a rounding of expected_bf16 is an exact tie (either of the two roundings when there is an addend)."""
    t = is_tie(conv_plus_bias_fp64)
    if addend is not None:
        t = t | is_tie(bf16(conv_plus_bias_fp64) + addend)
    return int(t.sum())


def check_exactness_conditions(inputs, abs_bound, want=None, addend=None, quantum=1.0, what=""):
    """What the method rests on, asserted from the oracle's side only (nothing here looks at a kernel's output):
      (a) every tensor of `inputs` - a dict name -> (fp64 tensor, stored as bf16?) - is integer-valued (a multiple of `quantum`
          for fp32 tensors when quantum != 1) and the bf16 ones survive the conversion to bfloat16 unchanged;
      (b) abs_bound - sum |terms| + |bias| + |addend| of the largest output: the oracle evaluated on absolute values, or
          K * max|x| * max|w| + ... - is below 2^24 * quantum, so every partial sum of any grouping is exact in fp32;
      (c) returns the number of exact bf16 ties among the outputs `want` (the exact conv + bias in fp64, with `addend` if the
          launch has one); 0 when want is None (fp32 outputs)."""
    for name, (t, stored_bf16) in inputs.items():
        q = 1.0 if stored_bf16 else quantum
        assert torch.equal(t / q, (t / q).round()), f"{what}: {name} is not integer-valued"
        if stored_bf16:
            assert torch.equal(bf16(t), t.double()), f"{what}: {name} does not survive the conversion to bfloat16"
        else:
            assert torch.equal(t.float().double(), t.double()), f"{what}: {name} is not fp32-representable"
    assert float(abs_bound) < EXACT_LIMIT * quantum, f"{what}: largest sum of absolute terms {float(abs_bound):.4g} is not below 2^24 * {quantum}"
    return 0 if want is None else count_ties(want, addend)


def conv_abs_bound(K, has_bias=True, has_addend=True, x_max=max(map(abs, ACT)), w_max=max(map(abs, KERNEL))):
    """K * max|x| * max|w| + max|bias| + max|addend| for this data set."""
    return K * x_max * w_max + (max(map(abs, BIAS)) if has_bias else 0) + (ADDEND_STEP * max(map(abs, ADDEND)) if has_addend else 0)


def assert_exact(got, want, what, tile=None):
    """Value equality of EVERY element (+0 == -0, as torch.equal).  got / want: tensors of one shape, on any device, of any
    floating type that holds both exactly; activations as [image, row, column, channel].  On failure the message carries the
    number of mismatches, the first ten as (index..., got, want) and, with tile=(rows, cols) for a 4-D tensor, how many distinct
    pixel tiles and channels they fall in."""
    assert tuple(got.shape) == tuple(want.shape), (what, tuple(got.shape), tuple(want.shape))
    w = want.to(got.device)
    g = got if got.dtype == torch.float64 else got.double()
    w = w if w.dtype == torch.float64 else w.double()
    bad = g != w                     # NaN != anything: a NaN on either side is a mismatch
    n_bad = int(bad.sum())
    STATS["comparisons"] += 1
    STATS["elements"] += g.numel()
    if n_bad == 0:
        return
    idx = bad.nonzero().cpu()
    gc, wc = g[bad].cpu(), w[bad].cpu()
    first = [tuple(int(i) for i in idx[j]) + (float(gc[j]), float(wc[j])) for j in range(min(10, n_bad))]
    msg = f"{what}: {n_bad} of {g.numel()} elements differ; first (index..., got, want): {first}"
    if g.dim() == 4:
        ch = torch.unique(idx[:, 3])
        msg += f"; {len(ch)} distinct channels (lowest {int(ch.min())}, highest {int(ch.max())})"
        if tile is not None:
            tiles = torch.unique(torch.stack([idx[:, 0], idx[:, 1] // tile[0], idx[:, 2] // tile[1]], 1), dim=0)
            msg += f", {len(tiles)} distinct {tile[0]} x {tile[1]} pixel tiles of {g.shape[0] * -(-g.shape[1] // tile[0]) * -(-g.shape[2] // tile[1])}"
            msg += f" (first tile: image {int(tiles[0][0])}, tile row {int(tiles[0][1])}, tile column {int(tiles[0][2])})"
    raise AssertionError(msg)


DATA_KINDS = ("uniform", "int")


def parametrize_kinds(argnames, cases):
    """pytest.mark.parametrize over cases x DATA_KINDS, the kind as the last argument `data`.  The "uniform" parametrisation keeps the
    id the case has without the kind (`case3`, `2-20-37-32`), the integer one appends `-int`."""
    import pytest
    names = [n.strip() for n in argnames.split(",")]
    params = []
    for i, c in enumerate(cases):
        vals = (c,) if len(names) == 1 else tuple(c)
        base = f"{names[0]}{i}" if len(names) == 1 else "-".join(str(v) for v in vals)
        params += [pytest.param(*vals, "uniform", id=base), pytest.param(*vals, "int", id=base + "-int")]
    return pytest.mark.parametrize(",".join(names + ["data"]), params)


def nhwc(t_nchw):
    return t_nchw.permute(0, 2, 3, 1).contiguous()
