"""Element-wise criterion for the streaming (HBM-bound) kernels of csrc/elementwise.hip, and the fp64 references they are held to.

A comparison "within tol of the tensor's LARGEST value" cannot see an error that is small against that value: a truncating bf16
store, one channel vector with its neighbour's parameters, a slab of rows missing from a sum over 10^5 pixels.  Here EVERY element
has a bound of its own, derived from the arithmetic the kernel performs and from nothing the kernel returns:

  fp32 outputs   |got - ref| <= d,  d = k * 2^-24 * S: ref the fp64 evaluation, S the fp64 sum of the absolute values of the terms
                 the formula adds for that element, k the number of fp32 roundings of the kernel's expression (a contracted fma
                 only lowers it; derivations beside each k below).
  bf16 outputs   with the same d: the value the kernel holds before its store lies in [ref - d, ref + d], and rounding to bf16 is
                 monotone, so the stored value lies in [bf16(ref - d), bf16(ref + d)] (round to nearest even, from fp64 in ONE
                 rounding).  Where the two ends agree the element is DECIDED and must equal bf16(ref); elsewhere it must be one of
                 the candidates (the two ends; where heavy cancellation makes d exceed the bf16 spacing at ref, any bf16 value
                 between them).  The share of undecided elements is asserted to be at most CAP = 1 % - from the reference alone,
                 before the kernel's output is looked at.
  activations    ReLU / LeakyReLU are monotone, so they are applied to the two ends: act(ref - d), act(ref + d).  LeakyReLU's
                 product 0.3f * r is one more rounding on the negative side, relative to |r| <= S: k + 1.  The slope is the
                 fp32 number 0.3f, not 0.3.
  reductions     the kernels accumulate in fp64 in a fixed order; the bound is the final conversion to fp32 (2^-24 relative)
                 plus n * 2^-24 * sum |addend| for addends that are fp32 expressions with n roundings, plus the fp64
                 accumulation itself (P * 2^-53 * sum |addend|: any order of P additions), which matters only where a difference
                 of sums cancels (variance of a channel with mean 100 and spread 0.5).
  chained passes what a kernel reads from another kernel (affine, saved, dgamma / dbeta) is checked in an assertion of its own
                 and then READ BACK and used as given in the reference of the pass that consumes it.

CPU only (torch), importable without the product; tests/test_streaming_check.py proves on emulated kernels that the criterion
accepts both ways of rounding a multiply-add and rejects six realistic mutants."""
import torch

U32 = 2.0 ** -24            # unit roundoff of fp32, round to nearest: |fl(v) - v| <= U32 * |v|
U64 = 2.0 ** -53
TINY = 2.0 ** -149          # smallest fp32 subnormal: the absolute floor of every fp32 bound (gradual underflow)
SLOPE = float(torch.tensor(0.3, dtype=torch.float32))          # keras LeakyReLU() alpha as the kernels hold it (0.3f)
CAP = 0.01                  # largest share of undecided elements of a bf16 tensor
# per kernel: comparisons, compared elements, largest undecided share (bf16), largest |got - ref| / d (fp32)
STATS = {}


def _bf16_spacing(v):
    """Spacing of the bfloat16 numbers at the fp64 tensor v, an exact power of two assembled from its bits (torch.ldexp goes
    through pow() on a GPU, which is not exact there).  |v| = m * 2^e with m in [0.5, 1); bf16 keeps 8 bits of m; below the
    smallest normal number 2^-126 the spacing stays that of 2^-126."""
    _, e = torch.frexp(v)
    return ((e.to(torch.int64).clamp(min=-125) - 8 + 1023) << 52).view(torch.float64)


def bf16_rne(v):
    """fp64 -> nearest bfloat16 (ties to even) in ONE rounding, returned as fp64.  (Going through fp32 rounds twice: 1 + 2^-8 +
    2^-30 is above the tie 1 + 2^-8 and belongs to 1 + 2^-7, but its fp32 rounding IS the tie, which then goes to 1.)"""
    v = v.double()
    q = _bf16_spacing(v)
    return torch.round(v / q) * q                           # torch.round: half to even; v / q and the product are exact


def bf16_trunc(v):
    """fp64 -> bfloat16 by dropping bits (round toward zero): what a store that forgets to round does."""
    v = v.double()
    q = _bf16_spacing(v)
    return torch.trunc(v / q) * q


def activate(z, act):
    """act 0: identity, 1: ReLU, 2: LeakyReLU(0.3f) - r > 0 ? r : slope * r as the kernels write it."""
    if act == 0:
        return z
    return torch.where(z > 0, z, z * (SLOPE if act == 2 else 0.0))


def note(kernel, n, undecided=None, ratio=None):
    st = STATS.setdefault(kernel, dict(comparisons=0, elements=0, undecided=0.0, ratio=0.0))
    st["comparisons"] += 1
    st["elements"] += int(n)
    if undecided is not None:
        st["undecided"] = max(st["undecided"], float(undecided))
    if ratio is not None:
        st["ratio"] = max(st["ratio"], float(ratio))
    return st


def check(got, ref, d, what, kernel=None, act=0, cap=CAP):
    """Every element of `got` (fp32 or bf16, any device) against act(ref) with the pre-activation bound d (fp64, broadcastable),
    as the module docstring states.  Raises AssertionError naming the number of violations and the first ten."""
    ref = ref.double().to(got.device)
    d = torch.as_tensor(d, dtype=torch.float64, device=got.device).expand_as(ref) + TINY
    assert bool(torch.isfinite(ref).all()) and bool(torch.isfinite(d).all()), f"{what}: the reference is not finite"
    check_interval(got, activate(ref - d, act), activate(ref, act), activate(ref + d, act), what, kernel, cap, d)


def check_interval(got, lo, mid, hi, what, kernel=None, cap=CAP, d=None):
    """The comparison itself: the value the kernel holds before its store lies in [lo, hi] (fp64), mid is the reference.  fp32:
    lo <= got <= hi.  bf16: decided where bf16(lo) == bf16(hi), and then got == bf16(mid); else bf16(lo) <= got <= bf16(hi)."""
    assert tuple(got.shape) == tuple(mid.shape), (what, tuple(got.shape), tuple(mid.shape))
    g = got.double()
    if got.dtype == torch.bfloat16:
        lo, mid, hi = bf16_rne(lo), bf16_rne(mid), bf16_rne(hi)
        decided = lo == hi
        share = 1.0 - float(decided.double().mean())
        note(kernel or what, g.numel(), undecided=share)
        assert share <= cap, f"{what}: {share:.3%} of the elements are undecided (cap {cap:.0%}): shrink the data's range"
        bad = torch.where(decided, g != mid, ~((g >= lo) & (g <= hi)))
        kind = f"bf16, {share:.2e} undecided"
    else:
        assert got.dtype == torch.float32, got.dtype
        bad = ~((g >= lo) & (g <= hi))                      # a NaN fails both comparisons
        ok = ~bad
        ratio = float(((g - mid).abs() / d)[ok].max()) if d is not None and bool(ok.any()) else None
        note(kernel or what, g.numel(), ratio=ratio)
        kind = "fp32"
    n_bad = int(bad.sum())
    if n_bad == 0:
        return
    idx = bad.nonzero()[:10].cpu()
    first = [tuple(int(i) for i in ix) + tuple(float(t[tuple(ix)]) for t in (g, lo, mid, hi)) for ix in idx]
    raise AssertionError(f"{what} ({kind}): {n_bad} of {g.numel()} elements outside their bound; first (index..., got, lowest, want, highest): {first}")


def accepts(got, ref, d, act=0):
    """check() as a predicate (tests/test_streaming_check.py)."""
    try:
        check(got, ref, d, "predicate", kernel="(cpu proof)", act=act)
    except AssertionError:
        return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# fp64 references of the BatchNorm family with their bounds.  Tensors are [P, C] (pixels x channels), parameters [C].
# ----------------------------------------------------------------------------------------------------------------------
def stats_ref(x, eps):
    """mean, biased variance (two passes in fp64), rstd = 1 / sqrt(var + eps) and their bounds for chan_partial_kernel<0> +
    bn_finalize_kernel: fp64 sums of exact fp32 values and exact squares; var = ss / P - mean^2 in fp64; saved[c] = (float)mean and
    (float)(1 / sqrt(var + eps)) are stored straight from doubles: 2^-24 relative, plus the fp64 accumulation propagated:
    |d mean| <= P 2^-53 mean|x|;  |d var| <= P 2^-53 (mean(x^2) + 2 |mean| mean|x|);  |d rstd| = rstd^3 / 2 * |d var|."""
    x = x.double()
    P = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    mabs = x.abs().mean(0)
    e_mean = P * U64 * mabs
    e_var = P * U64 * ((x * x).mean(0) + 2 * mean.abs() * mabs)
    return dict(mean=mean, var=var, rstd=rstd, e_var=e_var,
                d_mean=U32 * mean.abs() + e_mean, d_rstd=U32 * rstd + 0.5 * rstd ** 3 * e_var)


def scale_ref(rstd_f, gamma):
    """scale = gamma * rstd from the STORED rstd (bn_finalize_kernel after its conversions): 1 rounding; gamma NULL: 1."""
    scale = rstd_f.double() * (1.0 if gamma is None else gamma.double())
    return scale, U32 * scale.abs()


def shift_ref(mean_f, scale_f, beta):
    """shift = beta - (float)mean * scale from the STORED mean and scale: product and difference, 2 roundings (an fma 1)."""
    t = mean_f.double() * scale_f.double()
    b = torch.zeros_like(t) if beta is None else beta.double()
    return b - t, 2 * U32 * (b.abs() + t.abs())


def moving_ref(moving0, batch_f, momentum):
    """moving = momentum * moving + (1.f - momentum) * batch in fp32: two products and a sum, 3 roundings (an fma 2), with the
    fp32 constants the kernel holds: momentum as float, 1.f - momentum rounded to float."""
    m = float(torch.tensor(momentum, dtype=torch.float32))
    om = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(momentum, dtype=torch.float32))
    a, b = m * moving0.double(), om * batch_f.double()
    return a + b, 3 * U32 * (a.abs() + b.abs()), om


def apply_ref(x, scale=None, shift=None, addend=None, act=0):
    """Pre-activation reference and bound of bn_apply_kernel: r = x * scale + shift (product, sum: k = 2, an fma 1; no affine:
    r = x, k = 0), r += addend (k + 1), LeakyReLU's 0.3f * r (k + 1, see the module docstring).  S = |x scale| + |shift| + |addend|."""
    x = x.double()
    if scale is None:
        ref, S, k = x, x.abs(), 0
    else:
        t = x * scale.double()
        ref, S, k = t + shift.double(), t.abs() + shift.double().abs(), 2
    if addend is not None:
        ref, S, k = ref + addend.double(), S + addend.double().abs(), k + 1
    if act == 2:
        k += 1
    return ref, k * U32 * S


def bwd_ref(x, da, mask, scale, mean_f, rstd_f, act, P=None):
    """The two sums of chan_partial_kernel<2> and their bounds, from the STORED mean / rstd and the given activation decisions
    `mask` (True: the activation passed the element):
      g  = mask ? da : (act == 2 ? 0.3f * da : 0)         kg = 1 rounding where a LeakyReLU element is masked, else exact
      xh = (x - mean) * rstd                                2 roundings (difference, product)
      dbeta = sum g, dgamma = sum (double)g * (double)xh    fp64 sums; the fp64 product of two floats is exact
    d(dbeta) = 2^-24 |dbeta| + 2^-24 sum kg |g| + P 2^-53 sum |g|;  d(dgamma) = 2^-24 |dgamma| + 2^-24 sum (2 + kg) |g xh| + P 2^-53 sum |g xh|."""
    x, da = x.double(), da.double()
    P = x.shape[0] if P is None else P
    g = torch.where(mask, da, da * (SLOPE if act == 2 else 0.0)) if act else da
    kg = ((~mask).double() if act == 2 else torch.zeros_like(g))
    xh = (x - mean_f.double()) * rstd_f.double()
    gx = g * xh
    dbeta, dgamma = g.sum(0), gx.sum(0)
    d_dbeta = U32 * dbeta.abs() + U32 * (kg * g.abs()).sum(0) + P * U64 * g.abs().sum(0)
    d_dgamma = U32 * dgamma.abs() + U32 * ((2 + kg) * gx.abs()).sum(0) + P * U64 * gx.abs().sum(0)
    return dict(g=g, kg=kg, xh=xh, dbeta=dbeta, dgamma=dgamma, d_dbeta=d_dbeta, d_dgamma=d_dgamma)


def dx_ref(r, scale, dbeta_f, dgamma_f, P):
    """dx = scale * (g - c1 - xh * c2) of bn_bwd_apply_kernel with c1 = dbeta / P, c2 = dgamma / P from the STORED dbeta / dgamma
    (the kernel's coef[] holds (float)(s / P) of the same fp64 sums: each differs from the stored sum / P by two conversions).
    Roundings: g - c1, xh * c2, the difference, the product with scale: 4, each on a partial result of at most
    |g| + |c1| + |xh c2|; inside the terms: kg on g, 2 (the conversions) on c1, 2 (xh) + 2 (the conversions) on xh * c2:
    d = 2^-24 |scale| ((4 + kg) |g| + 6 |c1| + 8 |xh c2|)."""
    c1, c2 = dbeta_f.double() / P, dgamma_f.double() / P
    sc = scale.double()
    t = r["xh"] * c2
    ref = sc * (r["g"] - c1 - t)
    d = U32 * sc.abs() * ((4 + r["kg"]) * r["g"].abs() + 6 * c1.abs() + 8 * t.abs())
    return ref, d


def masked_grad(da, mask, act):
    """g = mask ? da : (act == 2 ? 0.3f * da : 0) as the fp32 number the kernels hold: one IEEE product of exact inputs, so
    the value is DETERMINED - no bound is needed (act_bwd, relu_bwd, gskip without an addend: equality in every element)."""
    gv = da.float()
    if not act:
        return gv
    return torch.where(mask, gv, gv * (torch.tensor(SLOPE, dtype=torch.float32, device=gv.device) if act == 2 else 0.0))


def gskip_interval(da, mask, act, addend=None):
    """(lowest, reference, highest) of gskip = g (+ gskip_add) before its store.  g is determined (masked_grad) and g + addend is
    ONE fp32 addition of two exact numbers, so the sum is determined as well - a bound of 2^-24 (|g| + |addend|) would leave
    every exact tie of the bf16 store undecided, and a sum of two bf16 numbers is a tie in several per cent of the elements.
    Only the masked LeakyReLU elements have two possible evaluations: fl(fl(0.3f da) + addend) and the contracted
    fl(0.3f da + addend); the interval spans the two."""
    g = masked_grad(da, mask, act)
    if addend is None:
        g = g.double()
        return g, g, g
    sep = (g + addend.float()).double()
    if act != 2:
        return sep, sep, sep
    fma = torch.where(mask, sep, (da.double() * SLOPE + addend.double()).float().double())
    return torch.minimum(sep, fma), sep, torch.maximum(sep, fma)


def old_close(actual, expected, tol):
    """The criterion the kernel tests used so far, as a predicate: max |a - e| <= tol * max |e|."""
    a, e = actual.double(), expected.double()
    return float((a - e).abs().max()) <= tol * (float(e.abs().max()) + 1e-30)
