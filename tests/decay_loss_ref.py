"""fp64 references of the decay loss (csrc/decayloss.hip) and of the vector-Jacobian product of PostProcess (csrc/istft_bwd.hip),
shared by the CPU and GPU tests.

(a) `loss` / `autograd`: the loss as literal torch fp64 expressions (flip / cumsum / log10); the gradient comes from autograd.
    `vjp_autograd`: the torch fp64 chain of tests/wave_loss_ref.py (t_denormalize, t_istft) under autograd with a given cotangent.
(b) `closed_form`: the derivation of the kernel file's header in NumPy, which also returns, per element of dwav, the sum of the
    absolute values of the terms that made it, and the number of terms; `vjp_closed_form`: the linear part of
    wave_loss_ref.closed_form with u = dwav / env, abs carried the same way.  The per-element bound of the GPU tests is

        |dev - ref| <= 2^-24 |ref| + n_terms 2^-53 abs          (one rounding to fp32 + sequential fp64 summation)

How abs and n_terms of the decay loss are made.  With u = 2^-53 and K = 10 / ln 10:
  - S[t] and E0 are sums of at most T non-negative terms: however paired, each carries a relative error of at most T u, on the device
    and in this reference alike.  The argument S / E0 + delta of a logarithm so carries (2 T + 3) u relative on each side, which
    moves c = 10 log10(.) by K times that: the logarithms' arguments are paid for with K per logarithm, 2 K in abs_d.
  - The cancellation d = c_y^ - c_y is paid for with |c_y^| + |c_y| (the logarithm's own few ulp, and the subtraction).
    abs_d[t] = |c_y^[t]| + |c_y[t]| + 2 K, good for 2 (2 T + 3) + 8 terms.
  - g[t] = (2 / T) K d[t] / (S_y^[t] + delta E0): abs_g[t] = (2 / T) K abs_d[t] / (S_y^[t] + delta E0); the denominator's relative error,
    (T + 3) u on each side, multiplies |g| <= abs_g: 2 T + 6 more terms.
  - G[s] = sum_{t <= s} g[t]: at most T terms on each side, 2 T more, on sum_{t <= s} abs_g[t].
  - dwav[s] = weight / global_batch 2 y^[s] G[s]: abs[s] = weight / global_batch 2 |y^[s]| sum_{t <= s} abs_g[t], a few roundings.
  n_terms = 8 T + 64.  Nothing here was measured on, or adjusted to, a kernel's output.

All take the fp32 values the kernels get."""
import math

import numpy as np
import torch

import features_check as FK
import wave_loss_ref as WR
from oracle import features as FO

K10 = 10.0 / math.log(10.0)
U53 = 2.0 ** -53

# the shapes of the GPU test: one sample, two, either side of a wave (64), an odd size past one sample per thread of four waves, one
# that is no multiple of four, one past a run of four per thread (4096: the next run length), the response length, and the largest
LENGTHS = (1, 2, 63, 64, 65, 257, 1000, 4097, 9600, 16384)
BATCHES = (1, 3)
FLOORS = (30.0, 60.0)


def inputs(T, B=3):
    """Read-only fp32 (wav_pred, wav_true) [B, T]: uniform noise under an exponential envelope.  The target's energy decays by 60 dB
    over 0.55 T .. 0.7 T samples (row by row), so for the long cases both curves run into the floor inside the row; the prediction
    decays at 0.8 of the target's time constant and sits 2 dB low - a rate error and a level error."""
    rng = np.random.default_rng(9000 + T)
    t = np.arange(T, dtype=np.float64)
    yp, yt = np.empty((B, T), np.float32), np.empty((B, T), np.float32)
    for b in range(B):
        tau = max((0.55 + 0.075 * b) * T, 2.0) / (3.0 * math.log(10.0))          # energy e^(-2 t / tau): -60 dB at 3 ln 10 tau
        yt[b] = (rng.uniform(-1.0, 1.0, T) * np.exp(-t / tau)).astype(np.float32)
        yp[b] = (10.0 ** (-2.0 / 20.0) * rng.uniform(-1.0, 1.0, T) * np.exp(-t / (0.8 * tau))).astype(np.float32)
    yp.setflags(write=False)
    yt.setflags(write=False)
    return yp, yt


# ------------------------------------------------------------------------------------------------------------ (a) torch
def curves(x, e0, delta):
    """10 log10(S[t] / E0 + delta) with S the backward integral of x^2 along the last axis"""
    S = torch.flip(torch.cumsum(torch.flip(x * x, dims=(-1,)), dim=-1), dims=(-1,))
    return 10.0 * torch.log10(S / e0 + delta)


def q_terms(wav_pred, wav_true, floor_db):
    """(Q [B], counted [B] bool) for fp64 tensors [B, T]"""
    delta = 10.0 ** (-floor_db / 10.0)
    e0 = (wav_true * wav_true).sum(dim=-1, keepdim=True)
    ok = e0[:, 0] != 0
    safe = torch.where(e0 != 0, e0, torch.ones_like(e0))
    d = curves(wav_pred, safe, delta) - curves(wav_true, safe, delta)
    Q = (d * d).mean(dim=-1)
    return torch.where(ok, Q, torch.zeros_like(Q)), ok


def loss(wav_pred, wav_true, floor_db=60.0, weight=1.0, global_batch=None):
    gb = wav_pred.shape[0] if global_batch is None else global_batch
    return weight / gb * q_terms(wav_pred, wav_true, floor_db)[0].sum()


def autograd(wp32, wt32, floor_db=60.0, weight=1.0, global_batch=None):
    """(loss value, d loss / d wav_pred fp64 [B, T]) at the fp32 values wp32"""
    p = torch.from_numpy(np.array(wp32)).double().requires_grad_(True)
    val = loss(p, torch.from_numpy(np.array(wt32)).double(), floor_db, weight, global_batch)
    val.backward()
    return float(val.detach()), p.grad.detach().numpy()


def vjp_autograd(pred32, dwav, des_shape, n_fft, win, hop, phase_ref=None):
    """(d y^ / d pred)^T dwav, fp64 [B, 2, H, W], by autograd through wave_loss_ref.t_waveform"""
    p = torch.from_numpy(np.array(pred32)).double().requires_grad_(True)
    ref = None if phase_ref is None else torch.from_numpy(np.array(phase_ref))
    wav = WR.t_waveform(p, des_shape, n_fft, win, hop, ref)
    (wav * torch.from_numpy(np.asarray(dwav, dtype=np.float64))).sum().backward()
    return p.grad.detach().numpy()


# ------------------------------------------------------------------------------------------------------ (b) closed form
def n_terms(T):
    return 8 * T + 64


def closed_form(wp32, wt32, floor_db=60.0, weight=1.0, global_batch=None):
    """dict: dwav, abs fp64 [B, T]; n_terms; Q [B]; counted [B]; decay_out (2,) = (sum_b Q_b, rows counted); decay_out_tol (2,);
    loss = weight / global_batch decay_out[0]; c_pred, c_true [B, T] (rows that are not counted: zeros)"""
    yp = np.asarray(wp32, dtype=np.float32).astype(np.float64)
    yt = np.asarray(wt32, dtype=np.float32).astype(np.float64)
    B, T = yp.shape
    gb = B if global_batch is None else global_batch
    k = weight / gb
    delta = 10.0 ** (-floor_db / 10.0)
    nt = n_terms(T)
    n_d = 2 * (2 * T + 3) + 8
    dwav, abs_, cp_all, ct_all = np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T)), np.zeros((B, T))
    Q, Q_tol, counted = np.zeros(B), np.zeros(B), np.zeros(B, dtype=bool)
    for b in range(B):
        Sp = np.cumsum((yp[b] * yp[b])[::-1])[::-1]
        St = np.cumsum((yt[b] * yt[b])[::-1])[::-1]
        e0 = St[0]
        if e0 == 0.0:
            continue
        counted[b] = True
        cp, ct = 10.0 * np.log10(Sp / e0 + delta), 10.0 * np.log10(St / e0 + delta)
        d = cp - ct
        abs_d = np.abs(cp) + np.abs(ct) + 2.0 * K10
        den = Sp + delta * e0
        g = (2.0 / T) * K10 * d / den
        abs_g = (2.0 / T) * K10 * abs_d / den
        dwav[b] = k * 2.0 * yp[b] * np.cumsum(g)
        abs_[b] = k * 2.0 * np.abs(yp[b]) * np.cumsum(abs_g)
        Q[b] = (d * d).sum() / T
        e_d = n_d * U53 * abs_d
        Q_tol[b] = (2.0 * np.abs(d) * e_d + e_d * e_d).sum() / T + (2 * T + 8) * U53 * Q[b]
        cp_all[b], ct_all[b] = cp, ct
    out = np.array([Q.sum(), float(counted.sum())])
    tol = np.array([Q_tol.sum() + (B + 8) * U53 * Q.sum(), 0.0])
    return {"dwav": dwav, "abs": abs_, "n_terms": nt, "Q": Q, "counted": counted, "decay_out": out, "decay_out_tol": tol,
            "loss": k * Q.sum(), "c_pred": cp_all, "c_true": ct_all}


def vjp_n_terms(des_shape, n_fft, win, hop):
    """the envelope's terms of one sample, the 2 win terms of the DFT and 16 for the elementary functions (wave_loss_ref.n_terms
    without the synthesis and the partial sums, which the cotangent does not pass through)"""
    return (-(-win // hop) + 1) + 2 * win + 16


def vjp_closed_form(pred32, dwav32, des_shape, n_fft, win, hop, phase_ref=None):
    """dict: grad, abs fp64 [B, 2, H, W] (zeros in rows >= n_bins and columns >= n_frames); n_terms"""
    pred = np.asarray(pred32, dtype=np.float32)
    B, _, H, W = pred.shape
    nb, nf = des_shape
    g = np.asarray(dwav32, dtype=np.float32).astype(np.float64)
    a = pred[:, 0, :nb, :nf].astype(np.float64)
    p32 = pred[:, 1, :nb, :nf]
    if phase_ref is not None:
        p32 = p32 + np.asarray(phase_ref, dtype=np.float32)[:, 1, :nb, :nf]
    e10 = 10.0 ** ((a * FO.MD - FO.MD) / 20.0)
    amp, ph = FO.denormalize(a, p32.astype(np.float64))
    env = FK.envelope(nf, n_fft, win, hop)
    live = env > FO.TINY32
    safe = np.where(live, env, 1.0)
    u = np.where(live, g / safe, 0.0)
    au = np.where(live, np.abs(g) / safe, 0.0)
    hann = FO.hann_padded(n_fft, win)
    at = np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]                    # padded coordinates of s_f[n]
    seg = np.pad(u, ((0, 0), (n_fft // 2, n_fft // 2)))[:, at] * hann[None, None, :]
    aseg = np.pad(au, ((0, 0), (n_fft // 2, n_fft // 2)))[:, at] * hann[None, None, :]
    kn = (np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    Cm, Sm = np.cos(WR.TWO_PI * kn / n_fft), np.sin(WR.TWO_PI * kn / n_fft)
    re, im = np.einsum("kn,bfn->bkf", Cm, seg), -np.einsum("kn,bfn->bkf", Sm, seg)
    ab = np.einsum("kn,bfn->bkf", np.abs(Cm), aseg) + np.einsum("kn,bfn->bkf", np.abs(Sm), aseg)
    c = np.full(nb, 2.0)
    c[0] = c[-1] = 1.0
    dre, dim = c[None, :, None] / n_fft * re, c[None, :, None] / n_fft * im
    dim[:, 0, :] = dim[:, -1, :] = 0.0
    cs, sn = np.cos(ph), np.sin(ph)
    grad, abs_ = np.zeros((B, 2, H, W)), np.zeros((B, 2, H, W))
    grad[:, 0, :nb, :nf] = (dre * cs + dim * sn) * WR.K_AMP * e10
    grad[:, 1, :nb, :nf] = WR.TWO_PI * amp * (dim * cs - dre * sn)
    abs_[:, 0, :nb, :nf] = c[None, :, None] / n_fft * ab * WR.K_AMP * e10
    abs_[:, 1, :nb, :nf] = WR.TWO_PI * np.abs(amp) * c[None, :, None] / n_fft * ab
    return {"grad": grad, "abs": abs_, "n_terms": vjp_n_terms(des_shape, n_fft, win, hop)}


def cotangent(name):
    """a read-only fp32 cotangent [B, T] for one geometry of tests/features_cases.py"""
    import features_cases as FC
    B = FC.GEOMETRIES[name][0]
    g = np.random.default_rng(sum(map(ord, name)) + 8100).standard_normal((B, FC.t_out(name))).astype(np.float32)
    g.setflags(write=False)
    return g


bound = WR.bound


def bound_accumulated(base32, ref, abs_, nt):
    """the allowance with accumulate: dev = fp32(base + g), so the rounding term is taken on the sum"""
    return 2.0 ** -24 * np.abs(np.asarray(base32, dtype=np.float64) + ref) + nt * U53 * abs_ + 2.0 ** -149
