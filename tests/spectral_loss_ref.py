"""fp64 references of the multi-resolution STFT loss (csrc/spectralloss.hip), shared by the CPU and GPU tests.

(a) `loss` / `autograd`: the definition as literal torch fp64 expressions on `torch.stft` (the centred periodic Hann padded to n_fft,
    center=True, pad_mode="reflect", onesided=True); the gradient comes from autograd.
(b) `closed_form`: the derivation of the kernel file's header in NumPy (explicit DFT matrices, the adjoint DFT, overlap-add and the
    reflect fold), which also returns, per element of dwav, the sum of the absolute values of the terms that made it, and the number
    of terms.  The per-element bound of the GPU tests is

        |dev - ref| <= 2^-24 |ref| + n_terms 2^-53 abs          (one rounding to fp32 + sequential fp64 summation)

How abs and n_terms are made.  u = 2^-53; everything is first order in u; "n" below is one count that is at least every stage's own
count, so each stage only has to name an `abs` with (stage error) <= n u abs, on the device and in this reference alike - n_terms is
twice n, for the two sides.  Per row and resolution, x_f[n] = w[n] x_pad[f h + n], a_f = sum_n |x_f[n]|:
  - Re X, Im X are sums of `win` products with a twiddle of modulus <= 1 that is itself off by up to 16 u (the argument 2 pi m / N
    rounded before the cosine, here; a few ulp of sincospi there): |err| <= (win + 16) u a_f.
  - E0 (T non-negative terms) and sum w^2 (N of them) carry T u and N u relative however they are paired, so delta P0 carries
    (T + N + 8) u.  S = |X|^2 + delta P0 then errs by 2 |Re| eRe + 2 |Im| eIm + (T + N + 8) u delta P0, and M = sqrt(S) by that over
    2 M plus its own rounding: with |X| <= M and delta P0 <= M^2,  eM <= (win + 16) u sqrt2 a_f + ((T + N) / 2 + 6) u M
    <= n u abs_M,  abs_M = 1.5 a_f + M,  n >= win + (T + N) / 2 + 24.
  - The cancellation D1 = M_y^ - M_y:  abs_D1 = abs_M_y^ + abs_M_y (which is >= |D1|, paying for the subtraction).
  - ln M errs by eM / M and two ulp of |ln M|; the cancellation D2 = ln M_y^ - ln M_y:
    abs_D2 = abs_M_y^ / M_y^ + abs_M_y / M_y + |ln M_y^| + |ln M_y|   (>= |D2|).
  - The row sum W = sum M_y^2: F K positive terms, (F K + 4) u relative from the summation however it is paired, plus the terms' own
    2 eM / M:  eW / W <= n u rel_W,  rel_W = 1 + 2 sum(M_y abs_M_y) / W,  n >= F K + 4.
  - g = c [scw 2 D1 / W + lw 2 D2 / (F K M_y^)] / M_y^:  a quotient's error is the numerator's over the denominator plus the
    quotient times the denominators' relative errors (eW / W, eM / M) and a handful of roundings (6 u <= n u):
    abs_g = c scw 2 / (W M_y^) [abs_D1 + |D1| (rel_W + abs_M_y^ / M_y^ + 1)] + c lw 2 / (F K M_y^^2) [abs_D2 + |D2| (2 abs_M_y^ / M_y^ + 1)].
  - dRe = g Re X^:  abs_dRe = abs_g |Re| + |g| a_f;  dIm alike.
  - a frame of the adjoint, w[n] sum_k (dRe cos - dIm sin): 2 K terms of modulus <= |dRe| + |dIm| summed with (2 K + 16) u, plus the
    terms' own errors:  abs = w[n] A_f,  A_f = sum_k (abs_dRe + abs_dIm + |dRe| + |dIm|),  n >= 2 K + 16.
  - the overlap-add and the fold: at most 3 (ceil(win / h) + 1) frames per resolution reach a sample, R resolutions; abs[t] is the
    same gather of w[n] A_f, and the count 3 R max_r (ceil(win / h) + 1) is added to n.
  n = max_r (win + (T + N) / 2 + F K + 64) + 3 R max_r (ceil(win / h) + 1);  n_terms = 2 n.
The sums of `spectral_out` get allowances from the same pieces (`spectral_out_tol`).  Nothing here was measured on, or adjusted to, a
kernel's output.

All take the fp32 values the kernels get."""
import math

import numpy as np
import torch

import decay_loss_ref as DR
from oracle import features as FO

U53 = 2.0 ** -53
TWO_PI = 2.0 * math.pi
DEFAULT = ((128, 64, 32), (512, 256, 128), (1024, 512, 256))

# single-resolution cases (T, n_fft, win, hop) of the GPU test: T just past the reflect limit; an odd window shorter than the transform
# and a hop that divides nothing; bins either side of one bin tile (64); frames either side of a frame tile (16); fewer frames than one
# frame tile; the response length at the finest and the coarsest default resolution; the largest T
SINGLE = ((9, 16, 16, 4), (100, 16, 7, 3), (257, 64, 64, 16), (1000, 128, 64, 32), (1000, 256, 100, 37), (2400, 1024, 512, 256),
          (9600, 128, 64, 32), (9600, 1024, 512, 256), (16384, 512, 256, 128))
MULTI = ((9600, DEFAULT), (1000, ((64, 64, 16), (256, 100, 37))))
BATCHES = (1, 3)
FLOORS = (30.0, 60.0)

inputs = DR.inputs
bound = DR.bound
bound_accumulated = DR.bound_accumulated


# ------------------------------------------------------------------------------------------------------------ (a) torch
def t_stft(x, n_fft, win, hop):
    """[B, T] fp64 -> complex [B, K, F]"""
    w = torch.from_numpy(FO.hann_padded(n_fft, win)).to(x.dtype)
    return torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect", normalized=False,
                      onesided=True, return_complex=True)


def terms(wav_pred, wav_true, resolutions, floor_db):
    """(SC [B, R], LM [B, R], counted [B] bool) for fp64 tensors [B, T]"""
    delta = 10.0 ** (-floor_db / 10.0)
    T = wav_true.shape[-1]
    e0 = (wav_true * wav_true).sum(dim=-1)
    ok = e0 != 0
    safe = torch.where(ok, e0, torch.ones_like(e0))
    sc, lm = [], []
    for n_fft, win, hop in resolutions:
        w = torch.from_numpy(FO.hann_padded(n_fft, win)).to(wav_true.dtype)
        dp0 = (delta * (w * w).sum() * safe / T)[:, None, None]
        Mp = torch.sqrt(t_stft(wav_pred, n_fft, win, hop).abs() ** 2 + dp0)
        My = torch.sqrt(t_stft(wav_true, n_fft, win, hop).abs() ** 2 + dp0)
        s = ((Mp - My) ** 2).sum(dim=(1, 2)) / (My ** 2).sum(dim=(1, 2))
        m = ((torch.log(Mp) - torch.log(My)) ** 2).mean(dim=(1, 2))
        sc.append(torch.where(ok, s, torch.zeros_like(s)))
        lm.append(torch.where(ok, m, torch.zeros_like(m)))
    return torch.stack(sc, dim=1), torch.stack(lm, dim=1), ok


def loss(wav_pred, wav_true, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0, global_batch=None):
    gb = wav_pred.shape[0] if global_batch is None else global_batch
    sc, lm, _ = terms(wav_pred, wav_true, resolutions, floor_db)
    return weight / gb * (sc_weight * sc + log_weight * lm).mean(dim=1).sum()


def autograd(wp32, wt32, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0, global_batch=None):
    """(loss value, d loss / d wav_pred fp64 [B, T]) at the fp32 values wp32"""
    p = torch.from_numpy(np.array(wp32)).double().requires_grad_(True)
    val = loss(p, torch.from_numpy(np.array(wt32)).double(), resolutions, floor_db, sc_weight, log_weight, weight, global_batch)
    val.backward()
    return float(val.detach()), p.grad.detach().numpy()


# ------------------------------------------------------------------------------------------------------ (b) closed form
def n_terms(T, resolutions):
    stage = max(win + (T + N) // 2 + (1 + T // hop) * (N // 2 + 1) + 64 for N, win, hop in resolutions)
    ola = 3 * len(resolutions) * max(-(-win // hop) + 1 for N, win, hop in resolutions)
    return 2 * (stage + ola)


def _fold(frames, T, N, hop):
    """overlap-add of [F, N] frames at padded positions f hop + n, then the reflect fold onto [0, T)"""
    half = N // 2
    p = np.zeros(T + N)
    for f in range(frames.shape[0]):
        p[f * hop:f * hop + N] += frames[f]
    out = p[half:half + T].copy()
    j = np.arange(half)
    np.add.at(out, half - j, p[j])                                   # j < N/2 reads sample N/2 - j
    j = np.arange(T + half, T + N)
    np.add.at(out, 2 * (T - 1) - (j - half), p[j])                   # j >= T + N/2 reads sample 2 (T - 1) - (j - N/2)
    return out


def closed_form(wp32, wt32, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0, global_batch=None):
    """dict: dwav, abs fp64 [B, T]; n_terms; SC, LM [B, R]; counted [B]; spectral_out (3,) = (sum_b mean_r SC, sum_b mean_r LM, rows
    counted); spectral_out_tol (3,); loss = weight / global_batch (sc_weight spectral_out[0] + log_weight spectral_out[1])"""
    yp = np.asarray(wp32, dtype=np.float32).astype(np.float64)
    yt = np.asarray(wt32, dtype=np.float32).astype(np.float64)
    B, T = yp.shape
    R = len(resolutions)
    gb = B if global_batch is None else global_batch
    c = weight / gb / R
    delta = 10.0 ** (-floor_db / 10.0)
    nt = n_terms(T, resolutions)
    dwav, abs_ = np.zeros((B, T)), np.zeros((B, T))
    SC, LM, SC_tol, LM_tol = np.zeros((B, R)), np.zeros((B, R)), np.zeros((B, R)), np.zeros((B, R))
    counted = np.zeros(B, dtype=bool)
    for r, (N, win, hop) in enumerate(resolutions):
        half, F, K = N // 2, 1 + T // hop, N // 2 + 1
        w = FO.hann_padded(N, win)
        at = np.arange(F)[:, None] * hop + np.arange(N)[None, :] - half            # sample index of frame f, tap n, before the reflection
        at = np.abs(at)
        at = np.where(at >= T, 2 * (T - 1) - at, at)
        kn = (np.arange(K)[:, None] * np.arange(N)[None, :]) % N
        Cm, Sm = np.cos(TWO_PI * kn / N), np.sin(TWO_PI * kn / N)
        for b in range(B):
            e0 = (yt[b] * yt[b]).sum()
            if e0 == 0.0:
                continue
            counted[b] = True
            dp0 = delta * ((w * w).sum() * e0 / T)
            xp, xt = w[None, :] * yp[b][at], w[None, :] * yt[b][at]
            a_p, a_t = np.abs(xp).sum(axis=1)[:, None], np.abs(xt).sum(axis=1)[:, None]
            Re, Im = xp @ Cm.T, -(xp @ Sm.T)
            Mp = np.sqrt(Re * Re + Im * Im + dp0)
            My = np.sqrt((xt @ Cm.T) ** 2 + (xt @ Sm.T) ** 2 + dp0)
            D1, D2 = Mp - My, np.log(Mp) - np.log(My)
            W = (My * My).sum()
            SC[b, r], LM[b, r] = (D1 * D1).sum() / W, (D2 * D2).sum() / (F * K)
            abs_Mp, abs_My = 1.5 * a_p + Mp, 1.5 * a_t + My
            abs_D1 = abs_Mp + abs_My
            abs_D2 = abs_Mp / Mp + abs_My / My + np.abs(np.log(Mp)) + np.abs(np.log(My))
            rel_W = 1.0 + 2.0 * (My * abs_My).sum() / W
            g = c * (sc_weight * 2.0 * D1 / W + log_weight * 2.0 * D2 / (F * K * Mp)) / Mp
            abs_g = (c * sc_weight * 2.0 / (W * Mp) * (abs_D1 + np.abs(D1) * (rel_W + abs_Mp / Mp + 1.0)) +
                     c * log_weight * 2.0 / (F * K * Mp * Mp) * (abs_D2 + np.abs(D2) * (2.0 * abs_Mp / Mp + 1.0)))
            dRe, dIm = g * Re, g * Im
            A_f = (abs_g * (np.abs(Re) + np.abs(Im)) + 2.0 * np.abs(g) * a_p + np.abs(dRe) + np.abs(dIm)).sum(axis=1)
            dwav[b] += _fold(w[None, :] * (dRe @ Cm - dIm @ Sm), T, N, hop)
            abs_[b] += _fold(w[None, :] * A_f[:, None], T, N, hop)
            e1, e2 = nt * U53 * abs_D1, nt * U53 * abs_D2
            SC_tol[b, r] = (2.0 * np.abs(D1) * e1 + e1 * e1).sum() / W + SC[b, r] * nt * U53 * rel_W
            LM_tol[b, r] = (2.0 * np.abs(D2) * e2 + e2 * e2).sum() / (F * K) + LM[b, r] * nt * U53
    out = np.array([SC.mean(axis=1).sum(), LM.mean(axis=1).sum(), float(counted.sum())])
    tol = np.array([SC_tol.mean(axis=1).sum() + (B + R + 8) * U53 * out[0], LM_tol.mean(axis=1).sum() + (B + R + 8) * U53 * out[1], 0.0])
    return {"dwav": dwav, "abs": abs_, "n_terms": nt, "SC": SC, "LM": LM, "counted": counted, "spectral_out": out, "spectral_out_tol": tol,
            "loss": weight / gb * (sc_weight * out[0] + log_weight * out[1])}
