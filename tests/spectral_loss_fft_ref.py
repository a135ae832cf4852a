"""References of the FFT form of the multi-resolution STFT loss (csrc/spectralloss_fft.hip), shared by the CPU and GPU tests.

`restatement`: the definition of tests/spectral_loss_ref.py as literal `torch.stft` expressions in fp32 / complex64 under autograd on
the CPU - the arithmetic the kernels restate (an fp32 transform and its adjoint; pocketfft's factorisation, not the kernels').  The fp64
truth is `spectral_loss_ref.autograd` / `terms`.  With e(v) = max_t |v - dwav64| / max_t |dwav64| per row, the kernels are held to

    e(kernel) <= 4 e(restatement) + 2^-22                                  (e(restatement) computed on the same data)
    |scalar - scalar64| <= 64 log2(N_max) 2^-24 |scalar64|                 (spectral_out[0:2], the loss_out increment)

`restatement(..., mutation=)` is the same with one line changed - the mistakes a kernel of this kind makes: "nyquist" (bin N/2
dropped), "nofold" (the reflected edge not folded back: nothing flows through the padding), "shift" (the window one tap late),
"nofloor" (delta P0 left out).  Each must fail one of the two checks on every case, or the checks would say nothing."""
import functools
import math

import numpy as np
import torch

import spectral_loss_ref as SR
from oracle import features as FO

DEFAULT = SR.DEFAULT
# (T, n_fft, win, hop): the least T (every sample reflected); an odd window and hop, many frames, a ragged last workgroup; each n_fft; a
# window that is no multiple of anything; the largest T
SINGLE = ((65, 128, 128, 32), (100, 128, 7, 3), (1000, 128, 64, 32), (1000, 256, 100, 37), (700, 512, 256, 128), (2400, 1024, 512, 256),
          (16384, 512, 256, 128))
MULTI = ((9600, DEFAULT), (1000, ((128, 64, 16), (256, 100, 37))))
CASES = [(c[0], (tuple(c[1:]),)) for c in SINGLE] + list(MULTI)
IDS = ["-".join(map(str, (T,) + tuple(v for r in res for v in r))) for T, res in CASES]
BATCHES = (1, 3)
FLOORS = (30.0, 60.0)
MUTATIONS = ("nyquist", "nofold", "shift", "nofloor")
KW = dict(sc_weight=0.8, log_weight=1.3, weight=0.7, global_batch=4)


def inputs(T, B=3):
    """Read-only fp32 (wav_pred, wav_true) [B, T]: independent uniform noise in (-1, 1)"""
    rng = np.random.default_rng(7100 + T)
    yp = rng.uniform(-1.0, 1.0, (B, T)).astype(np.float32)
    yt = rng.uniform(-1.0, 1.0, (B, T)).astype(np.float32)
    yp.setflags(write=False)
    yt.setflags(write=False)
    return yp, yt


def scalar_bound(resolutions):
    """the relative allowance of spectral_out[0:2] and of the loss_out increment: 6.66 u per radix-2 level in L2 (Higham, Theorem 24.2),
    twice for M_y^ - M_y, twice for the square, |M| / |M_y^ - M_y| <= 2 on independent data: 53 log2(N) u, rounded up"""
    return 64.0 * math.log2(max(r[0] for r in resolutions)) * 2.0 ** -24


def rel_err(v, truth):
    """e(v) per row"""
    return np.abs(np.asarray(v, dtype=np.float64) - truth).max(axis=1) / np.abs(truth).max(axis=1)


def _stft32(x, n_fft, win, hop, mutation):
    w = torch.from_numpy(FO.hann_padded(n_fft, win)).float()
    if mutation == "shift":
        w = torch.roll(w, 1)
    if mutation == "nofold":
        pad = torch.nn.functional.pad(x[:, None, :], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0, :].detach()
        x = torch.cat((pad[:, :n_fft // 2], x, pad[:, -(n_fft // 2):]), dim=1)
    X = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w, center=mutation != "nofold", pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    return X[:, :-1, :] if mutation == "nyquist" else X


def restatement(wp32, wt32, resolutions, floor_db=60.0, sc_weight=1.0, log_weight=1.0, weight=1.0, global_batch=None, mutation=None):
    """dict: dwav fp32 [B, T] (autograd); SC, LM fp32 [B, R]; spectral_out (3,) and loss as fp64 sums of the fp32 terms"""
    p = torch.from_numpy(np.array(wp32, dtype=np.float32)).requires_grad_(True)
    y = torch.from_numpy(np.array(wt32, dtype=np.float32))
    B, T = y.shape
    gb = B if global_batch is None else global_batch
    delta = 10.0 ** (-floor_db / 10.0)
    e0 = (y * y).sum(dim=-1)
    ok = e0 != 0
    safe = torch.where(ok, e0, torch.ones_like(e0))
    sc, lm = [], []
    for n_fft, win, hop in resolutions:
        w = torch.from_numpy(FO.hann_padded(n_fft, win)).float()
        dp0 = (delta * (w * w).sum() * safe / T)[:, None, None] * (0.0 if mutation == "nofloor" else 1.0)
        Mp = torch.sqrt(_stft32(p, n_fft, win, hop, mutation).abs() ** 2 + dp0)
        My = torch.sqrt(_stft32(y, n_fft, win, hop, mutation).abs() ** 2 + dp0)
        s = ((Mp - My) ** 2).sum(dim=(1, 2)) / (My ** 2).sum(dim=(1, 2))
        m = ((torch.log(Mp) - torch.log(My)) ** 2).mean(dim=(1, 2))
        sc.append(torch.where(ok, s, torch.zeros_like(s)))
        lm.append(torch.where(ok, m, torch.zeros_like(m)))
    sc, lm = torch.stack(sc, dim=1), torch.stack(lm, dim=1)
    val = weight / gb * (sc_weight * sc + log_weight * lm).mean(dim=1).sum()
    val.backward()
    SC, LM = sc.detach().numpy().astype(np.float64), lm.detach().numpy().astype(np.float64)
    out = np.array([SC.mean(axis=1).sum(), LM.mean(axis=1).sum(), float(ok.sum())])
    return {"dwav": p.grad.numpy(), "SC": SC, "LM": LM, "spectral_out": out,
            "loss": weight / gb * (sc_weight * out[0] + log_weight * out[1])}


@functools.lru_cache(maxsize=None)
def truth(T, res, floor_db):
    """fp64, three rows (a row's figures do not depend on the batch: global_batch is fixed): dict dwav [3, T]; SC, LM [3, R]"""
    yp, yt = inputs(T)
    _, grad = SR.autograd(yp, yt, res, floor_db, **KW)
    sc, lm, ok = SR.terms(torch.from_numpy(np.array(yp)).double(), torch.from_numpy(np.array(yt)).double(), res, floor_db)
    assert bool(ok.all())
    return {"dwav": grad, "SC": sc.numpy(), "LM": lm.numpy()}


def truth_scalars(tr, B):
    """(spectral_out (3,), loss) of the first B rows"""
    out = np.array([tr["SC"][:B].mean(axis=1).sum(), tr["LM"][:B].mean(axis=1).sum(), float(B)])
    return out, KW["weight"] / KW["global_batch"] * (KW["sc_weight"] * out[0] + KW["log_weight"] * out[1])


@functools.lru_cache(maxsize=None)
def restated(T, res, floor_db, mutation=None):
    yp, yt = inputs(T)
    return restatement(yp, yt, res, floor_db, **KW, mutation=mutation)


def passes(got, T, res, floor_db):
    """whether a result dict (dwav, spectral_out, loss) of three rows passes the two checks of the kernels -> (dwav ok, scalars ok)"""
    tr, rs = truth(T, res, floor_db), restated(T, res, floor_db)
    tol = 4.0 * rel_err(rs["dwav"], tr["dwav"]) + 2.0 ** -22
    want, loss = truth_scalars(tr, 3)
    sb = scalar_bound(res)
    scal = (np.abs(got["spectral_out"][:2] - want[:2]) <= sb * want[:2]).all() and abs(got["loss"] - loss) <= sb * loss
    return bool((rel_err(got["dwav"], tr["dwav"]) <= tol).all()), bool(scal)
