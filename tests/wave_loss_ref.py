"""fp64 references of the waveform-domain loss (csrc/waveloss.hip), shared by the CPU and GPU tests.

(a) `loss` / `autograd`: the loss as literal torch fp64 expressions over oracle.features' un-pad / denormalise / istft arithmetic,
    restated in torch so that autograd runs; the gradient comes from autograd.
(b) `closed_form`: the derivation of the kernel file's header in NumPy, which also returns, per element of dpred, the sum of the
    absolute values of the terms that made it, and the number of terms - the per-element bound of the GPU test:

        |dev - ref| <= 2^-24 |ref| + n_terms 2^-53 abs          (one rounding to fp32 + sequential fp64 summation, (n - 1) u sum|terms|)

    abs is carried through the whole chain: the synthesis (features_check.abs_synthesis, plus |y| for the residual, so the
    cancellation of y^ against y is paid for), the division by the envelope, the per-sample factor, the window, the DFT with
    |cos|, |sin| in place of the twiddles, and the chain rule with |cos phi|, |sin phi| <= 1 (an error of a few ulp in phi turns
    the one into the other).  n_terms counts the synthesis terms of one sample (2 n_bins per frame that reaches it), the partial
    sums behind D_b, the 2 win terms of the DFT and 16 for the elementary functions (pow, sincos: a few ulp each, far below one
    term each).  Nothing here was measured on, or adjusted to, a kernel's output.

Both take the fp32 values the kernel gets.  The phase sum pred + phase_ref and the target's t1 - phase_ref are fp32 operations, as in
the kernels; alpha and inv_norm are rounded to fp32 as the C ABI passes them."""
import math

import numpy as np
import torch

import features_check as FK
from oracle import features as FO

TWO_PI = 2.0 * math.pi
K_AMP = FO.AMP_REF * (math.log(10.0) * FO.MD / 20.0)        # d amp / d a = K_AMP * 10^((100 a - 100) / 20)


def f32(v):
    return float(np.float32(v))


# the geometries of tests/features_cases.py the wave loss is held to, as (name, tight) layouts
LAYOUTS = [("rir", False), ("rir", True), ("oddwin", False), ("hop_eq_win", False), ("gaps", False), ("n512", False), ("edge", False)]
LAYOUT_IDS = [n + ("-tight" if t else "") for n, t in LAYOUTS]
ALPHA = 0.9


def inputs(name, tight):
    """Read-only fp32 inputs of one layout: pred = the "range" planes with rubbish in the padding (a phase-difference model's
    output range, wrap points planted), wav_true = the noise waveforms cut to T, phase_ref = small phases (NCHW, plane 0 unused),
    spec_target = the "feature" planes, time_weight = a 50-ms-style step (ones over the first quarter, zeros after), phase_weight =
    preprocess.sigmoid(0.5) columns; plus the geometry."""
    import features_cases as FC
    B, T0, n_fft, win, hop = FC.GEOMETRIES[name]
    nb, nf = FC.dims(name)
    H, W = FC.shape(name, tight)
    T = FC.t_out(name)
    rng = np.random.default_rng(sum(map(ord, name)) + 7000)
    x = np.linspace(-10.0, 10.0, W)
    out = {"pred": FC.planes(name, "range", tight, True), "wav_true": np.ascontiguousarray(FC.waves(name, "noise")[:, :T]),
           "phase_ref": rng.uniform(-0.5, 0.5, (B, 2, H, W)).astype(np.float32), "spec_target": FC.planes(name, "feature", tight, False),
           "time_weight": (np.arange(T) < max(T // 4, 1)).astype(np.float32),
           "phase_weight": (1.0 / (1.0 + np.exp(-(x + 5.0) * 0.5)))[::-1].astype(np.float32)}
    for v in out.values():
        v.setflags(write=False)
    out.update(B=B, H=H, W=W, T=T, des_shape=(nb, nf), n_fft=n_fft, win=win, hop=hop, inv_norm=1.0 / (2.0 * H * W * B))
    return out


def options(inp, norm, tw, ref, fused, weight=1.0):
    """keyword arguments of `loss` / `closed_form` for one combination of the switches"""
    kw = dict(norm=norm, weight=weight, time_weight=inp["time_weight"] if tw else None, phase_ref=inp["phase_ref"] if ref else None)
    if fused:
        kw.update(spec_target=inp["spec_target"], alpha=ALPHA, inv_norm=inp["inv_norm"], phase_weight=inp["phase_weight"])
    return kw


# ------------------------------------------------------------------------------------------------------------ (a) torch
def t_denormalize(a, p):
    """oracle.features.denormalize"""
    amp = (10.0 ** ((a * FO.MD - FO.MD) / 20.0) - FO.EP) * FO.AMP_REF
    phase = p * 2.0 * math.pi - math.pi
    return amp, torch.remainder(phase + math.pi, TWO_PI) - math.pi


def t_istft(S, n_fft, win, hop):
    """oracle.features.istft for S complex128 [B, n_bins, n_frames] -> [B, hop (n_frames - 1)]"""
    B, _, nf = S.shape
    w = torch.from_numpy(FO.hann_padded(n_fft, win))
    frames = torch.fft.irfft(S, n=n_fft, dim=1)
    total = n_fft + hop * (nf - 1)
    idx = (torch.arange(n_fft)[:, None] + hop * torch.arange(nf)[None, :]).reshape(-1)
    y = torch.zeros((B, total), dtype=torch.float64).index_add(1, idx, (w[None, :, None] * frames).reshape(B, -1))
    wss = torch.zeros(total, dtype=torch.float64).index_add(0, idx, (w * w)[:, None].expand(n_fft, nf).reshape(-1))
    nz = wss > FO.TINY32
    y = torch.where(nz, y / torch.where(nz, wss, torch.ones_like(wss)), y)
    return y[:, n_fft // 2: total - n_fft // 2]


class _F32Sum(torch.autograd.Function):
    """fp32(a + b) as an fp64 tensor; the rounding has slope 1, and the gradient stays fp64"""

    @staticmethod
    def forward(ctx, a, b):
        return (a.float() + b.float()).double()

    @staticmethod
    def backward(ctx, g):
        return g, None


def t_waveform(pred, des_shape, n_fft, win, hop, phase_ref=None):
    """oracle.features.feature_to_wav for a batch [B, 2, H, W] (fp64 tensor holding fp32 values)"""
    nb, nf = des_shape
    a, p = pred[:, 0, :nb, :nf], pred[:, 1, :nb, :nf]
    if phase_ref is not None:
        p = _F32Sum.apply(p, phase_ref[:, 1, :nb, :nf])
    amp, ph = t_denormalize(a, p)
    return t_istft(torch.complex(amp * torch.cos(ph), amp * torch.sin(ph)), n_fft, win, hop)


def wave_terms(pred, wav_true, des_shape, n_fft, win, hop, norm="mse", time_weight=None, phase_ref=None):
    """(y^ [B, T], E [B], D [B], sum_b E_b / D_b with the D_b == 0 rule)"""
    yh = t_waveform(pred, des_shape, n_fft, win, hop, phase_ref)
    y = wav_true.double()
    w = torch.ones(y.shape[1], dtype=torch.float64) if time_weight is None else time_weight.double()
    E = (w * (yh - y) ** 2).sum(dim=1)
    D = torch.full_like(E, float(y.shape[1])) if norm == "mse" else (w * y * y).sum(dim=1)
    ok = D != 0
    ratio = torch.where(ok, E / torch.where(ok, D, torch.ones_like(D)), torch.zeros_like(E))
    return yh, E, D, ratio.sum()


def spec_loss(pred, target, alpha, inv_norm, phase_ref=None, phase_weight=None):
    """compute_loss without the regulariser (oracle.torch_ref.data_loss) with the normalisation as one factor inv_norm"""
    alpha, inv_norm = f32(alpha), f32(inv_norm)
    t1 = target[:, 1]
    if phase_ref is not None:
        t1 = (t1.float() - phase_ref[:, 1].float()).double()
    e_amp = (target[:, 0] - pred[:, 0]) ** 2
    yt, yp = t1 * TWO_PI - math.pi, pred[:, 1] * TWO_PI - math.pi
    e_ph = 1.0 - torch.cos(torch.remainder((yt - yp) + math.pi, TWO_PI) - math.pi)
    if phase_weight is not None:
        e_ph = e_ph * phase_weight.double().view(1, 1, -1)
    return (alpha * e_amp + (1.0 - alpha) * e_ph).sum() * inv_norm


def loss(pred, wav_true, des_shape, n_fft, win, hop, norm="mse", weight=1.0, global_batch=None, time_weight=None, phase_ref=None,
         spec_target=None, alpha=0.9, inv_norm=None, phase_weight=None):
    """weight / global_batch sum_b E_b / D_b (+ the spectrogram loss with spec_target)"""
    gb = pred.shape[0] if global_batch is None else global_batch
    total = weight / gb * wave_terms(pred, wav_true, des_shape, n_fft, win, hop, norm, time_weight, phase_ref)[3]
    if spec_target is not None:
        total = total + spec_loss(pred, spec_target, alpha, inv_norm, phase_ref, phase_weight)
    return total


def autograd(pred32, wav_true, des_shape, n_fft, win, hop, **kw):
    """(loss value, d loss / d pred fp64 [B, 2, H, W]) of `loss` at the fp32 values pred32"""
    p = torch.from_numpy(np.array(pred32)).double().requires_grad_(True)
    t = lambda v: None if v is None else torch.from_numpy(np.array(v))
    for k in ("time_weight", "phase_ref", "spec_target", "phase_weight"):
        if k in kw:
            kw[k] = t(kw[k])
    if kw.get("spec_target") is not None:
        kw["spec_target"] = kw["spec_target"].double()
    val = loss(p, t(wav_true), des_shape, n_fft, win, hop, **kw)
    val.backward()
    return float(val.detach()), p.grad.detach().numpy()


# ------------------------------------------------------------------------------------------------------ (b) closed form
def n_terms(des_shape, n_fft, win, hop):
    nb, nf = des_shape
    T = hop * (nf - 1)
    return 2 * nb * (-(-win // hop) + 1) + (-(-T // 64) + 8) + 2 * win + 16


def closed_form(pred32, wav_true, des_shape, n_fft, win, hop, norm="mse", weight=1.0, global_batch=None, time_weight=None, phase_ref=None,
                spec_target=None, alpha=0.9, inv_norm=None, phase_weight=None):
    """dict: grad, abs fp64 [B, 2, H, W]; n_terms; wav fp64 [B, T]; E, D [B]; wave_out (2,); loss = weight / global_batch wave_out[0]"""
    pred = np.asarray(pred32, dtype=np.float32)
    B, _, H, W = pred.shape
    nb, nf = des_shape
    T = hop * (nf - 1)
    gb = B if global_batch is None else global_batch
    y = np.asarray(wav_true, dtype=np.float32).astype(np.float64)
    w = np.ones(T) if time_weight is None else np.asarray(time_weight, dtype=np.float32).astype(np.float64)
    a = pred[:, 0, :nb, :nf].astype(np.float64)
    p32 = pred[:, 1, :nb, :nf]
    if phase_ref is not None:
        p32 = p32 + np.asarray(phase_ref, dtype=np.float32)[:, 1, :nb, :nf]
    e10 = 10.0 ** ((a * FO.MD - FO.MD) / 20.0)
    amp, ph = FO.denormalize(a, p32.astype(np.float64))
    yh = np.stack([FO.istft(amp[b] * (np.cos(ph[b]) + 1j * np.sin(ph[b])), n_fft, win, hop) for b in range(B)])
    env = FK.envelope(nf, n_fft, win, hop)
    live = env > FO.TINY32
    r = yh - y
    E = (w * r * r).sum(axis=1)
    D = np.full(B, float(T)) if norm == "mse" else (w * y * y).sum(axis=1)
    ok = D != 0
    ratio = np.where(ok, E / np.where(ok, D, 1.0), 0.0)
    scale = np.where(ok, 2.0 * weight / (gb * np.where(ok, D, 1.0)), 0.0)
    abs_r = np.stack([FK.abs_synthesis(amp[b], n_fft, win, hop) for b in range(B)]) + np.abs(y)
    safe = np.where(live, env, 1.0)
    u = np.where(live, w * r / safe, 0.0) * scale[:, None]
    au = np.where(live, np.abs(w) * abs_r / safe, 0.0) * scale[:, None]
    hann = FO.hann_padded(n_fft, win)
    at = np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]                    # padded coordinates of s_f[n]
    seg = np.pad(u, ((0, 0), (n_fft // 2, n_fft // 2)))[:, at] * hann[None, None, :]
    aseg = np.pad(au, ((0, 0), (n_fft // 2, n_fft // 2)))[:, at] * hann[None, None, :]
    kn = (np.arange(nb)[:, None] * np.arange(n_fft)[None, :]) % n_fft
    Cm, Sm = np.cos(TWO_PI * kn / n_fft), np.sin(TWO_PI * kn / n_fft)
    re, im = np.einsum("kn,bfn->bkf", Cm, seg), -np.einsum("kn,bfn->bkf", Sm, seg)
    ab = np.einsum("kn,bfn->bkf", np.abs(Cm), aseg) + np.einsum("kn,bfn->bkf", np.abs(Sm), aseg)
    c = np.full(nb, 2.0)
    c[0] = c[-1] = 1.0
    dre, dim = c[None, :, None] / n_fft * re, c[None, :, None] / n_fft * im
    dim[:, 0, :] = dim[:, -1, :] = 0.0
    cs, sn = np.cos(ph), np.sin(ph)
    grad, abs_ = np.zeros((B, 2, H, W)), np.zeros((B, 2, H, W))
    grad[:, 0, :nb, :nf] = (dre * cs + dim * sn) * K_AMP * e10
    grad[:, 1, :nb, :nf] = TWO_PI * amp * (dim * cs - dre * sn)
    abs_[:, 0, :nb, :nf] = c[None, :, None] / n_fft * ab * K_AMP * e10
    abs_[:, 1, :nb, :nf] = TWO_PI * np.abs(amp) * c[None, :, None] / n_fft * ab
    if spec_target is not None:
        al, inv = f32(alpha), f32(inv_norm)
        tg = np.asarray(spec_target, dtype=np.float32)
        t1 = tg[:, 1]
        if phase_ref is not None:
            t1 = t1 - np.asarray(phase_ref, dtype=np.float32)[:, 1]
        t0, p0, p1 = tg[:, 0].astype(np.float64), pred[:, 0].astype(np.float64), pred[:, 1].astype(np.float64)
        wg = np.ones(W) if phase_weight is None else np.asarray(phase_weight, dtype=np.float32).astype(np.float64)
        d = ((t1.astype(np.float64) * TWO_PI - math.pi) - (p1 * TWO_PI - math.pi)) + math.pi
        phs = np.mod(d, TWO_PI) - math.pi
        grad[:, 0] += -2.0 * al * inv * (t0 - p0)
        grad[:, 1] += -(1.0 - al) * inv * TWO_PI * np.sin(phs) * wg[None, None, :]
        abs_[:, 0] += 2.0 * al * inv * (np.abs(t0) + np.abs(p0))
        abs_[:, 1] += (1.0 - al) * inv * TWO_PI * np.abs(wg)[None, None, :]
    # the sums' own allowances: y^[t] carries delta = n_syn 2^-53 abs_r[t], so w r^2 carries w (2 |r| delta + delta^2); a sum of T
    # non-negative terms, however paired, carries at most T 2^-53 of itself (+ 3 roundings inside each term)
    u53, n_syn = 2.0 ** -53, 2 * nb * (-(-win // hop) + 1)
    delta = n_syn * u53 * abs_r
    E_tol = (np.abs(w) * (2.0 * np.abs(r) * delta + delta * delta)).sum(axis=1) + (T + 3) * u53 * E
    D_tol = np.zeros(B) if norm == "mse" else (T + 3) * u53 * D
    safe_d = np.where(ok, D, 1.0)
    ratio_tol = np.where(ok, E_tol / safe_d + E * D_tol / (safe_d * safe_d) + 2.0 * u53 * ratio, 0.0)
    out_tol = np.array([ratio_tol.sum() + (B + 8) * u53 * ratio.sum(), E_tol.sum() + (B + 8) * u53 * E.sum()])
    return {"grad": grad, "abs": abs_, "n_terms": n_terms(des_shape, n_fft, win, hop), "wav": yh, "E": E, "D": D,
            "wave_out": np.array([ratio.sum(), E.sum()]), "wave_out_tol": out_tol, "loss": weight / gb * ratio.sum(), "scale": scale}


def adjoint(g, des_shape, n_fft, win, hop):
    """adj of S -> istft(S) for one cotangent g [T] (on y^): complex [n_bins, n_frames] holding (dL/dRe S, dL/dIm S), the linear part
    of closed_form on its own - for the identity <istft(S), g> = <S, adj(g)> (real inner product over Re and Im)"""
    nb, nf = des_shape
    env = FK.envelope(nf, n_fft, win, hop)
    live = env > FO.TINY32
    u = np.where(live, g / np.where(live, env, 1.0), 0.0)
    at = np.arange(nf)[:, None] * hop + np.arange(n_fft)[None, :]
    seg = np.pad(u, (n_fft // 2, n_fft // 2))[at] * FO.hann_padded(n_fft, win)[None, :]
    G = np.fft.rfft(seg, axis=1).T                                                   # [n_bins, n_frames]
    c = np.full(nb, 2.0)
    c[0] = c[-1] = 1.0
    out = c[:, None] / n_fft * G
    out[0, :] = out[0, :].real
    out[-1, :] = out[-1, :].real
    return out


def bound(ref, abs_, nt):
    """per-element allowance of the GPU test (module docstring)"""
    return 2.0 ** -24 * np.abs(ref) + nt * 2.0 ** -53 * abs_ + 2.0 ** -149
