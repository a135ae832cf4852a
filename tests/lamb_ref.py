"""fp64 restatement of tfa.optimizers.LAMB._resource_apply_dense (tensorflow_addons/optimizers/lamb.py), the optimizer the legacy
trainer of the reference selects (trainer.py:37-38).  PARITY UNPINNED: tensorflow_addons is not available to this project; this file
restates the source text and tests/test_lamb_ref.py holds it to a second, independently written form.

Per variable, step t (1-based), g already multiplied by grad_scale:

    m  = b1 m + (1 - b1) g            v = b2 v + (1 - b2) g^2
    m^ = m / (1 - b1^t)               v^ = v / (1 - b2^t)
    u  = m^ / (sqrt(v^) + eps)  [+ weight_decay w   if the variable is decayed]
    r  = ||w||_2 / ||u||_2  if the variable is adapted and both norms > 0, else 1
    w  = w - lr r u

Plain torch on the CPU.  `step` works on ALL variables at once (one flat tensor, segment sums for the norms); the constants enter
as given, so a caller comparing against fp32 kernels passes the fp32-rounded constants the kernels hold."""
import torch

D = torch.float64


def corrections(beta1, beta2, t):
    """1 - beta^t, the two bias corrections."""
    return 1.0 - float(beta1) ** t, 1.0 - float(beta2) ** t


def step(variables, lr, beta1=0.9, beta2=0.999, eps=1e-6, weight_decay=0.0, corr1=None, corr2=None, grad_scale=1.0, t=None,
         one_minus=None):
    """variables: list of (w, g, m, v, (decayed, adapted)), tensors of any shape and float type.  Returns a list of dicts
    (w, m, v, u, r) in fp64 - the variables after the step, the update and the trust ratio.  Either t or corr1 / corr2.
    one_minus(b): 1 - b as the caller's arithmetic holds it (default exact)."""
    if corr1 is None:
        corr1, corr2 = corrections(beta1, beta2, t)
    om1, om2 = (1.0 - beta1, 1.0 - beta2) if one_minus is None else (one_minus(beta1), one_minus(beta2))
    sizes = [v[0].numel() for v in variables]
    cat = lambda k: torch.cat([v[k].reshape(-1).to(D) for v in variables])
    w, g, m, v = cat(0), cat(1) * grad_scale, cat(2), cat(3)
    seg = torch.repeat_interleave(torch.arange(len(variables)), torch.tensor(sizes))
    dec = torch.tensor([bool(x[4][0]) for x in variables])[seg]
    ada = torch.tensor([bool(x[4][1]) for x in variables])
    m = beta1 * m + om1 * g
    v = beta2 * v + om2 * g * g
    u = (m / corr1) / (torch.sqrt(v / corr2) + eps)
    u = torch.where(dec, u + weight_decay * w, u)
    zero = torch.zeros(len(variables), dtype=D)
    nw = torch.sqrt(zero.index_add(0, seg, w * w))
    nu = torch.sqrt(zero.index_add(0, seg, u * u))
    r = torch.where(ada & (nw > 0) & (nu > 0), nw / torch.where(nu > 0, nu, torch.ones_like(nu)), torch.ones_like(nw))
    w = w - lr * r[seg] * u
    out, o = [], 0
    for i, (x, n) in enumerate(zip(variables, sizes)):
        shp = x[0].shape
        out.append({"w": w[o:o + n].reshape(shp), "m": m[o:o + n].reshape(shp), "v": v[o:o + n].reshape(shp), "u": u[o:o + n].reshape(shp),
                    "r": float(r[i])})
        o += n
    return out
