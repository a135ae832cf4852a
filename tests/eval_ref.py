"""The yardstick of the evaluation tests: a NumPy fp64 restatement of the scoring arithmetic of the reference's evaluation
script, rir_generation.py:173-225 (the seven figures of one sample) and :311-357 (their means, globally and per room).

Each line cites the reference line it restates.  Inputs are the fp32 arrays the device scores; every difference, square,
cosine and sum is taken in fp64 (the reference works in fp32 through TensorFlow; the device kernels accumulate in fp64 from
the same fp32 values, so this is the exact form of what both compute).  The one fp32 operation is the `diff_gen` phase sum
(:174): the reference adds two fp32 tensors, and that fp32 plane is also what its reconstruction receives.

Parity with TensorFlow is UNPINNED, like the rest of the oracle: the script needs TensorFlow and the dataset, and does not
parse as committed (rir_generation.py:63).  `tests/test_evaluate.py` checks this file on its own by identities.

Degenerate samples: where the reference raises (`math.log10(0)`) or divides by zero, IEEE values are returned (-inf, +inf,
NaN), which is the documented rule of the device kernels.
"""
import math

import numpy as np

METRICS = ("mse_spec", "mse_amp", "phase", "mis_amp", "mse_wav", "mse_wav50", "mis_wav")


def _mse(y_true, y_pred):
    """amplitude_loss (:31-34) followed by np.mean (:195, :197, :215, :218): the mean of the squared difference."""
    d = np.asarray(y_true, dtype=np.float64) - np.asarray(y_pred, dtype=np.float64)
    return float(np.mean(d * d))


def _phase(y_true, y_pred):
    """phase_loss (:36-40)."""
    y_true = np.asarray(y_true, dtype=np.float64) * 2 * math.pi - math.pi            # :37
    y_pred = np.asarray(y_pred, dtype=np.float64) * 2 * math.pi - math.pi            # :38
    return float(np.mean(1 - np.cos(y_true - y_pred)))                               # :39


def _misalignment(pred, true):
    """20 log10(|pred - true|_2 / |true|_2) (:203-205, :221-223), arrays flattened."""
    num = np.linalg.norm(np.asarray(pred, dtype=np.float64).ravel() - np.asarray(true, dtype=np.float64).ravel())
    den = np.linalg.norm(np.asarray(true, dtype=np.float64).ravel())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(20 * np.log10(np.float64(num) / np.float64(den)))


def scored_phase(pred, spec_in=None):
    """The phase plane that is scored and reconstructed, [H, W] fp32 from NHWC [H, W, 2] samples: the prediction's, or under
    diff_gen (:174, :191) prediction + input phase, added in fp32 as the reference adds them."""
    p = np.asarray(pred, dtype=np.float32)[..., 1]
    if spec_in is None:
        return p                                                                      # :193
    return (p + np.asarray(spec_in, dtype=np.float32)[..., 1]).astype(np.float32)     # :174


def sample_metrics(pred, target, wav_pred=None, wav_true=None, spec_in=None, n50=2400):
    """One sample, NHWC [H, W, 2] fp32 (`spec_in` given = diff_gen) -> the seven figures in the order of METRICS."""
    pred = np.asarray(pred, dtype=np.float32)
    target = np.asarray(target, dtype=np.float32)
    stft_true, phase_true = target[..., 0], target[..., 1]                            # :185-186
    stft_pred = pred[..., 0]                                                          # :188
    phase_pred = scored_phase(pred, spec_in)                                          # :190-193
    out = np.full(7, np.nan)
    out[1] = _mse(stft_true, stft_pred)                                               # :195
    out[2] = _phase(phase_true, phase_pred)                                           # :196
    out[0] = _mse(target, pred)                                                       # :197, the raw prediction also under diff_gen
    out[3] = _misalignment(stft_pred, stft_true)                                      # :203-205
    if wav_pred is not None:
        wav_pred = np.asarray(wav_pred, dtype=np.float32)
        wav_true = np.asarray(wav_true, dtype=np.float32)
        out[4] = _mse(wav_true, wav_pred)                                             # :215
        out[5] = _mse(wav_true[:n50], wav_pred[:n50])                                 # :218 (n50 = 2400 there)
        out[6] = _misalignment(wav_pred, wav_true)                                    # :221-223
    return out


def batch_metrics(pred, target, wav_pred=None, wav_true=None, spec_in=None, n50=2400):
    """NHWC [B, H, W, 2] batches -> fp64 [B, 7] (the loop :170-225)."""
    B = len(pred)
    return np.stack([sample_metrics(pred[j], target[j], None if wav_pred is None else wav_pred[j],
                                    None if wav_true is None else wav_true[j], None if spec_in is None else spec_in[j], n50)
                     for j in range(B)])


def group_means(rows, group, n_groups):
    """rows [N, 7], group [N] ints -> (means [n_groups + 1, 7], counts [n_groups + 1]): row 0 over every sample (:311-317), row
    1 + g over the samples of room g (:227-290, :319-357).  A sample whose group is outside 0..n_groups-1 matches none of the
    `if characteristic_out[0] == ...` tests and is in the global row only; an empty room is np.mean([]) = NaN."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    group = np.asarray(group)
    means = np.full((n_groups + 1, 7), np.nan)
    counts = np.zeros(n_groups + 1, dtype=np.int64)
    sel = [np.ones(len(rows), dtype=bool)] + [group == g for g in range(n_groups)]
    for i, s in enumerate(sel):
        counts[i] = int(s.sum())
        if counts[i]:
            means[i] = rows[s].mean(axis=0)
    return means, counts
