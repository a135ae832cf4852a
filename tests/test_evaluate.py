"""Evaluation without a device: the module imports, the two scoring entry points exist and validate their arguments, the
report files have the reference's headers / labels / number formats, and the NumPy yardstick (tests/eval_ref.py) satisfies
the identities its definitions imply."""
import math
import os
import re

import numpy as np
import pytest
import torch

import eval_ref
from oracle import detrand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 10001


def test_module_constants_and_exports():
    import unet_rir_amd
    from unet_rir_amd import evaluate
    assert evaluate.ROOMS == ("HemiAnechoicRoom", "LargeMeetingRoom", "MediumMeetingRoom", "ShoeBoxRoom", "SmallMeetingRoom")
    assert evaluate.METRICS == ("mse_spec", "mse_amp", "phase", "mis_amp", "mse_wav", "mse_wav50", "mis_wav")
    assert evaluate.METRICS == eval_ref.METRICS
    assert sorted(evaluate.__all__) == sorted(["ROOMS", "METRICS", "score", "Evaluator", "write_report"])
    assert unet_rir_amd.Evaluator is evaluate.Evaluator and unet_rir_amd.score is evaluate.score
    hdr = open(os.path.join(ROOT, "include", "unetrir.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("unetrir_eval_metrics_f32", "unetrir_eval_accumulate"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in unet_rir_amd._lib.EXPORTS


def test_entry_points_validate_arguments_without_gpu():
    import unet_rir_amd
    L = unet_rir_amd._lib.lib()
    m = L.unetrir_eval_metrics_f32
    p = 4096                                     # any non-null value: refused calls never dereference it
    assert m(None, p, None, 1, 8, 8, None, None, 0, 2400, p, None) == EINVAL          # pred
    assert m(p, None, None, 1, 8, 8, None, None, 0, 2400, p, None) == EINVAL          # target
    assert m(p, p, None, 1, 8, 8, None, None, 0, 2400, None, None) == EINVAL          # out
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, -8, 8), (1, 8, -8)):
        assert m(p, p, None, B, H, W, None, None, 0, 2400, p, None) == EINVAL, (B, H, W)
    assert m(p, p, None, 1, 8, 8, p, None, 16, 2400, p, None) == EINVAL               # half a waveform pair
    assert m(p, p, None, 1, 8, 8, None, p, 16, 2400, p, None) == EINVAL
    assert m(p, p, None, 1, 8, 8, p, p, 0, 2400, p, None) == EINVAL                   # waveforms of no length
    assert m(p, p, None, 1, 8, 8, p, p, -4, 2400, p, None) == EINVAL
    a = L.unetrir_eval_accumulate
    assert a(None, p, 1, 5, p, None) == EINVAL
    assert a(p, None, 1, 5, p, None) == EINVAL
    assert a(p, p, 1, 5, None, None) == EINVAL
    assert a(p, p, 0, 5, p, None) == EINVAL
    assert a(p, p, 1, 0, p, None) == EINVAL                                           # G = 0
    assert a(p, p, 1, -1, p, None) == EINVAL


def _result():
    nan = float("nan")
    return {
        "rooms": ["HemiAnechoicRoom", "LargeMeetingRoom", "MediumMeetingRoom", "ShoeBoxRoom", "SmallMeetingRoom"],
        "n": [7, 2, 3, 0, 1, 1],
        "mse_spec": [0.012345678, 0.5, 0.25, nan, 0.125, 1.0],
        "mse_amp": [0.00012345, 0.1, 0.2, nan, 0.3, 0.4],
        "phase": [0.98765432, 1.0, 0.75, nan, 0.5, 0.25],
        "mis_amp": [-3.0102999, -1.5, 2.25, nan, -10.0, 0.5],
        "mse_wav": [1.2345678e-7, 1e-4, 2.5e-5, nan, 3e-6, 1.5e-3],
        "mse_wav50": [9.87654321e-6, 1e-4, 2.5e-5, nan, 3e-6, 1.5e-3],
        "mis_wav": [12.3456789, 1.0, 2.0, nan, 3.0, 4.0],
        "timing": {"n_batches": 4, "batch_size": 2, "inference_s": 0.0123456789, "postprocess_s": 0.000123456, "loss_s": 2.6e-5,
                   "total_s": 1.5},
    }


def test_write_report_files_and_formats(tmp_path):
    from unet_rir_amd.evaluate import write_report
    write_report(_result(), str(tmp_path / "rep"), "unet_x")
    folder = tmp_path / "rep"
    assert sorted(p.name for p in folder.iterdir()) == ["unet_x_infer_time.csv", "unet_x_losses.csv", "unet_x_results_inference.txt"]
    losses = (folder / "unet_x_losses.csv").read_text().split("\n")
    assert losses[0] == ("room,n samples,MSE spectrogram,MSE magnitude,1-cos(y-y_) phase,MSE waveform,MSE waveform 50ms,"
                         "Misalignment magnitude,Misalignment waveform")
    assert losses[1] == "Global,7,0.0123,0.0001,0.9877,1.2346e-07,9.8765e-06,-3.0103e+00,1.2346e+01"
    assert losses[2] == "HemiAnechoic,2,0.5,0.1,1.,1.e-04,1.e-04,-1.5e+00,1.e+00"
    assert losses[4] == "Medium,0,nan,nan,nan,nan,nan,nan,nan"                        # an empty room
    assert [r.split(",")[0] for r in losses[1:7]] == ["Global", "HemiAnechoic", "Large", "Medium", "Shoe", "Small"]
    assert losses[7:] == [""]
    times = (folder / "unet_x_infer_time.csv").read_text().split("\n")
    assert times[0] == "n_samples,t_model_inference_avg,batch_size,t_postprocess,t_loss_calc,t_global"
    assert times[1] == "7,0.01235,2,0.00012,0.00003,1.5"
    text = (folder / "unet_x_results_inference.txt").read_text()
    assert text.startswith("unet_x results:\n\nTook 0.01235 s on average to infer spectrograms with batch size of 2\n")
    assert "Total loss: 0.0123 (MSE whole spectrogram)\t|\tAmplitude loss: 0.0001 (MSE amplitude)\t|\tPhase loss: 0.9877 " \
           "(1-cos(y_true - y_pred))\n" in text
    assert "Waveform loss: 1.2346e-07 (MSE)\t|\t 50 ms waveform loss: 9.8765e-06 (MSE)\n" in text
    assert "Misalignment loss (amplitude): -3.0103e+00 (dB)\t|\t Misalignment loss (wav): 1.2346e+01 (dB)\n" in text
    assert "MediumMeetingRoom losses (0 samples):\nTotal loss: nan (MSE whole spectrogram)" in text
    assert "for 7 samples\n" in text


def test_score_refuses_cpu_tensors():
    from unet_rir_amd.evaluate import Evaluator, score
    x = torch.zeros((1, 2, 8, 8))
    with pytest.raises(ValueError):
        score(x, x)
    with pytest.raises(ValueError):
        score(x, x, wav_pred=torch.zeros((1, 16)), wav_true=torch.zeros((1, 16)))
    with pytest.raises(ValueError):
        Evaluator(None).update_scored(x, x, x, None, None, ["ShoeBoxRoom"])


# ---- the yardstick on its own ----------------------------------------------------------------------

def _sample(name, H=12, W=10, T=3000):
    target = detrand.uniform(name + "/t", (H, W, 2))
    pred = detrand.uniform(name + "/p", (H, W, 2))
    wt = detrand.uniform(name + "/wt", (T,), -1e-2, 1e-2)
    wp = detrand.uniform(name + "/wp", (T,), -1e-2, 1e-2)
    return pred, target, wp, wt


def test_yardstick_identical_prediction_scores_zero():
    _, target, _, wt = _sample("ident")
    m = eval_ref.sample_metrics(target, target, wt, wt)
    assert m[0] == 0 and m[1] == 0 and m[2] == 0 and m[4] == 0 and m[5] == 0
    assert m[3] == -np.inf and m[6] == -np.inf            # documented: IEEE where the reference raises


@pytest.mark.parametrize("a", [1.0, 0.5, 0.125, 0.03125])
def test_yardstick_misalignment_of_a_scaled_magnitude(a):
    """pred0 = (1 + a) target0 -> |pred0 - target0| / |target0| = a.  a and the magnitudes are chosen so that (1 + a) t is
    exact in fp32 (t has 24 random bits below 1; a is a power of two; t is cut to 16 bits here)."""
    _, target, _, _ = _sample("scaled")
    target = target.copy()
    target[..., 0] = np.floor(target[..., 0] * 65536) / 65536
    pred = target.copy()
    pred[..., 0] = (1 + a) * target[..., 0]
    assert np.array_equal(pred[..., 0].astype(np.float64), (1 + a) * target[..., 0].astype(np.float64))
    m = eval_ref.sample_metrics(pred, target)
    assert abs(m[3] - 20 * math.log10(a)) <= 1e-9
    assert np.isnan(m[4]) and np.isnan(m[5]) and np.isnan(m[6])


def test_yardstick_phase_is_periodic():
    pred, target, _, _ = _sample("period")
    pred = pred.copy()
    pred[..., 1] = np.floor(pred[..., 1] * 4096) / 4096       # exact after adding small integers in fp32
    base = eval_ref.sample_metrics(pred, target)[2]
    assert 0.5 < base < 1.5
    for k in (1, -1, 3):
        shifted = pred.copy()
        shifted[..., 1] += k
        assert abs(eval_ref.sample_metrics(shifted, target)[2] - base) <= 1e-12


def test_yardstick_first_50ms_window():
    pred, target, wp, wt = _sample("w50")
    wp = wt.copy()
    wp[2400:] += 1e-3
    m = eval_ref.sample_metrics(pred, target, wp, wt)
    assert m[5] == 0 and m[4] > 0
    assert abs(m[4] - 600 * 1e-6 / 3000) <= 1e-6 * m[4]        # fp32 rounding of the shifted samples


def test_yardstick_diff_gen_uses_the_sum_for_phase_only():
    pred, target, _, _ = _sample("diff")
    spec_in = detrand.uniform("diff/in", pred.shape)
    summed = pred.copy()
    summed[..., 1] = pred[..., 1] + spec_in[..., 1]
    a = eval_ref.sample_metrics(pred, target, spec_in=spec_in)
    b = eval_ref.sample_metrics(summed, target)
    c = eval_ref.sample_metrics(pred, target)
    assert a[2] == b[2] and a[2] != c[2]                     # phase from the sum
    assert a[0] == c[0] and a[0] != b[0]                     # mse_spec from the raw prediction
    assert a[1] == c[1] and a[3] == c[3]


def test_yardstick_group_means_of_a_hand_made_table():
    rows = np.zeros((5, 7))
    rows[:, 0] = [1, 2, 3, 4, 10]
    rows[:, 3] = [-10, -20, -30, -40, -100]
    means, counts = eval_ref.group_means(rows, [0, 2, 0, 7, 2], 3)
    assert counts.tolist() == [5, 2, 0, 2]
    assert means[0, 0] == 4 and means[1, 0] == 2 and means[3, 0] == 6          # the stray sample (7) only in the global row
    assert means[0, 3] == -40 and means[1, 3] == -20 and means[3, 3] == -60     # dB figures are averaged as dB
    assert np.isnan(means[2]).all()                                            # np.mean([]) of an empty room


def test_gpu_test_inputs_are_nowhere_degenerate():
    """The inputs of tests/test_evaluate_gpu.py give 7 x B finite reference values: no comparison there is ever vacuous."""
    import test_evaluate_gpu as G
    for H, W, T, n50 in ((144, 160, 9600, 2400), (9, 7, 101, 300)):
        d = G.make_inputs("score", 5, H, W, T)
        for ref in (None, d["spec_in"]):
            want = eval_ref.batch_metrics(d["pred"], d["target"], d["wav_pred"], d["wav_true"], ref, n50)
            assert want.shape == (5, 7) and np.isfinite(want).all()
