"""The uncertainty restatement (tests/uncertainty_ref.py) against identities with known answers, the host arithmetic of
utils/uncertainty.py, and the argument errors that need no device."""
import math

import numpy as np
import pytest
import torch

import sw_blend_ref as BR
import uncertainty_ref as UR
from dycon_paper_replication_amd.networks.VNet import VNet
from dycon_paper_replication_amd.utils import uncertainty as U
from dycon_paper_replication_amd.utils.sliding_window import Blend

PATCH, VOL = (4, 4, 4), (6, 4, 4)
ENTS = [(0, 0, 0, 0), (2, 0, 0, 0), (2, 0, 0, 3)]


def _tabs():
    return BR.tables(PATCH, "gaussian", 0.25)


def test_identical_members_have_no_mutual_information_and_no_variance():
    """every entry of every member carries the same softmax at every voxel: a constant logit vector is flip-invariant"""
    logits = np.broadcast_to(np.array([0.3, -1.2, 2.0]), (len(ENTS),) + PATCH + (3,))
    out = UR.maps_from_members([logits, logits], ENTS, PATCH, VOL, _tabs())
    p = BR.softmax64(np.array([0.3, -1.2, 2.0])[:, None])[:, 0]
    np.testing.assert_allclose(out["entropy"], -(p * np.log(p)).sum(), rtol=1e-14)
    np.testing.assert_allclose(out["expected_entropy"], out["entropy"], rtol=1e-14)
    assert np.abs(out["mutual_info"]).max() <= 1e-15 and np.abs(out["variance"]).max() <= 1e-15
    assert (out["label"] == 2).all()


def test_two_opposite_one_hot_members():
    """two members, one sure of class 0 and one of class 1, constant weights: prob = (1/2, 1/2), entropy = ln 2, expected entropy 0,
    variance = sum_k (1/2 - 1/4) = 1/2; saturated logits give 0 ln 0 = 0, not nan"""
    a = np.zeros((1,) + PATCH + (2,))
    a[..., 0], a[..., 1] = 800.0, -800.0                                        # exp(-1600) == 0 in fp64: one-hot softmaxes
    out = UR.maps_from_members([a, a[..., ::-1]], [(0, 0, 0, 0)], PATCH, PATCH, BR.tables(PATCH, "constant"))
    np.testing.assert_allclose(out["prob"], 0.5, rtol=1e-15)
    np.testing.assert_allclose(out["entropy"], math.log(2), rtol=1e-15)
    assert (out["expected_entropy"] == 0).all() and not any(np.isnan(v).any() for v in out.values())
    np.testing.assert_allclose(out["mutual_info"], math.log(2), rtol=1e-15)
    np.testing.assert_allclose(out["variance"], 0.5, rtol=1e-15)
    assert (out["label"] == 0).all()                                             # the lowest index on a tie


def test_mutual_information_is_non_negative_on_random_members():
    rng = np.random.default_rng(0)
    members = [4.0 * rng.standard_normal((len(ENTS),) + PATCH + (3,)) for _ in range(3)]
    score, cnt, hsum, sq = UR.moments(members, ENTS, PATCH, VOL, _tabs())
    out = UR.finalize(score, cnt, hsum, sq)
    raw = out["entropy"] - out["expected_entropy"]                               # Jensen: H(mean) >= mean(H), before the clamp
    assert raw.min() >= -1e-14 and raw.max() > 0.1
    assert (out["mutual_info"] >= 0).all() and (out["variance"] >= 0).all() and out["variance"].max() <= 1 - 1 / 3
    assert out["entropy"].max() <= math.log(3) + 1e-14
    np.testing.assert_allclose(out["prob"].sum(0), 1.0, rtol=1e-14)


def test_ece_mce_of_a_hand_made_table():
    """bins of 10, 30 and 60 voxels with accuracy 0.5, 0.7, 0.95 and mean confidence 0.6, 0.7, 0.9; one empty bin"""
    n, correct, conf_sum = [10, 0, 30, 60], [5, 0, 21, 57], [6.0, 0.0, 21.0, 54.0]
    ece, mce = UR.ece_mce(n, correct, conf_sum)
    assert ece == pytest.approx(0.1 * 0.1 + 0.3 * 0.0 + 0.6 * 0.05, rel=1e-12) and mce == pytest.approx(0.1, rel=1e-12)
    got = U.calibration_summary(n, correct, conf_sum, 12.5, 25.0)
    assert got["ece"] == pytest.approx(0.04, rel=1e-12) and got["mce"] == pytest.approx(0.1, rel=1e-12)
    assert got["n"] == 100 and got["accuracy"] == 0.83 and got["brier"] == 0.125 and got["nll"] == 0.25
    np.testing.assert_allclose(got["reliability"], [[10, 0.5, 0.6], [0, 0, 0], [30, 0.7, 0.7], [60, 0.95, 0.9]], rtol=1e-15)
    assert "error_auroc" not in got and "aurc" not in got


def test_error_detection_curves_of_hand_made_histograms():
    # every wrong voxel is more uncertain than every correct one: perfect detection; accepting the correct ones first costs nothing
    got = U.calibration_summary([10], [6], [7.0], 1.0, 1.0, unc_hist=[[6, 0, 0], [0, 0, 4]])
    assert got["error_auroc"] == 1.0
    assert got["aurc"] == pytest.approx((0.0 + 0.0) / 2 * 0.6 + 0.0 + (0.0 + 0.4) / 2 * 0.4, rel=1e-12)
    # uncertainty says nothing: one bin
    flat = U.calibration_summary([10], [6], [7.0], 1.0, 1.0, unc_hist=[[6], [4]])
    assert flat["error_auroc"] == 0.5 and flat["aurc"] == pytest.approx(0.4, rel=1e-12)
    hist = [[10, 3, 1], [1, 2, 3]]
    assert U.calibration_summary([20], [14], [1.0], 1.0, 1.0, unc_hist=hist)["error_auroc"] == pytest.approx(UR.error_auroc(hist), rel=1e-12)
    assert math.isnan(U.calibration_summary([4], [4], [4.0], 0.0, 0.0, unc_hist=[[4, 0], [0, 0]])["error_auroc"])


def test_bin_edges():
    assert UR.bin_index(np.float32(1.0), 15) == 14 and UR.bin_index(np.float32(1.0), 16) == 15
    k = np.arange(17)
    assert UR.bin_index((k / 16).astype(np.float32), 16).tolist() == list(range(16)) + [15]
    below = np.nextafter((k[1:] / 16).astype(np.float32), np.float32(0))
    assert UR.bin_index(below, 16).tolist() == list(range(16))
    assert UR.unc_bin_index(np.float32(math.log(3)), np.float32(math.log(3)), 15) == 14
    assert UR.unc_bin_index(np.float32(0), math.log(2), 15) == 0
    prob = np.array([[0.25, 1.0, 0.5], [0.75, 0.0, 0.5]], np.float32)
    ref = UR.calibration_counts(prob, [1, 1, 0], 16)
    assert ref["n"].tolist() == [0] * 8 + [1] + [0] * 3 + [1] + [0] * 2 + [1]        # 0.5 -> 8, 0.75 -> 12, 1.0 -> 15
    assert ref["correct"].tolist() == [0] * 8 + [1] + [0] * 3 + [1] + [0] * 3       # the tie predicts class 0; (1, 0) against label 1 is wrong
    assert ref["brier_sum"] == 0.125 + 2.0 + 0.5 and ref["nll_sum"] == pytest.approx(-math.log(0.75) - math.log(1e-12) - math.log(0.5))


def test_argument_errors_without_a_device():
    prob, label = np.full((2, 3, 4), 0.5, np.float32), np.zeros((3, 4), np.int64)
    for bins in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="bins"):
            U.calibration(prob, label, bins=bins)
    with pytest.raises(ValueError, match="C in 2..8"):
        U.calibration(np.zeros((9, 4), np.float32), np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="C in 2..8"):
        U.calibration(np.zeros(4, np.float32), np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="label has shape"):
        U.calibration(prob, label[:2])
    with pytest.raises(ValueError, match="mask has shape"):
        U.calibration(prob, label, mask=np.ones((4, 3)))
    with pytest.raises(ValueError, match="uncertainty has shape"):
        U.calibration(prob, label, uncertainty=np.zeros(12, np.float32))
    with pytest.raises(ValueError, match="u_max"):
        U.calibration(prob, label, uncertainty=np.zeros((3, 4), np.float32), u_max=0.0)
    with pytest.raises(ValueError, match="u_max"):
        U.calibration(prob, label, u_max=1.0)
    image = np.zeros((16, 16, 16), np.float32)
    plain, dropping = VNet(has_dropout=False), VNet(has_dropout=True)
    with pytest.raises(ValueError, match="has_dropout"):
        U.single_case_uncertainty_device(plain, image, 8, 8, (16, 16, 16), mc_passes=2)
    with pytest.raises(ValueError, match="has_dropout"):
        U.single_case_uncertainty_device([dropping, torch.nn.Conv3d(1, 2, 1)], image, 8, 8, (16, 16, 16), mc_passes=2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="mc_passes"):
            U.single_case_uncertainty_device(dropping, image, 8, 8, (16, 16, 16), mc_passes=bad)
    for models in ([], [dropping] * 5, [dropping, "net"]):
        with pytest.raises(ValueError, match="models"):
            U.single_case_uncertainty_device(models, image, 8, 8, (16, 16, 16))
    with pytest.raises(TypeError, match="blend"):
        U.single_case_uncertainty_device(dropping, image, 8, 8, (16, 16, 16), blend="gaussian")
    with pytest.raises(RuntimeError, match="MI355X"):
        U.single_case_uncertainty_device(dropping, image, 8, 8, (16, 16, 16), blend=Blend("gaussian"))      # a model on the CPU
    with pytest.raises(ValueError, match="uncertainty is one of"):
        U.test_all_case_uncertainty(dropping, [], 2, (16, 16, 16), 8, 8, uncertainty="label")
    with pytest.raises(ValueError, match="forward_mc needs"):
        plain.forward_mc(torch.zeros(1, 1, 16, 16, 16), 0, 0)
    assert U.UncertaintyMaps._fields == UR.MAPS
