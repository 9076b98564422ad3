"""Host side of the lesion statistics and the ISLES22 protocol (utils/lesions.py, utils/isles_eval.py): the scipy reference
(tests/lesion_ref.py) on hand-made cases whose counts are written down here, `metrics_from_counts` with every empty branch, argument
validation and the C-ABI declarations.  No GPU.  `isles_case_metrics` counts its voxels on the device, so its four branches are held
to the restated script in tests/test_lesions_gpu.py; here the restated script's own empty-mask branches are pinned to the values of
code/test_ISLES22.py:98-121."""
import os
import re

import numpy as np
import pytest
import torch

import lesion_ref as LR
from conftest import ROOT

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import isles_eval as IE
from dycon_paper_replication_amd.utils import lesions as LS

# (case, connectivity, min_voxels) -> n_gt, n_pred, tp, fn, fp, vox_gt, vox_pred, vox_and
EXPECTED = {
    ("checker_opposite", 1, 1): (105, 105, 0, 105, 105, 105, 105, 0),
    ("checker_opposite", 2, 1): (1, 1, 0, 1, 1, 105, 105, 0),
    ("checker_opposite", 3, 1): (1, 1, 0, 1, 1, 105, 105, 0),
    ("checker_same", 1, 1): (105, 105, 105, 0, 0, 105, 105, 105),
    ("cubes", 3, 1): (2, 2, 2, 0, 0, 28, 28, 2),
    ("cubes", 3, 2): (1, 1, 0, 1, 1, 27, 27, 0),            # the filter turns a hit into a miss
    ("touching", 1, 1): (1, 1, 0, 1, 1, 1, 1, 0),           # touching is not overlap
    ("touching", 3, 1): (1, 1, 0, 1, 1, 1, 1, 0),
}


def test_count_fields():
    assert LS.COUNT_FIELDS == LR.FIELDS == ("n_gt", "n_pred", "tp", "fn", "fp", "vox_gt", "vox_pred", "vox_and")


@pytest.mark.parametrize("key", sorted(EXPECTED), ids=lambda k: "-".join(map(str, k)))
def test_reference_reproduces_the_hand_made_counts(key):
    name, connectivity, min_voxels = key
    pred, gt = LR.HAND[name]
    assert tuple(LR.counts(pred, gt, connectivity, min_voxels)) == EXPECTED[key]


def test_reference_tables():
    pred, gt = LR.HAND["cubes"]
    assert LR.table(pred, gt, "gt").tolist() == [[1, 27, 1], [2, 1, 1]]
    assert LR.table(pred, gt, "pred").tolist() == [[1, 1, 1], [2, 27, 1]]
    assert LR.table(pred, gt, "gt", min_voxels=2).tolist() == [[1, 27, 0]]
    assert LR.table(pred, gt, "pred", min_voxels=28).shape == (0, 3)
    t = LR.table(*LR.HAND["checker_same"], "gt", connectivity=1)
    assert t.shape == (105, 3) and (t[:, 0] == np.arange(1, 106)).all() and (t[:, 1:] == 1).all()


@pytest.mark.parametrize("key", sorted(EXPECTED), ids=lambda k: "-".join(map(str, k)))
@pytest.mark.parametrize("empty_value", [1.0, 0.0, float("nan")])
def test_metrics_from_counts_on_the_hand_made_cases(key, empty_value):
    row = np.array(EXPECTED[key], np.int64)
    got = LS.metrics_from_counts(row, voxel_volume=2.5, empty_value=empty_value)
    ref = LR.metrics(row, 2.5, empty_value)
    assert set(got) == set(ref) == {"lesion_f1", "lesion_recall", "lesion_precision", "lesion_count_diff", "abs_volume_diff", "dice"}
    for name in ref:
        assert got[name].dtype == np.float64 and got[name].shape == ()
        np.testing.assert_allclose(got[name], ref[name], rtol=1e-12, atol=0, equal_nan=True)


def test_metrics_from_counts_values_and_empty_branches():
    n = {k: i for i, k in enumerate(LS.COUNT_FIELDS)}
    rows = np.zeros((5, 8), np.int64)
    rows[1, [n["n_pred"], n["fp"], n["vox_pred"]]] = (2, 2, 9)               # no ground truth: recall and nothing else is empty
    rows[2, [n["n_gt"], n["fn"], n["vox_gt"]]] = (3, 3, 7)                    # no prediction: precision is empty
    rows[3] = (4, 3, 2, 2, 1, 40, 30, 14)
    rows[4] = EXPECTED[("cubes", 3, 1)]
    for empty in (1.0, 0.25):
        m = LS.metrics_from_counts(rows, voxel_volume=0.5, empty_value=empty)
        np.testing.assert_array_equal(m["lesion_f1"], [empty, 0.0, 0.0, 2 / 3.5, 1.0])
        np.testing.assert_array_equal(m["lesion_recall"], [empty, empty, 0.0, 0.5, 1.0])
        np.testing.assert_array_equal(m["lesion_precision"], [empty, 0.0, empty, 2 / 3, 1.0])
        np.testing.assert_array_equal(m["lesion_count_diff"], [0, 2, 3, 1, 0])
        np.testing.assert_array_equal(m["abs_volume_diff"], [0.0, 4.5, 3.5, 5.0, 0.0])
        np.testing.assert_array_equal(m["dice"], [empty, 0.0, 0.0, 28 / 70, 4 / 56])
        for k, row in enumerate(rows):
            ref = LR.metrics(row, 0.5, empty)
            for name in ref:
                np.testing.assert_allclose(m[name][k], ref[name], rtol=1e-12, atol=0)
    one = LS.metrics_from_counts(rows[3])
    assert all(v.shape == () and v.dtype == np.float64 for v in one.values()) and one["abs_volume_diff"] == 10.0
    with pytest.raises(ValueError, match="8 columns"):
        LS.metrics_from_counts(np.zeros((2, 7), np.int64))


def test_restated_script_empty_branches():
    """code/test_ISLES22.py:98-121: the three branches that need no surface distance"""
    shape = (16, 12, 9)
    zero, one = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    one[3, 4, 5] = 1
    far = float(np.linalg.norm(shape))
    assert LR.isles_case(zero, zero) == dict(dice=1.0, hd95=0.0, asd=0.0, sensitivity=1.0, specificity=1.0)
    assert LR.isles_case(one, zero) == dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=0.0)
    assert LR.isles_case(zero, one) == dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=1.0)
    got = LR.isles_case(one, one, percase=lambda p, g: (1.0, 1.0, 0.0, 0.0))
    n = float(np.prod(shape))
    assert got["sensitivity"] == 1 / (1 + 1e-10) and got["specificity"] == (n - 1) / (n - 1 + 1e-10)
    assert IE.CASE_FIELDS == tuple(got)


def test_argument_validation():
    """everything here is refused before the device is touched"""
    ok = np.zeros((4, 5, 6), np.uint8)
    for f in (LS.lesion_counts, LS.lesion_metrics, LS.lesion_table):
        for bad in (0, -1, 1.5, True, "2", None):
            with pytest.raises(ValueError, match="min_voxels"):
                f(ok, ok, min_voxels=bad)
        for bad in (0, 4, 1.5):
            with pytest.raises(ValueError, match="connectivity"):
                f(ok, ok, connectivity=bad)
        with pytest.raises(ValueError, match=r"\(X, Y, Z\) or \(n_vol, X, Y, Z\)"):
            f(np.zeros((4, 4), np.uint8), ok)
        with pytest.raises(ValueError, match="CUDA tensor"):
            f(torch.zeros((4, 5, 6), dtype=torch.uint8), ok)
    with pytest.raises(ValueError, match='"gt" or "pred"'):
        LS.lesion_table(ok, ok, of="both")
    with pytest.raises(ValueError, match="voxelspacing"):
        LS.lesion_metrics(ok, ok, voxelspacing=(1.0, 2.0))
    with pytest.raises(ValueError, match=r"\(H, W, D\)"):
        IE.isles_case_metrics(np.zeros((2, 4, 5, 6), np.uint8), np.zeros((2, 4, 5, 6), np.uint8))
    with pytest.raises(ValueError, match=r"\(H, W, D\)"):
        IE.isles_case_metrics(np.zeros((4, 5, 7), np.uint8), ok)


def test_header_declares_the_lesion_functions():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    for name in ("dycon_lesion_workspace", "dycon_lesion_counts"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.dycon_lesion_workspace(1, 4, 5, 6) == 4 * 512               # four sections of 120 int32, each padded to 256 bytes
    assert lib.dycon_lesion_workspace(3, 17, 13, 70) == 4 * ((3 * 17 * 13 * 70 * 4 + 255) // 256 * 256)
    assert lib.dycon_lesion_workspace(1, 4, 5, 513) == 0                   # the limits of dycon_cc_roots
    assert lib.dycon_lesion_workspace(0, 4, 5, 6) == 0
