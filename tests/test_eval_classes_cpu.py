"""CPU: the contract around the multi-class evaluation (utils/eval_classes.py, csrc/evalc.hip): the C ABI surface, the host arithmetic
(metrics_from_confusion, the chunk boxes, the ISLES pad rule), the argument guards, and the fixture tests/golden/make_golden_eval_classes.py
wrote.  `dice_case` / `binary_batch` rebuild the fixture's inputs from seeds, for the generator and for tests/test_eval_classes_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils.test_3d_patch import _windows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("dycon_sw_accumulate_all", "dycon_sw_finalize_argmax", "dycon_argmax_labels", "dycon_class_confusion",
                    "dycon_batch_class_confusion")
DICE_CASES = ("bool_arrays", "float_tensors", "multi_valued", "empty_masks")
DICE_SHAPE = (9, 8, 7)
BATCH_SHAPE = (3, 6, 5, 4)


def dice_case(name):
    """(input, target, ignore_index) of one recorded call of the reference's metrics.dice"""
    rng = np.random.default_rng(11 + DICE_CASES.index(name))
    if name == "bool_arrays":
        return rng.random(DICE_SHAPE) > 0.5, rng.random(DICE_SHAPE) > 0.6, 1
    if name == "float_tensors":
        return (torch.from_numpy(rng.random(DICE_SHAPE).astype(np.float32)),
                torch.from_numpy((rng.random(DICE_SHAPE) > 0.5).astype(np.float32)), 0)
    if name == "multi_valued":
        return rng.random(DICE_SHAPE).astype(np.float32), rng.integers(0, 4, DICE_SHAPE).astype(np.float32), 2
    return np.zeros(DICE_SHAPE, bool), np.zeros(DICE_SHAPE, bool), 0


def binary_batch():
    """binary (B, D, H, W) float32 output / label of the recorded compute_dice / compute_jaccard; the last sample is empty on both sides"""
    rng = np.random.default_rng(17)
    out, lab = (rng.random(BATCH_SHAPE) > 0.5).astype(np.float32), (rng.random(BATCH_SHAPE) > 0.4).astype(np.float32)
    out[-1] = lab[-1] = 0
    return out, lab


def test_new_entry_points_declared_exported_bound_and_defined():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    declared = set(re.findall(r"\b(dycon_[a-z0-9_]+)\s*\(", hdr))
    csrc = os.path.join(ROOT, "dycon_paper_replication_amd", "csrc")
    assert re.search(r"global:\s*dycon_\*;", open(os.path.join(csrc, "exports.map")).read())
    src = open(os.path.join(csrc, "evalc.hip")).read()
    assert re.search(r"^SRCS\s*=.*\bevalc\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
        assert re.search(r'extern "C" int ' + name + r"\(", src), name
        assert hasattr(raw, name) and getattr(lib, name).argtypes is not None, name


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """the guards run on the host: no device is needed to be refused"""
    lib = _lib.load()
    int3 = ctypes.c_int * 3
    one = ctypes.c_void_p(64)                       # never dereferenced: every call below is refused first
    acc = lambda C, nb, lo, hi: lib.dycon_sw_accumulate_all(one, C, nb, 8, 6, 5, one, one, one, 13, 9, 7, int3(*lo), int3(*hi), None)  # noqa: E731
    assert acc(1, 4, (0, 0, 0), (13, 9, 7)) != 0 and b"2..8" in lib.dycon_last_error()
    assert acc(9, 4, (0, 0, 0), (13, 9, 7)) != 0
    assert acc(3, 65, (0, 0, 0), (13, 9, 7)) != 0 and b"65 patches" in lib.dycon_last_error()
    for lo, hi in (((0, 0, 0), (14, 9, 7)), ((-1, 0, 0), (13, 9, 7)), ((0, 0, 7), (13, 9, 7)), ((0, 5, 0), (13, 4, 7))):
        assert acc(3, 4, lo, hi) != 0 and b"outside the volume" in lib.dycon_last_error(), (lo, hi)
    assert lib.dycon_sw_finalize_argmax(one, one, 9, 10, one, None, None) != 0
    assert lib.dycon_argmax_labels(one, 1, 10, one, None) != 0
    assert lib.dycon_class_confusion(one, one, 4, 10, 3, one, None) != 0 and b"uint8 or int64" in lib.dycon_last_error()
    assert lib.dycon_class_confusion(one, one, 1, 10, 9, one, None) != 0
    assert lib.dycon_batch_class_confusion(one, one, 8, 2, 10, 1, one, None) != 0


def test_fixture_is_finite_and_small():
    path = os.path.join(ROOT, "tests", "golden", "eval_classes.npz")
    assert os.path.getsize(path) < 100 * 1024
    g = load_golden("eval_classes")
    assert list(g["dice.cases"]) == list(DICE_CASES)
    for i, name in enumerate(DICE_CASES):
        assert int(g["dice.ignore_index"][i]) == dice_case(name)[2]
    for k in g.files:
        if g[k].dtype.kind == "f":
            assert np.isfinite(g[k]).all(), k
    assert g["dice.plain"].shape == g["dice.ignored"].shape == (len(DICE_CASES),)
    assert g["dice.plain"][DICE_CASES.index("empty_masks")] == 1.0            # (0 + 1) / (0 + 0 + 1)
    assert g["batch.dice"].shape == g["batch.jaccard"].shape == (BATCH_SHAPE[0],)
    assert g["batch.dice"][-1] == 0.0 and g["batch.jaccard"][-1] == 0.0       # 0 / 1e-8
    # the recorded numbers are the formulas of code/utils/metrics.py:39-109 on the rebuilt inputs
    inp, tgt, k = dice_case("multi_valued")
    keep = tgt != k
    np.testing.assert_allclose(g["dice.plain"][2], (2 * (inp * tgt).sum(dtype=np.float64) + 1) / (inp.sum(dtype=np.float64) + tgt.sum(dtype=np.float64) + 1),
                               rtol=1e-6)
    np.testing.assert_allclose(g["dice.ignored"][2], (2 * (inp * tgt)[keep].sum(dtype=np.float64) + 1)
                               / (inp[keep].sum(dtype=np.float64) + tgt[keep].sum(dtype=np.float64) + 1), rtol=1e-6)
    out, lab = binary_batch()
    inter = (out * lab).sum((1, 2, 3), dtype=np.float64)
    np.testing.assert_allclose(g["batch.dice"], 2 * inter / (out.sum((1, 2, 3)) + lab.sum((1, 2, 3)) + 1e-8), rtol=1e-6)
    np.testing.assert_allclose(g["batch.jaccard"], inter / (out.sum((1, 2, 3)) + lab.sum((1, 2, 3)) - inter + 1e-8), rtol=1e-6)


def test_metrics_from_confusion_known_answers():
    # identical maps: the matrix is diagonal, every class scores (1, 1)
    np.testing.assert_array_equal(EC.metrics_from_confusion(np.diag([50, 7, 3])), [[1.0, 1.0], [1.0, 1.0]])
    # a known 3-class answer, rows = prediction, columns = ground truth
    conf = np.array([[80, 2, 1],
                     [3, 10, 2],
                     [0, 4, 6]])
    got = EC.metrics_from_confusion(conf)
    # class 1: |P| = 15, |G| = 16, I = 10;  class 2: |P| = 10, |G| = 9, I = 6
    np.testing.assert_allclose(got, [[20 / 31, 10 / 21], [12 / 19, 6 / 13]], rtol=1e-15)
    assert EC.metrics_from_confusion(torch.from_numpy(conf)).shape == (2, 2)
    # class 2 missing from the prediction, then from the ground truth: Dice = Jaccard = 0 for it, class 1 unaffected
    no_pred = EC.metrics_from_confusion(np.array([[80, 0, 5], [0, 10, 2], [0, 0, 0]]))
    np.testing.assert_allclose(no_pred, [[20 / 22, 10 / 12], [0.0, 0.0]], rtol=1e-15)
    no_gt = EC.metrics_from_confusion(np.array([[80, 0, 0], [0, 10, 0], [5, 2, 0]]))
    np.testing.assert_allclose(no_gt, [[20 / 22, 10 / 12], [0.0, 0.0]], rtol=1e-15)
    with pytest.raises(ZeroDivisionError):                   # absent on both sides: medpy's jc divides by the empty union
        EC.metrics_from_confusion(np.diag([50, 7, 0]))
    with pytest.raises(ValueError):
        EC.metrics_from_confusion(np.zeros((2, 3)))


def test_chunk_boxes():
    patch = (32, 32, 16)
    wins = _windows((40, 36, 24), patch, 8, 4)
    assert len(wins) == 12 and wins[:3] == [(0, 0, 0), (0, 0, 4), (0, 0, 8)]      # 2 x 2 x 3, z fastest
    # windows of one z-run: the box is one window wide in x and y and spans the run in z
    assert EC.chunk_box(wins[0:3], patch) == ((0, 0, 0), (32, 32, 24))
    assert EC.chunk_box(wins[1:3], patch) == ((0, 0, 4), (32, 32, 24))
    # batch_size 5: the first chunk holds the z-run of y = 0 and two windows of y = 4; the second straddles two x rows
    assert EC.chunk_box(wins[0:5], patch) == ((0, 0, 0), (32, 36, 24))
    assert wins[5:10] == [(0, 4, 8), (8, 0, 0), (8, 0, 4), (8, 0, 8), (8, 4, 0)]
    assert EC.chunk_box(wins[5:10], patch) == ((0, 0, 0), (40, 36, 24))
    assert EC.chunk_box(wins[10:12], patch) == ((8, 4, 4), (40, 36, 24))
    for i in range(0, 12, 5):                                                     # every box lies inside the volume
        lo, hi = EC.chunk_box(wins[i:i + 5], patch)
        assert all(0 <= a < b <= s for a, b, s in zip(lo, hi, (40, 36, 24)))


def test_isles_pad_rule():
    patch = (32, 32, 16)
    assert EC.isles_pad((32, 32, 16), patch) == (0, 0, 0)              # equal to the patch: no padding
    assert EC.isles_pad((48, 40, 32), patch) == (0, 0, 0)              # larger on every axis
    assert EC.isles_pad((24, 20, 10), patch) == (5, 7, 4)              # smaller: (p - s) // 2 + 1 per side
    # one short axis pads every axis, the `// 2 + 1` quirk of :358-360: an axis of exactly one patch grows by 2, a longer one stays
    assert EC.isles_pad((32, 32, 10), patch) == (1, 1, 4)
    assert EC.isles_pad((48, 31, 16), patch) == (0, 1, 1)
    assert EC.isles_pad((33, 34, 15), patch) == (0, 0, 1)              # (32 - 33) // 2 + 1 = 0, (32 - 34) // 2 + 1 = 0


def test_evaluator_needs_the_gpu_and_more_than_one_class():
    image = np.zeros((32, 32, 16), np.float32)
    with pytest.raises(RuntimeError, match="MI355X only"):
        EC.test_single_case_classes(net_factory_3d("vnet", 1, 3, 2), image, 8, 4, (32, 32, 16))
    with pytest.raises(RuntimeError, match="MI355X only"):
        EC.isles_val_dice(net_factory_3d("vnet", 1, 3, 2), image, image, (32, 32, 16))
    with pytest.raises(ValueError, match="at least 2 classes"):
        EC.test_single_case_classes(net_factory_3d("vnet", 1, 1, 2), image, 8, 4, (32, 32, 16), device="cuda")


def test_class_metrics_refuse_bad_shapes_before_any_gpu_call():
    from dycon_paper_replication_amd.utils import metrics as M
    lab = torch.zeros(2, 4, 6, 8, dtype=torch.int64)
    with pytest.raises(ValueError, match="2..8 classes"):
        M.class_dice_from_logits(torch.zeros(2, 9, 4, 6, 8), lab)
    with pytest.raises(ValueError, match="2..8 classes"):
        M.class_dice_from_logits(torch.zeros(2, 4, 6, 8, 1), lab)
    with pytest.raises(ValueError, match="do not match"):
        M.class_dice_from_logits(torch.zeros(2, 3, 4, 6, 9), lab)
    with pytest.raises(ValueError):
        M.class_dice_from_logits(torch.zeros(2, 3, 4, 6), lab)
    with pytest.raises(ValueError, match="2..8 classes"):
        M._class_confusion(torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8), 9)
    np.testing.assert_allclose(M.cal_dice(np.array([0, 1, 2, 2]), np.array([0, 1, 1, 2]), 3), [2 / 3, 2 / 3], rtol=1e-8)   # numpy path
