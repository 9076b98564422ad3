"""TrainConfig(num_classes=C), CPU side: the configuration contract, the declared C ABI of the C-class voxel losses, the 2-class
guard of the train-time metrics and the fixture tests/golden/voxel_losses_nc.npz (tests/golden/make_golden_trainer_nc.py)."""
import fnmatch
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from dycon_paper_replication_amd.trainer import TrainConfig
from dycon_paper_replication_amd.utils import metrics

ENTRY_POINTS = ("dycon_seg_lossesc_nsums", "dycon_seg_lossesc_fwd", "dycon_seg_lossesc_bwd", "dycon_seg_lossesc_finalize",
                "dycon_step_lossesc")


def test_default_is_two_classes():
    assert TrainConfig().num_classes == 2


@pytest.mark.parametrize("C", [2, 3, 8])
def test_class_count_constructs(C):
    assert TrainConfig(num_classes=C).num_classes == C


@pytest.mark.parametrize("kw", [dict(num_classes=1), dict(num_classes=9), dict(num_classes=3, use_gambling=1)],
                         ids=["one", "nine", "gambling3"])
def test_class_count_refused(kw):
    with pytest.raises(ValueError):
        TrainConfig(**kw)


def test_gambling_stays_available_for_two_classes():
    assert TrainConfig(num_classes=2, use_gambling=1).use_gambling == 1


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in include/dycon_hip.h"
    assert "5 + 3 * classes" in header                       # the accumulator layout is fixed in the header comment
    exports = open(os.path.join(ROOT, "dycon_paper_replication_amd", "csrc", "exports.map")).read()
    exports = re.sub(r"/\*.*?\*/", "", exports, flags=re.S)
    globs = [g.strip() for g in re.search(r"global:(.*?)local:", exports, re.S).group(1).split(";") if g.strip()]
    for name in ENTRY_POINTS:
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), f"{name} is not exported by csrc/exports.map"
    from dycon_paper_replication_amd import _lib
    source = open(os.path.join(ROOT, "dycon_paper_replication_amd", "csrc", "losses.hip")).read()
    for name in ENTRY_POINTS:
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert re.search(r'extern "C" int %s\(' % name, source), f"{name} is not defined in csrc/losses.hip"


def test_replay_patches_the_new_entry_points():
    """the replay patches scalars by entry-point name: the C-class entry points need theirs (a missing one replays stale schedules)"""
    import inspect
    from dycon_paper_replication_amd.trainer import DyconTrainer
    src = inspect.getsource(DyconTrainer._replay_step)
    for name in ("dycon_seg_lossesc_fwd", "dycon_seg_lossesc_bwd", "dycon_step_lossesc"):
        assert f'"{name}"' in src


@pytest.mark.parametrize("shape", [(1, 3, 4, 4, 4), (1, 4, 4, 4, 3)])
def test_metrics_refuse_other_widths_before_any_gpu_call(shape):
    logits = torch.zeros(shape)                                # a CPU tensor: a kernel call would fail differently
    labels = torch.zeros((1, 4, 4, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"class axis of width [34]"):
        metrics.batch_dice_from_logits(logits, labels)
    m = metrics.AsyncTrainMetrics(every=0)
    try:
        with pytest.raises(ValueError, match=r"class axis of width [34]"):
            m.update(0, logits, labels)
    finally:
        m.close()


def test_fixture_is_finite_and_labels_cover_the_classes():
    g = load_golden("voxel_losses_nc")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "voxel_losses_nc.npz")) < 1_000_000
    for k in g.files:
        if g[k].dtype.kind in "fiu":
            assert np.isfinite(g[k]).all(), k
    cases = [str(c) for c in g["cases"]]
    assert sorted(int(g[f"{c}.classes"]) for c in cases) == [3, 4, 4, 5, 5, 8]
    for c in cases:
        C, absent, counts = int(g[f"{c}.classes"]), int(g[f"{c}.absent"]), g[f"{c}.label_counts"]
        assert len(counts) == C and all((counts[k] > 0) != (k == absent) for k in range(C)), c
        if f"{c}.label" in g.files:
            lab = g[f"{c}.label"]
            assert lab.shape == (3, 6, 8, 10) and np.array_equal(np.bincount(lab.reshape(-1), minlength=C), counts)
        else:                                                  # the large case: more voxels than one pass of a 2048 x 256 grid
            assert 3 * int(np.prod(g[f"{c}.shape"])) > 2048 * 256
        for t in g["terms"]:
            assert g[f"{c}.{t}.fp32_dist"].shape == (2,)
    assert [str(c) for c in cases if int(g[f"{c}.absent"]) >= 0] == ["c4_absent"]
