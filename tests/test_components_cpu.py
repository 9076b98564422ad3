"""The component kernels' declarations, and the oracle and named inputs of tests/test_components_gpu.py checked on the host: every
named case has the property it is named for, so the GPU tests cannot pass vacuously."""
import inspect
import os
import re

import numpy as np
import pytest

import components_ref as CR
from dycon_paper_replication_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dycon_cc_workspace", "dycon_cc_roots", "dycon_cc_labels", "dycon_cc_largest")


def test_entry_points_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    declared = set(re.findall(r"\b(dycon_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRY_POINTS:
        assert name in declared and name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    srcs = re.search(r"^SRCS\s*=(.*)$", open(os.path.join(ROOT, "dycon_paper_replication_amd", "csrc", "Makefile")).read(), re.M).group(1)
    assert "components.hip" in srcs.split()


def test_module_exported():
    from dycon_paper_replication_amd import utils
    for name in ("component_roots", "label_components", "largest_component", "largest_component_per_class"):
        assert callable(getattr(utils.components, name))
    for name in ("test_all_case", "test_all_case_BraTS19", "test_all_case_Pancreas", "test_all_case_ISLES22"):
        f = getattr(utils.device_eval, name)
        assert f.__test__ is False and inspect.signature(f).parameters["nms"].default == 0
        assert list(inspect.signature(f).parameters) == list(inspect.signature(getattr(utils.test_3d_patch, name)).parameters)
    assert inspect.signature(utils.eval_classes.test_all_case_classes).parameters["nms"].default == 0
    assert callable(utils.sliding_window.single_case_device)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_by_value_oracle_is_a_flood_fill(connectivity):
    vol = np.random.default_rng(11).integers(0, 4, (4, 5, 6))
    vol[0, 0, 0] = 300                                        # outside 1..255: background
    labels, n, root = CR.label_by_value(vol, connectivity)
    flood, m = CR.flood_by_value(vol, connectivity)
    assert n == m and n > 3
    np.testing.assert_array_equal(labels, flood)
    assert labels[0, 0, 0] == 0 and root[0, 0, 0] == 0
    idx = np.arange(vol.size).reshape(vol.shape)
    for k in range(1, n + 1):
        assert (root[labels == k] == idx[labels == k].min() + 1).all()
        assert len(np.unique(vol[labels == k])) == 1


def test_binary_oracle_roots_and_numbering():
    vol = CR.random_mask((5, 7, 9), 0.3, 2)
    labels, n = CR.label(vol, 1)
    root = CR.roots(labels, n)
    first = [int(np.flatnonzero(labels.ravel() == k)[0]) for k in range(1, n + 1)]
    assert first == sorted(first)                             # scipy numbers components in raster order of their first voxel
    assert [int(root.ravel()[i]) for i in first] == [i + 1 for i in first]
    by_value = CR.label_by_value(vol, 1)
    np.testing.assert_array_equal(by_value[0], labels)       # one value: the binary labelling
    np.testing.assert_array_equal(by_value[2], root)


@pytest.mark.parametrize("shape", CR.SHAPES)
def test_named_cases_have_their_property(shape):
    cases = CR.named(shape)
    assert sorted(cases) == sorted(CR.NAMES)
    count = lambda name, c: CR.label(cases[name], c)[1]      # noqa: E731
    assert [count("pair_110", c) for c in (1, 2, 3)] == [8, 4, 4]
    assert [count("pair_111", c) for c in (1, 2, 3)] == [8, 8, 4]
    n_even = int(cases["checkerboard"].sum())
    assert [count("checkerboard", c) for c in (1, 2, 3)] == [n_even, 1, 1] and n_even > 1000
    assert count("serpentine", 1) == 1 and cases["serpentine"].sum() > shape[2] * (shape[0] // 2) * (shape[1] // 2)
    s = cases["serpentine"].astype(int)
    # one voxel wide: no 2 x 2 square in an axis-aligned plane
    assert (s[:-1, :-1] + s[1:, :-1] + s[:-1, 1:] + s[1:, 1:]).max() < 4 and (s[:, :-1, :-1] + s[:, 1:, :-1] + s[:, :-1, 1:] +
                                                                             s[:, 1:, 1:]).max() < 4
    assert count("full", 1) == 1 and cases["full"].all()
    assert count("empty", 3) == 0
    assert count("corner", 3) == 1 and cases["corner"].sum() == 1 and cases["corner"][-1, -1, -1]
    assert count("frame", 1) == 1 and cases["frame"].sum() == 4 * (sum(shape) - 6) + 8
    labels, n = CR.label(cases["two_cubes"], 3)
    assert n == 2 and np.bincount(labels.ravel())[1:].tolist() == [27, 27]
    mask, size = CR.largest(cases["two_cubes"], 3)
    assert size == 27 and mask[1, 1, 2] == 1 and mask[-2, -2, -3] == 0      # the earlier in raster order wins
    assert [count("faces", c) for c in (1, 2, 3)] == [2, 2, 2]


def test_largest_per_class_oracle():
    vol = np.zeros((6, 6, 6), np.int64)
    vol[0:2, 0:2, 0:2] = 1
    vol[4, 4, 4] = 1
    vol[3:6, 0:2, 0] = 3
    vol[0, 5, 5] = 3
    out = CR.largest_per_class(vol, 4)
    assert out.sum() == 8 * 1 + 6 * 3 and out[4, 4, 4] == 0 and out[0, 5, 5] == 0 and (out == 2).sum() == 0
