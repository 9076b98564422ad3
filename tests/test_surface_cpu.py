"""Surface distances without a GPU: the numpy restatements of the kernels (tests/surface_ref.py) against scipy, the fp64 restatement of
the finalise kernel (utils/surface.metrics_from_hists) against the oracle's hd95 / asd, and the C ABI's declarations."""
import functools
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import surface_ref as SR
from conftest import ROOT
from oracle import evaluate as OE

from dycon_paper_replication_amd.utils import surface

ENTRY_POINTS = ["dycon_surface_workspace", "dycon_surface_hist", "dycon_surface_metrics"]


@functools.lru_cache(maxsize=None)
def _cases(shape):
    return SR.cases(shape)


@pytest.mark.parametrize("shape,name", SR.ALL_CASES)
def test_border_and_integer_edt_equal_scipy(shape, name):
    for m in _cases(shape)[name]:
        border = SR.border6(m)
        assert np.array_equal(border, m ^ ndimage.binary_erosion(m))
        edt = ndimage.distance_transform_edt(~border)
        d2 = SR.edt2_separable(border)
        assert d2.max() < SR.FAR
        assert np.array_equal(d2, np.rint(edt ** 2).astype(np.int64))
        assert np.array_equal(np.sqrt(d2.astype(np.float64)), edt)            # bit for bit


@pytest.mark.parametrize("shape,name", SR.ALL_CASES)
def test_metrics_from_hists_match_the_oracle(shape, name):
    a, b = _cases(shape)[name]
    hist, nborder = SR.hists(a, b)
    assert hist.shape == (2, SR.nbins_of(shape)) == (2, surface.nbins_of(shape))
    assert hist[0].sum() == nborder[0] and hist[1].sum() == nborder[1]
    got = surface.metrics_from_hists(hist, nborder, 95.0)
    assert got.shape == (1, 5)
    hd, asd_ab, asd_ba = OE.hd95(a, b), OE.asd(a, b), OE.asd(b, a)
    print(f"{shape} {name}: hd95 {got[0, 0]!r} oracle {hd!r}  asd {got[0, 1]!r} / {got[0, 2]!r} oracle {asd_ab!r} / {asd_ba!r}")
    assert got[0, 0] == hd
    np.testing.assert_allclose(got[0, 1:3], [asd_ab, asd_ba], rtol=1e-12, atol=0)
    assert got[0, 3:].tolist() == nborder.tolist()
    if name == "corners":
        assert hist[0, -1] == 1 and hist[1, -1] == 1
    if name == "identical":
        assert hist[:, 1:].sum() == 0


@pytest.mark.parametrize("q", [0.0, 50.0, 77.5, 100.0])
def test_other_percentiles_follow_numpy(q):
    a, b = _cases((17, 33, 70))["blobs"]
    hist, nborder = SR.hists(a, b)
    both = np.hstack((OE.surface_distances(a, b), OE.surface_distances(b, a)))
    assert surface.metrics_from_hists(hist, nborder, q)[0, 0] == np.percentile(both, q)


def test_empty_borders_give_nan_and_counts():
    a = _cases((5, 7, 130))["blobs"][0]
    empty = np.zeros_like(a)
    for x, y in ((a, empty), (empty, a), (empty, empty)):
        hist, nborder = SR.hists(x, y)
        assert hist.sum() == 0
        got = surface.metrics_from_hists(hist, nborder)
        assert np.isnan(got[0, :3]).all() and got[0, 3:].tolist() == [SR.border6(x).sum(), SR.border6(y).sum()]


def test_entry_points_declared_bound_and_built():
    header = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    from dycon_paper_replication_amd import _lib
    csrc = os.path.join(ROOT, "dycon_paper_replication_amd", "csrc")
    source = open(os.path.join(csrc, "surface.hip")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, header), f"{name} is not declared in include/dycon_hip.h"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"
        assert re.search(r'extern "C" (int|size_t) %s\(' % name, source), f"{name} is not defined in csrc/surface.hip"
    assert re.search(r"^SRCS\s*=.*\bsurface\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    assert len(_lib.SIGNATURES["dycon_surface_hist"][1]) == 15 and len(_lib.SIGNATURES["dycon_surface_metrics"][1]) == 7
    lib = _lib.load()                                           # host-side query: no GPU needed
    assert lib.dycon_surface_workspace(3, 96, 96, 96) == 3 * 2 * 96 ** 3 * 4
    assert "atomicAdd" in source and not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)", source)


def test_refusals_before_any_gpu_call():
    z = np.zeros((2, 4, 513), np.uint8)
    with pytest.raises(ValueError, match="1..512"):
        surface.surface_hists(z, z)
    with pytest.raises(ValueError, match="differ in shape"):
        surface.surface_hists(np.zeros((2, 3, 4)), np.zeros((2, 3, 5)))
    with pytest.raises(ValueError, match="lo >= 1"):
        surface.surface_hists(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), classes=(0, 2))
    with pytest.raises(ValueError, match="percentile"):
        surface.surface_metrics(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), q=101.0)
