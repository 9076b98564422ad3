"""utils/filters.py on the host: the numpy twin of the Gaussian kernel equals scipy.ndimage.gaussian_filter in every bit, and the
argument guards of the Python layer and of the C ABI (which rejects before any launch, so no GPU is needed)."""
import numpy as np
import pytest
from scipy import ndimage

import warp_ref as WR
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import filters as F


@pytest.mark.parametrize("mode", WR.GAUSS_MODES)
@pytest.mark.parametrize("shape,sigma", WR.GAUSS_CASES, ids=[f"c{n}" for n in range(len(WR.GAUSS_CASES))])
def test_host_twin_equals_scipy(shape, sigma, mode):
    a = np.random.default_rng(len(shape) + int(10 * sigma[0])).standard_normal(shape).astype(np.float32)
    ref = np.stack([ndimage.gaussian_filter(v, sigma, mode=mode) for v in a])
    got = F.gaussian_filter_host(a, sigma, mode)
    assert ref.dtype == np.float32 and np.count_nonzero(ref) > 0.9 * ref.size
    assert WR.same_bits(got, ref)
    assert not WR.same_bits(got, a)


def test_scalar_sigma_truncate_and_skipped_axes():
    a = np.random.default_rng(0).standard_normal((6, 7, 8)).astype(np.float32)
    assert WR.same_bits(F.gaussian_filter_host(a, 1.5, truncate=2.5), ndimage.gaussian_filter(a, 1.5, truncate=2.5))
    assert WR.same_bits(F.gaussian_filter_host(a, 0), a)                       # every axis skipped: a copy
    assert WR.same_bits(F.gaussian_filter_host(a, (0, 0.8, 0)), ndimage.gaussian_filter(a, (0, 0.8, 0)))
    assert F.gaussian_weights(0) is None and len(F.gaussian_weights(16)) == 2 * F.MAX_RADIUS + 1


def test_guards():
    a = np.zeros((4, 4, 4), dtype=np.float32)
    with pytest.raises(ValueError, match="limit is 64"):
        F.gaussian_filter_host(a, 16.2)                                         # radius 65
    with pytest.raises(ValueError, match="mode"):
        F.gaussian_filter_host(a, 1.0, mode="wrap")
    with pytest.raises(ValueError, match="sigma"):
        F.gaussian_filter_host(a, (1.0, 2.0))
    with pytest.raises(ValueError, match="sigma"):
        F.gaussian_filter_host(a, -1.0)
    with pytest.raises(ValueError, match="float32"):
        F.gaussian_filter_host(a.astype(np.float64), 1.0)
    import torch
    with pytest.raises(ValueError, match="CUDA float32"):
        F.gaussian_filter(torch.zeros(4, 4, 4), 1.0)


def test_library_rejects_before_any_launch():
    """the C ABI names the radius limit, rejects weights that are not symmetric and a workspace that is too small; the pointers are
    never dereferenced"""
    fake, w = 0x10000, np.ones(2 * 65 + 1)
    with pytest.raises(_lib.DyconLibraryError, match="0..64"):
        _lib.call("dycon_gaussian_filter", fake, fake + 4096, 1, 4, 4, 4, w.ctypes.data, 65, None, 0, None, 0, 0, 1.0, None, 0, None)
    w = np.array([0.25, 0.5, 0.26])
    with pytest.raises(_lib.DyconLibraryError, match="symmetric"):
        _lib.call("dycon_gaussian_filter", fake, fake + 4096, 1, 4, 4, 4, w.ctypes.data, 1, None, 0, None, 0, 0, 1.0, None, 0, None)
    w = np.array([0.25, 0.5, 0.25])
    with pytest.raises(_lib.DyconLibraryError, match="workspace"):
        _lib.call("dycon_gaussian_filter", fake, fake + 4096, 1, 4, 4, 4, w.ctypes.data, 1, w.ctypes.data, 1, None, 0, 0, 1.0, None, 0,
                  None)
    with pytest.raises(_lib.DyconLibraryError, match="mode"):
        _lib.call("dycon_gaussian_filter", fake, fake + 4096, 1, 4, 4, 4, w.ctypes.data, 1, None, 0, None, 0, 3, 1.0, None, 0, None)
    q = _lib.load().dycon_gaussian_filter_workspace
    assert [q(2, 3, 4, 5, n, 0) for n in range(4)] == [0, 0, 480, 480]
    assert [q(2, 3, 4, 5, n, 1) for n in range(4)] == [0, 480, 480, 960]
