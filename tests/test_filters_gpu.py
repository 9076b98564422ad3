"""dycon_gaussian_filter on the GPU: equal to the numpy twin and to scipy.ndimage.gaussian_filter itself in every bit (torch.equal
on the bit patterns), over the shapes that reach every path of the two kernels."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import warp_ref as WR
from dycon_paper_replication_amd.utils import filters as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("mode", WR.GAUSS_MODES)
@pytest.mark.parametrize("shape,sigma", WR.GAUSS_CASES, ids=[f"c{n}" for n in range(len(WR.GAUSS_CASES))])
def test_kernel_equals_twin_and_scipy(shape, sigma, mode):
    """c0, c1: radius above the axis lengths 9 and 7; c2: an axis of length 1, a row longer than a wave; c3: a skipped axis, ragged
    tiles, a row over 128; c4: the largest radius (64) on axes of 5 and 3"""
    a = np.random.default_rng(len(shape) + int(10 * sigma[0])).standard_normal(shape).astype(np.float32)
    twin = F.gaussian_filter_host(a, sigma, mode)
    ref = np.stack([ndimage.gaussian_filter(v, sigma, mode=mode) for v in a])
    assert WR.same_bits(twin, ref) and np.count_nonzero(ref) > 0.9 * ref.size
    x = torch.from_numpy(a).to(DEV)
    got = F.gaussian_filter(x, sigma, mode)
    assert torch.equal(_bits(got), _bits(torch.from_numpy(ref).to(DEV)))
    assert torch.equal(x.cpu(), torch.from_numpy(a))                                # the input is left alone
    # in place, with a caller's workspace, gives the same bits
    naxes = sum(s > 0 for s in sigma)
    ws = torch.empty(max(F.workspace_bytes(shape[0], shape[1:], naxes, True), 1), dtype=torch.uint8, device=DEV)
    y = x.clone()
    assert F.gaussian_filter(y, sigma, mode, out=y, workspace=ws) is y
    assert torch.equal(_bits(y), _bits(got))


def test_scale_single_axis_and_batch_axes():
    a = np.random.default_rng(5).standard_normal((2, 3, 9, 10, 11)).astype(np.float32)
    x = torch.from_numpy(a).to(DEV)
    ref = F.gaussian_filter_host(a, (0, 1.2, 0), "constant")
    got = F.gaussian_filter(x, (0, 1.2, 0), "constant", scale=2.5)
    assert WR.same_bits(got.cpu().numpy(), np.float32(2.5) * ref)
    y = x.clone()
    F.gaussian_filter(y, (0, 0, 0.9), out=y)                                         # one axis in place: through the workspace
    assert WR.same_bits(y.cpu().numpy(), F.gaussian_filter_host(a, (0, 0, 0.9)))
    assert torch.equal(F.gaussian_filter(x, 0), x)                                   # nothing to filter: a copy
    with pytest.raises(ValueError, match="limit is 64"):
        F.gaussian_filter(x, 16.2)
    with pytest.raises(ValueError, match="workspace"):
        F.gaussian_filter(x, 1.0, workspace=torch.empty(8, dtype=torch.uint8, device=DEV))
