"""GPU parity of conv_k3_halo_kernel: the small levels' bf16 k=3 convolution (Cin = 128) in one launch -- 4x4x4 voxel blocks x 64
columns, the split-K ranges of conv_k3_tile done by the waves of one workgroup, partials summed in LDS in the finish's order.

Every case is checked ELEMENT-WISE against F.conv3d in fp32 on the same bf16-rounded inputs and weights, with the bound of
test_fullsize_gpu (bf16 rounding of the result plus fp32 accumulation-order noise).  Shapes: the V-Net's 12^3 level at B = 4 (4 split
ranges), B = 8 (2) and B = 16 (1), ragged blocks in every direction (14 x 14 x 10, 13^3) and 256 output columns."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import ops
    from dycon_paper_replication_amd._lib import BF16, CONV_K3
from test_fullsize_gpu import assert_bf16_elementwise
from test_ops_gpu import mini_engine, nc, nd

DEV = "cuda:0"

# B, cin, cout, spatial: every shape here is served by conv_k3_halo_kernel (Cin = 128, at most 4 split ranges)
CASES = [
    (4, 128, 128, (12, 12, 12)),
    (4, 128, 128, (14, 14, 10)),
    (4, 128, 128, (13, 13, 13)),
    (2, 128, 256, (12, 12, 12)),
    (8, 128, 128, (12, 12, 12)),
    (16, 128, 128, (12, 12, 12)),
]


def _case(B, cin, cout, sp):
    rng = np.random.default_rng(zlib.crc32(repr((B, cin, cout, sp)).encode()))
    w = torch.from_numpy((rng.standard_normal((cout, cin, 3, 3, 3)) / np.sqrt(27 * cin)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal(cout).astype(np.float32))
    x = torch.from_numpy(rng.standard_normal((B, cin) + sp).astype(np.float32)).bfloat16().float()
    y0 = torch.from_numpy(rng.standard_normal((B, cout) + sp).astype(np.float32)).bfloat16().float()
    return w.bfloat16().float(), b, x, y0


def _run(w, b, x, out=None, accumulate=False):
    cout, cin = w.shape[:2]
    wd = w.to(DEV)
    wf = ops.pack_bfrag(wd, torch.bfloat16, 27, cin, cout, cout, 1, 27, 0, cin * 27)
    return ops.conv_gemm(nd(x, torch.bfloat16), wf, b.to(DEV), CONV_K3, cout, cout, out=out, accumulate=accumulate)


@pytest.mark.parametrize("B,cin,cout,sp", CASES)
def test_halo_conv_forward(B, cin, cout, sp):
    w, b, x, _ = _case(B, cin, cout, sp)
    assert ops.query("dycon_conv_gemm_splits", BF16, CONV_K3, 0, B, *sp, cin, cout) == 1
    assert ops.query("dycon_conv_gemm_workspace", BF16, CONV_K3, 0, B, *sp, cin, cout) == 0
    y = _run(w, b, x)
    torch.cuda.synchronize()
    assert_bf16_elementwise(nc(y), F.conv3d(x, w, b, padding=1), f"y {cin}->{cout} @ {sp} B={B}")


@pytest.mark.parametrize("B,cin,cout,sp", [CASES[0], CASES[2], CASES[4]])
def test_halo_conv_accumulate(B, cin, cout, sp):
    """accumulate = 1: y += conv(x) in place (the skip-gradient accumulation of the backward)"""
    w, b, x, y0 = _case(B, cin, cout, sp)
    y = nd(y0, torch.bfloat16)
    _run(w, b, x, out=y, accumulate=True)
    torch.cuda.synchronize()
    assert_bf16_elementwise(nc(y), F.conv3d(x, w, b, padding=1) + y0, f"y += conv {cin}->{cout} @ {sp} B={B}")


@pytest.mark.parametrize("B,cin,cout,sp", [CASES[0], CASES[5]])
def test_halo_conv_bitwise_repeatable(B, cin, cout, sp):
    """the in-workgroup reduction sums the waves' partials in a fixed order: two launches agree bit for bit"""
    w, b, x, _ = _case(B, cin, cout, sp)
    y1 = _run(w, b, x)
    y2 = _run(w, b, x)
    torch.cuda.synchronize()
    assert torch.equal(y1, y2)


@pytest.mark.parametrize("B,cin,cout,sp", [CASES[0], CASES[1]])
def test_halo_conv_data_gradient_engine(B, cin, cout, sp):
    """the data gradient of a k=3 conv through the engine (flipped, transposed weight fragments, the same entry point)"""
    w, b, x, _ = _case(B, cin, cout, sp)
    xr = x.clone().requires_grad_(True)
    yr = F.conv3d(xr, w, b, padding=1)
    gy = torch.randn(tuple(yr.shape), generator=torch.Generator().manual_seed(11)).bfloat16().float()
    yr.backward(gy)
    e = mini_engine({"l.weight": w, "l.bias": b}, torch.bfloat16)
    xd = nd(x, torch.bfloat16)
    y = e._conv("l", xd, "k3", need_gx=True)
    e.G[id(y)] = nd(gy, torch.bfloat16)
    for fn in reversed(e.tape):
        fn()
    torch.cuda.synchronize()
    assert_bf16_elementwise(nc(y), yr.detach(), f"y {cin}->{cout} @ {sp}")
    assert_bf16_elementwise(nc(e.G[id(xd)]), xr.grad, f"gx {cin}->{cout} @ {sp}")
