"""The comparison helpers of the GPU parity tests, on the CPU: they must reject a NaN or an Inf anywhere in a result (a NaN compares
False with every bound), still accept a result within its bound, and the fp64 convolution / normalisation references of
tests/ref64.py must agree with torch autograd in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ref64 import conv_ref64, norm_ref64
from test_fullsize_gpu import assert_bf16_elementwise


def _pair(seed=0, shape=(2, 3, 4, 8, 8)):
    ref = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return ref.bfloat16().float(), ref       # the bf16 rounding of ref is within the helper's bound


def test_bf16_elementwise_accepts_rounded_result():
    got, ref = _pair()
    assert_bf16_elementwise(got, ref, "rounded")
    assert_bf16_elementwise(got.bfloat16(), ref.double(), "rounded, other dtypes")


@pytest.mark.parametrize("where", ["first", "middle", "last", "half", "all"])
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_bf16_elementwise_rejects_non_finite(where, bad):
    got, ref = _pair(1)
    flat = got.reshape(-1)
    sel = {"first": slice(0, 1), "middle": slice(flat.numel() // 2, flat.numel() // 2 + 1), "last": slice(-1, None),
           "half": slice(0, None, 2), "all": slice(None)}[where]
    flat[sel] = bad
    with pytest.raises(AssertionError, match="NaN / Inf"):
        assert_bf16_elementwise(got, ref, "poisoned")


def test_bf16_elementwise_rejects_non_finite_reference():
    got, ref = _pair(2)
    ref.reshape(-1)[7] = float("nan")
    with pytest.raises(AssertionError, match="reference"):
        assert_bf16_elementwise(got, ref, "bad reference")


def test_bf16_elementwise_still_rejects_a_wrong_element():
    got, ref = _pair(3)
    got[1, 2, 3, 4, 5] += 0.1 * float(ref.abs().max())
    with pytest.raises(AssertionError, match="one wrong element: 1 elements off"):
        assert_bf16_elementwise(got, ref, "one wrong element")


def test_empty_is_nan_under_deterministic_fill():
    """the poisoned-memory fixture of test_dispatch_parity_gpu.py relies on this (checked there again on the GPU)"""
    prev = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    try:
        torch.use_deterministic_algorithms(True, warn_only=True)
        assert torch.utils.deterministic.fill_uninitialized_memory
        assert torch.isnan(torch.empty(1000)).all() and torch.isnan(torch.empty(10, dtype=torch.bfloat16)).all()
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])


# kind, B, cin, cout, spatial (input): ragged, odd channel counts, every tap of every kind
CONV_CASES = [("k3", 2, 3, 5, (5, 4, 7)), ("k3", 1, 1, 4, (3, 6, 2)), ("k3", 3, 4, 2, (1, 2, 3)),
              ("k2s2", 2, 3, 5, (6, 4, 8)), ("k2s2", 1, 2, 3, (2, 2, 2)),
              ("deconv", 2, 5, 3, (3, 2, 5)), ("deconv", 1, 2, 4, (1, 1, 1)),
              ("1x1", 2, 6, 3, (3, 5, 2))]


@pytest.mark.parametrize("kind,B,cin,cout,sp", CONV_CASES)
def test_conv_ref64_matches_torch_autograd(kind, B, cin, cout, sp):
    gen = torch.Generator().manual_seed(B * 100 + cin * 10 + cout)
    k = {"k3": 3, "k2s2": 2, "deconv": 2, "1x1": 1}[kind]
    wshape = (cin, cout, k, k, k) if kind == "deconv" else (cout, cin, k, k, k)
    x = torch.randn((B, cin) + sp, generator=gen, dtype=torch.float64, requires_grad=True)
    w = torch.randn(wshape, generator=gen, dtype=torch.float64, requires_grad=True)
    b = torch.randn(cout, generator=gen, dtype=torch.float64, requires_grad=True)
    if kind == "k3":
        y = F.conv3d(x, w, b, padding=1)
    elif kind == "k2s2":
        y = F.conv3d(x, w, b, stride=2)
    elif kind == "deconv":
        y = F.conv_transpose3d(x, w, b, stride=2)
    else:
        y = F.conv3d(x, w, b)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    y.backward(gy)
    cl = lambda t: t.permute(0, 2, 3, 4, 1).contiguous()   # noqa: E731
    y2, gx2, gw2, gb2 = conv_ref64(kind, cl(x.detach()), w.detach(), b.detach(), cl(gy))
    for name, got, ref in (("y", y2, cl(y.detach())), ("gx", gx2, cl(x.grad)), ("gw", gw2, w.grad), ("gb", gb2, b.grad)):
        assert got.dtype == torch.float64 and got.shape == ref.shape, name
        np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-11, atol=1e-11, err_msg=name)


@pytest.mark.parametrize("kind,mode", [("gn", "relu"), ("in", "skip"), ("bn", "scale"), ("bn", "eval")])
def test_norm_ref64_layout_and_running_statistics(kind, mode):
    """the channels-last wrapper against the same torch calls on NCDHW, BatchNorm's running statistics included"""
    gen = torch.Generator().manual_seed(5)
    B, C, sp = 3, 32, (4, 3, 5)
    z = torch.randn((B,) + sp + (C,), generator=gen)
    gy = torch.randn((B,) + sp + (C,), generator=gen)
    skip = torch.randn((B,) + sp + (C,), generator=gen) if mode == "skip" else None
    cs = (torch.rand(B * C, generator=gen) > 0.5).float() * 2 if mode == "scale" else None
    gamma = torch.randn(C, generator=gen) * 0.3 + 1 if kind != "in" else None
    beta = torch.randn(C, generator=gen) * 0.3 if kind != "in" else None
    run = (torch.randn(C, generator=gen, dtype=torch.float64), torch.rand(C, generator=gen, dtype=torch.float64) + 0.5)
    run0 = tuple(t.clone() for t in run)
    training = mode != "eval"
    y, gz, dg, db, gs = norm_ref64(kind, z, gy, gamma, beta, relu=True, skip=skip, chan_scale=cs,
                                   running=run if kind == "bn" else None, training=training)
    zr = z.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    if kind == "gn":
        n = F.group_norm(zr, 16, gamma.double(), beta.double(), 1e-5)
    elif kind == "in":
        n = F.instance_norm(zr, eps=1e-5)
    else:
        rm, rv = run0[0].clone(), run0[1].clone()
        n = F.batch_norm(zr, rm, rv, gamma.double(), beta.double(), training, 0.1, 1e-5)
        np.testing.assert_allclose(run[0].numpy(), rm.numpy(), rtol=1e-14)
        np.testing.assert_allclose(run[1].numpy(), rv.numpy(), rtol=1e-14)
        assert torch.equal(run[0], run0[0]) != training, "running mean updated in eval mode / not updated in training"
    r = F.relu(n)
    if cs is not None:
        r = r * cs.double().reshape(B, C, 1, 1, 1)
    if skip is not None:
        r = r + skip.double().permute(0, 4, 1, 2, 3)
    r.backward(gy.double().permute(0, 4, 1, 2, 3))
    np.testing.assert_allclose(y.numpy(), r.detach().permute(0, 2, 3, 4, 1).numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gz.numpy(), zr.grad.permute(0, 2, 3, 4, 1).numpy(), rtol=1e-12, atol=1e-12)
    if skip is not None:
        assert torch.equal(gs, gy.double())
