"""GPU: the rest of the reference's utils/losses.py on the HIP kernels (csrc/reflosses.hip, second half) against the reference's fp64
twin (tests/golden/losses_extra.npz; cases, call table and restatement in test_losses_extra_cpu.py).

Bounds, the package's fp32 contract (those of test_boundary_gpu.test_reference_loss_callables_golden): value rtol 1e-5; gradient
rtol 1e-4 with an absolute floor of 1e-6 * max |gradient|.  Every figure is printed before it is asserted (run with -s)."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_losses_extra_cpu import EXTRA_CASES, R, calls, fecl_case, losses_case, run_call, stride_of

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd.utils import losses

DEV = "cuda:0"
V_RTOL, G_RTOL, G_FLOOR = 1e-5, 1e-4, 1e-6
# an entropy MAP holds voxels whose probabilities are exactly one-hot; there H = -log(1 + 1e-6) ~ -1e-6, and p + 1e-6 is rounded to
# the fp32 grid, whose spacing at 1 is 2^-23: no fp32 evaluation (the reference's own included, see
# test_losses_extra_cpu.test_entropy_inputs_hold_exact_zeros_and_ones_and_fp32_rounds_there) is closer than that to the twin
MAP_ATOL = 2.0 ** -23


def check_value(tag, got, want):
    got, want = float(got), float(want)
    print(f"{tag}: value {got:.9g} twin {want:.9g} rel {abs(got - want) / abs(want):.2e}")
    assert math.isfinite(got) and abs(got - want) <= V_RTOL * abs(want), tag


def check_grad(tag, got, want, norm=None, norm_want=None, count=None):
    """got / want: numpy arrays (the sampled gradient and the twin's); optionally the 2-norms of the whole gradients"""
    assert np.isfinite(got).all(), tag
    gmax = np.abs(want).max()
    excess = np.abs(got - want) - (G_RTOL * np.abs(want) + G_FLOOR * gmax)
    print(f"{tag}: grad max|err| {np.abs(got - want).max():.3e} max|twin| {gmax:.3e} worst margin {excess.max():.3e}")
    assert (excess <= 0).all(), tag
    if norm is not None:
        # elements within rtol |g| + floor each put the norm within rtol ||g|| + floor sqrt(count)
        print(f"{tag}: grad norm {norm:.9g} twin {norm_want:.9g}")
        assert abs(norm - norm_want) <= G_RTOL * norm_want + G_FLOOR * gmax * math.sqrt(count), tag


def to_layout(t, layout):
    """the case on the device: plain NCDHW, channels-last-3D, or every (N, C, ...) input a slice x[1:, :C] of a larger tensor"""
    C = t["C"]
    out = {}
    for k, v in t.items():
        if not torch.is_tensor(v):
            out[k] = v
            continue
        v = v.to(DEV)
        if k in ("a", "b", "p", "q"):
            if layout == "channels_last":
                v = v.contiguous(memory_format=torch.channels_last_3d)
            elif layout == "sliced":
                big = torch.full((v.shape[0] + 1, C + 1) + tuple(v.shape[2:]), 7.0, device=DEV)
                big[1:, :C] = v
                v = big[1:, :C]
                assert v.storage_offset() > 0 and v.stride(1) * (C + 1) == big.stride(0)
        out[k] = v
    return out


@pytest.mark.parametrize("layout", ["ncdhw", "channels_last", "sliced"])
@pytest.mark.parametrize("i", range(len(EXTRA_CASES)))
def test_callables_against_fp64_twin(i, layout):
    """every entry of the call table (dice_loss1 on the class slice p[:, 1] with a hard and a soft target, softmax_dice_loss, the four
    entropy names, symmetric_mse_loss, compute_kl_loss, FocalLoss over gamma / alpha / size_average): value and the gradient of
    every differentiable input against the reference's fp64 twin, in three memory layouts"""
    g = load_golden("losses_extra")
    t = to_layout(losses_case(i), layout)
    st = stride_of(i)
    for name, (fn, wrt) in calls(t["C"]).items():
        v, gr = run_call(losses, fn, wrt, t)
        key = f"c{i}_{name}"
        assert v.dtype == torch.float32
        check_value(f"{key}/{layout}", v, g[key + "_v64"])
        for k, gk in enumerate(gr):
            assert gk.shape == t[wrt[k]].shape and gk.dtype == torch.float32
            check_grad(f"{key}/{layout}/d{wrt[k]}", gk.flatten()[::st].cpu().numpy(), g[f"{key}_g{k}_64"], gk.double().norm().item(),
                       float(g[f"{key}_g{k}n_64"]), gk.numel())
    for name, m in (("entropy_map", losses.entropy_map(t["p"])), ("entropy_loss_map", losses.entropy_loss_map(t["p"], C=t["C"]))):
        assert m.shape == (t["p"].shape[0], 1) + tuple(t["p"].shape[2:]) and m.dtype == torch.float32
        got, want = m.flatten()[::st].cpu().numpy(), g[f"c{i}_{name}_out64"]
        print(f"c{i}_{name}/{layout}: map max|err| {np.abs(got - want).max():.3e}")
        np.testing.assert_allclose(got, want, rtol=V_RTOL, atol=MAP_ATOL)


def test_focal_2d_input_and_uint8_target():
    """(M, C) logits, as the reference's dim() == 2 branch, and a uint8 target"""
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(37, 3, generator=gen)
    y = torch.randint(0, 3, (37,), generator=gen)
    xd = x.double().requires_grad_(True)
    want = R.FocalLoss(2, [0.2, 0.3, 0.5], True)(xd, y)
    gw = torch.autograd.grad(want, xd)[0].numpy()
    for tgt in (y.to(DEV), y.to(torch.uint8).to(DEV)):
        xg = x.to(DEV).requires_grad_(True)
        v = losses.FocalLoss(2, [0.2, 0.3, 0.5], True)(xg, tgt)
        check_value("focal (M, C)", v, want.item())
        check_grad("focal (M, C)", torch.autograd.grad(v, xg)[0].cpu().numpy(), gw)


@pytest.mark.parametrize("shape", [(5, 2), (3, 4, 7), (2, 3, 5, 64), (2, 2, 3, 96), (3, 2, 200), (2, 2, 256), (1, 3, 700)])
def test_compute_kl_last_dimension_lengths(shape):
    """the last-dimension softmax over the lane-group sizes of the kernel (L = 2 .. 256 and beyond), fp64 restatement on the host"""
    gen = torch.Generator().manual_seed(shape[-1])
    a, b = 2 * torch.randn(*shape, generator=gen), 2 * torch.randn(*shape, generator=gen)
    ad, bd = a.double().requires_grad_(True), b.double().requires_grad_(True)
    want = R.compute_kl_loss(ad, bd)
    gw = torch.autograd.grad(want, [ad, bd])
    ag, bg = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    v = losses.compute_kl_loss(ag, bg)
    check_value(f"compute_kl {shape}", v, want.item())
    for gk, wk in zip(torch.autograd.grad(v, [ag, bg]), gw):
        check_grad(f"compute_kl {shape}", gk.cpu().numpy(), wk.numpy())


def test_compute_kl_refuses_unsupported_length():
    from dycon_paper_replication_amd._lib import DyconLibraryError
    a = torch.zeros(2, 1025, device=DEV)
    with pytest.raises(DyconLibraryError, match="1 <= L <= 1024"):
        losses.compute_kl_loss(a, a)


def test_legacy_fecl_against_reference():
    """losses.FeCLoss(device, temperature) against the reference's LEGACY class (fixture), not against dycon_losses.FeCLoss"""
    g = load_golden("losses_extra")
    feat, mask = fecl_case()
    f = feat.to(DEV).requires_grad_(True)
    v = losses.FeCLoss(DEV, temperature=0.6)(f, mask.to(DEV))
    check_value("legacy fecl", v, g["fecl_v64"])
    check_grad("legacy fecl", torch.autograd.grad(v, f)[0].cpu().numpy(), g["fecl_g64"])


@pytest.fixture(scope="module")
def full():
    """(4, 2, 96, 96, 96) inputs on the device, built once"""
    gen = torch.Generator().manual_seed(77)
    shape = (4, 2, 96, 96, 96)
    a = (2.0 * torch.randn(*shape, generator=gen)).to(DEV)
    b = (a + 1.5 * torch.randn(*shape, generator=gen).to(DEV))
    label = torch.randint(0, 2, (4, 96, 96, 96), generator=gen).to(DEV)
    r = (0.5 + torch.rand(4, 1, 96, 96, 96, generator=gen)).to(DEV)
    return {"a": a, "b": b, "p": torch.softmax(a, 1), "q": torch.softmax(b, 1), "label": label, "tf": (label == 1).float(), "r": r, "C": 2}


@pytest.mark.parametrize("name", ["dice1_soft", "softmax_dice", "entropy_min", "entropy_map", "sym_mse", "compute_kl", "focal3"])
def test_full_size_against_fp64_on_device(full, name):
    """one case per family at the training shape against the restatement run on the device in fp64: grid and stride arithmetic at
    28 M elements and the double accumulators at real voxel counts"""
    fn, wrt = calls(2)[name]
    v, gr = run_call(losses, fn, wrt, full)
    want, gw = run_call(R, fn, wrt, full, torch.float64)
    check_value(f"full {name}", v, want.item())
    for k, (gk, wk) in enumerate(zip(gr, gw)):
        gmax = wk.abs().max()
        excess = ((gk.double() - wk).abs() - (G_RTOL * wk.abs() + G_FLOOR * gmax)).max().item()
        print(f"full {name} d{wrt[k]}: max|twin| {gmax.item():.3e} worst margin {excess:.3e}")
        assert torch.isfinite(gk).all() and excess <= 0


def test_nan_in_gives_nan_out():
    """a NaN input is a NaN loss (never a clamped number); a map is NaN at that voxel only"""
    t = to_layout(losses_case(1), "ncdhw")
    for name, (fn, wrt) in calls(t["C"]).items():
        tt = dict(t)
        for k in wrt:
            x = t[k].clone()
            x[0, 1, 3, 4, 2] = float("nan")
            tt[k] = x
        assert torch.isnan(fn(losses, tt)).item(), name
    p = t["p"].clone()
    p[0, 1, 3, 4, 2] = float("nan")
    m = losses.entropy_map(p)
    assert torch.isnan(m[0, 0, 3, 4, 2]).item() and int(torch.isnan(m).sum()) == 1
    lab = t["label"].clone()
    lab[0, 1, 1, 1] = 9                                     # a label outside 0..C-1: the reference raises, this is NaN
    assert torch.isnan(losses.FocalLoss()(t["a"], lab)).item()


def test_determinism():
    """two calls on the same input: the element-wise outputs (maps, gradients) have no cross-thread sums and are bit-equal; a scalar
    is a sum of per-block doubles added atomically in arrival order, so its double may differ in the last bits and its fp32 rounding
    by at most one ulp (the existing softmax_kl_loss has the same property)"""
    t = to_layout(losses_case(0), "ncdhw")
    assert torch.equal(losses.entropy_map(t["p"]), losses.entropy_map(t["p"]))
    assert torch.equal(losses.entropy_loss_map(t["p"], C=2), losses.entropy_loss_map(t["p"], C=2))
    for name, (fn, wrt) in calls(t["C"]).items():
        (v1, g1), (v2, g2) = run_call(losses, fn, wrt, t), run_call(losses, fn, wrt, t)
        assert abs(v1.item() - v2.item()) <= float(np.spacing(np.float32(abs(v1.item())))), name
        if name in ("entropy_min", "entropy_map", "entropy_loss", "entropy_loss_map", "sym_mse", "compute_kl") or name.startswith("focal"):
            for x, y in zip(g1, g2):                        # these gradients do not read the forward's sums
                assert torch.equal(x, y), name
