"""dataloaders/device_warp.py on the host: the numpy twins of the warp kernels equal scipy.ndimage.affine_transform /
map_coordinates in every bit, draw_plan_warp is deterministic, the default DeviceBatchLoader draws what it drew before, and the
argument guards."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import warp_ref as WR
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.dataloaders import (DeviceBatchLoader, DeviceVolumeCache, apply_plan_host, draw_plan)
from dycon_paper_replication_amd.dataloaders import device_warp as W
from dycon_paper_replication_amd.dataloaders.brats19 import TwoStreamBatchSampler
from dycon_paper_replication_amd.dataloaders.device_cache import PLAN_DTYPE


def _host():
    cs = WR.cases()
    return [c["image"] for c in cs], [c["label"] for c in cs]


def test_warp_volume_twin_equals_scipy_on_random_cases():
    """60 cases: volume axes 1..11, output axes 1..9 (some volumes smaller than the output), integer coordinates on the edges,
    scale-only and general matrices, a displacement every third case; order 1 on fp32 / fp64, order 0 on uint8"""
    rng = np.random.default_rng(11)
    voxels = inside = 0
    for case in range(60):
        n = tuple(rng.integers(1 if case % 6 == 0 else 6, 12, 3))
        shape = tuple(int(v) for v in rng.integers(1, 10, 3))
        v32 = rng.standard_normal(n).astype(np.float32)
        v8 = rng.integers(0, 5, n).astype(np.uint8)
        if case % 4 == 0:
            m, off = np.eye(3), rng.integers(-1, 3, 3).astype(np.float64)           # exact integers: the edges n - 1 are hit
        elif case % 4 == 1:
            m, off = np.diag(rng.uniform(0.8, 1.25, 3)), rng.uniform(-1, 3, 3)
        else:
            m, off = W.affine_of(rng.uniform(0.8, 1.25), rng.uniform(-20, 20, 3), rng.integers(-1, 3, 3), shape)
        disp = (1.5 * rng.standard_normal((3,) + shape)).astype(np.float32) if case % 3 == 0 else None
        for a, order in ((v32, 1), (v32.astype(np.float64), 1), (v8, 0)):
            if disp is None:
                ref = ndimage.affine_transform(a, m, off, output_shape=shape, order=order, mode="constant", cval=0)
            else:
                ref = ndimage.map_coordinates(a, W.source_coordinates(m, off, shape, disp), order=order, mode="constant", cval=0)
            got = W.warp_volume_host(a, m, off, shape, order, disp)
            assert WR.same_bits(got, ref), (case, order, a.dtype)
        voxels += int(np.prod(shape))
        inside += int(np.count_nonzero(W.warp_volume_host(np.ones(n, np.uint8), m, off, shape, 0, disp)))
    assert voxels > 5000 and 0.2 * voxels < inside < 0.95 * voxels


@pytest.mark.parametrize("kind", WR.KINDS)
def test_plan_twin_equals_scipy(kind):
    """every rot90 count with every flip: scipy's transform of the stored case, then np.rot90 and np.flip"""
    images, labels = _host()
    plan, disp = WR.make_plan(kind, 3)
    out = W.apply_warp_plan_host(plan, images, labels, disp, onehot=3)
    print(kind, "inside the source:", WR.check_band(out))
    for n, rec in enumerate(plan):
        img, lab, m = images[rec["case"]], labels[rec["case"]], rec["m"].reshape(3, 3)
        if rec["elastic"]:
            c = W.source_coordinates(m, rec["off"], WR.PATCH, disp[n])
            ri = ndimage.map_coordinates(img, c, order=1, mode="constant", cval=0)
            rl = ndimage.map_coordinates(lab, c, order=0, mode="constant", cval=0)
        else:
            ri = ndimage.affine_transform(img, m, rec["off"], output_shape=WR.PATCH, order=1, mode="constant", cval=0)
            rl = ndimage.affine_transform(lab, m, rec["off"], output_shape=WR.PATCH, order=0, mode="constant", cval=0)
        ri, rl = np.rot90(ri, rec["k"]), np.rot90(rl, rec["k"])
        if rec["flip_axis"] >= 0:
            ri, rl = np.flip(ri, rec["flip_axis"]), np.flip(rl, rec["flip_axis"])
        assert WR.same_bits(out["image"][n, 0], np.ascontiguousarray(ri)), n
        assert np.array_equal(out["label"][n], rl), n
    assert np.array_equal(out["onehot_label"], np.stack([out["label"] == c for c in range(3)], axis=1))
    if kind == "shift":                                                           # the identity: assemble_batch's bits
        plain = np.zeros(len(plan), dtype=PLAN_DTYPE)
        for f in PLAN_DTYPE.names:
            plain[f] = plan[f]
        ref = apply_plan_host(plain, images, labels)
        assert WR.same_bits(out["image"], ref["image"]) and np.array_equal(out["label"], ref["label"])
        idle = plan.copy()
        idle["warp"] = 0                                                          # and so is a record that is not warped at all
        again = W.apply_warp_plan_host(idle, images, labels)
        assert WR.same_bits(again["image"], ref["image"]) and np.array_equal(again["label"], ref["label"])


def test_draw_plan_warp_is_deterministic_and_draws_a_fixed_number():
    warp = W.Warp(p_affine=0.7, p_elastic=0.5, alpha=(10, 30), sigma=(2, 4))
    inten = W.Intensity(p_gain=0.5, p_bias=0.5, p_gamma=0.5, p_blur=0.5)
    idx = [0, 1, 2, 1, 0, 2, 1, 1]
    np.random.seed(4)
    a = W.draw_plan_warp(WR.SHAPES, idx, WR.PATCH, warp, inten)
    state = np.random.get_state()[1].copy()
    np.random.seed(4)
    b = W.draw_plan_warp(WR.SHAPES, idx, WR.PATCH, warp, inten)
    assert a.tobytes() == b.tobytes() and a.dtype == W.WARP_PLAN_DTYPE
    assert 0 < a["warp"].sum() and 0 < a["elastic"].sum() < len(idx) and (a["gain"] != 1).any() and (a["gain"] == 1).any()
    assert ((a["elastic"] == 0) | (a["warp"] == 1)).all()
    # every coin that does not show still draws: a plan with other probabilities leaves the generator in the same state
    np.random.seed(4)
    c = W.draw_plan_warp(WR.SHAPES, idx, WR.PATCH, W.Warp(p_affine=0, p_elastic=0), W.Intensity())
    assert np.array_equal(np.random.get_state()[1], state)
    assert not c["warp"].any() and (c["gain"] == 1).all() and (c["blur_sigma"] == 0).all()
    for f in PLAN_DTYPE.names:
        assert np.array_equal(a[f], c[f])
    for rec in a[a["warp"] == 1]:
        m, off = W.affine_of(rec["scale"], rec["angles"], rec["origin"], rec["patch"])
        assert np.array_equal(m.reshape(9), rec["m"]) and np.array_equal(off, rec["off"])
        ctr = (np.asarray(WR.PATCH) - 1) / 2
        assert np.allclose(m @ ctr + off, rec["origin"] + ctr, atol=1e-9)         # the patch centre stays where the crop put it
    # without a Warp or an Intensity: draw_plan's draws
    np.random.seed(9)
    d = W.draw_plan_warp(WR.SHAPES, idx, WR.PATCH)
    s1 = np.random.get_state()[1].copy()
    np.random.seed(9)
    e = draw_plan(WR.SHAPES, idx, WR.PATCH)
    assert np.array_equal(np.random.get_state()[1], s1)
    for f in PLAN_DTYPE.names:
        assert np.array_equal(d[f], e[f])


def test_default_loader_draws_what_it_drew_before():
    """warp=None, intensity=None: DeviceBatchLoader.plans() consumes np.random as draw_plan run directly does"""
    cache = DeviceVolumeCache(WR.cases(), device="cpu")
    np.random.seed(12)
    sampler = TwoStreamBatchSampler([0, 1, 0, 1], [2], 3, 1)
    loader = DeviceBatchLoader(cache, sampler, WR.PATCH)
    plans = list(loader.plans())
    state = np.random.get_state()[1].copy()
    np.random.seed(12)
    direct = [draw_plan(cache.shapes, [int(i) for i in batch], WR.PATCH) for batch in TwoStreamBatchSampler([0, 1, 0, 1], [2], 3, 1)]
    assert np.array_equal(np.random.get_state()[1], state)
    assert len(plans) == len(direct) == 2
    for p, q in zip(plans, direct):
        assert p.dtype == PLAN_DTYPE and p.tobytes() == q.tobytes()
    assert loader._aug is None
    # with a Warp the records extend those, from the same crop draws in front of its own
    np.random.seed(12)
    wl = DeviceBatchLoader(cache, TwoStreamBatchSampler([0, 1, 0, 1], [2], 3, 1), WR.PATCH, warp=W.Warp())
    first = next(iter(wl.plans()))
    assert first.dtype == W.WARP_PLAN_DTYPE and np.array_equal(first["origin"][0], direct[0]["origin"][0])


def test_guards():
    images, labels = _host()
    cache = DeviceVolumeCache(WR.cases(), device="cpu")
    sampler = TwoStreamBatchSampler([0, 1, 0, 1], [2], 3, 1)
    with pytest.raises(ValueError, match="rot=True"):
        DeviceBatchLoader(cache, sampler, WR.PATCH, rot=True, warp=W.Warp())
    with pytest.raises(ValueError, match="Warp"):
        DeviceBatchLoader(cache, sampler, WR.PATCH, warp=(0.5, 1.0))
    for bad in (dict(p_affine=1.5), dict(scale=(0, 1)), dict(scale=(1.2, 0.9)), dict(angles_deg=(10, 10)), dict(alpha=(-1, 2)),
                dict(sigma=(0, 1))):
        with pytest.raises(ValueError):
            W.Warp(**bad)
    for bad in (dict(p_blur=-0.1), dict(gamma=(0, 1)), dict(range=(1, 1)), dict(blur_sigma=(2, 1))):
        with pytest.raises(ValueError):
            W.Intensity(**bad)
    plan, disp = WR.make_plan("general_disp", 3)
    with pytest.raises(ValueError, match="displacement"):
        W.apply_warp_plan_host(plan, images, labels)
    with pytest.raises(ValueError, match="displacement"):
        W.apply_warp_plan_host(plan, images, labels, disp.astype(np.float64))
    with pytest.raises(ValueError, match="WARP_PLAN_DTYPE"):
        W.apply_warp_plan_host(draw_plan(WR.SHAPES, [0], WR.PATCH), images, labels)
    odd = plan.copy()
    odd["patch"] = (8, 7, 6)
    with pytest.raises(ValueError, match="square"):
        W.apply_warp_plan_host(odd, images, labels, disp)
    nan = plan.copy()
    nan["m"][0, 0] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        W.apply_warp_plan_host(nan, images, labels, disp)
    with pytest.raises(_lib.DyconLibraryError, match="GPU only"):
        W.assemble_batch_warp(cache, WR.make_plan("general", 3)[0])
    with pytest.raises(ValueError, match="order"):
        W.warp_volume_host(images[0], np.eye(3), np.zeros(3), (4, 4, 4), order=3)
    with pytest.raises(ValueError, match="CUDA"):
        W.warp_volume(torch.zeros(4, 4, 4), np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="CUDA"):
        W.intensity_augment(torch.zeros(2, 4))


def test_library_rejects_before_any_launch():
    fake = 0x10000
    job = np.zeros(1, dtype=W._WARP_JOB_DTYPE)
    job["X"], job["Y"], job["Z"], job["elastic"] = 4, 4, 4, 1
    with pytest.raises(_lib.DyconLibraryError, match="elastic needs warp"):
        _lib.call("dycon_assemble_batch_warp", fake, fake, job.ctypes.data, 1, None, 4, 4, 4, fake, fake, 1, None, 0, 0, None)
    job["elastic"], job["warp"], job["m"][0, 0] = 0, 1, np.inf
    with pytest.raises(_lib.DyconLibraryError, match="NaN or an infinity"):
        _lib.call("dycon_assemble_batch_warp", fake, fake, job.ctypes.data, 1, None, 4, 4, 4, fake, fake, 1, None, 0, 0, None)
    m, off = np.eye(3).reshape(9), np.zeros(3)
    with pytest.raises(_lib.DyconLibraryError, match="order"):
        _lib.call("dycon_warp_volume", fake, 4, 4, 4, fake, 4, 4, 4, 2, 4, m.ctypes.data, off.ctypes.data, None, None)
    with pytest.raises(_lib.DyconLibraryError, match="bytes"):
        _lib.call("dycon_warp_volume", fake, 4, 4, 4, fake, 4, 4, 4, 1, 1, m.ctypes.data, off.ctypes.data, None, None)
    par = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    with pytest.raises(_lib.DyconLibraryError, match="lo < hi"):
        _lib.call("dycon_intensity_augment", fake, fake, 64, None, par.ctypes.data, 1, None)
    assert W._WARP_JOB_DTYPE.itemsize == 152      # sizeof(dycon_warp_job_t)
