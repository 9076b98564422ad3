"""dataloaders/device_augment.py on the host: the rotation restated against scipy itself, draw_plan_rot and the numpy twin against
the transform chain with RandomRot in front (tests/augment_ref.py) and against the reference's own classes (tests/golden/
augment.npz), the one-hot planes, malformed plans, the library's argument checks, and the untouched default path."""
import ctypes

import numpy as np
import pytest
import torch
from scipy import ndimage

import augment_ref as A
import device_cache_ref as R
from conftest import load_golden
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.dataloaders import (PLAN_DTYPE, ROT_PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, apply_plan_host,
                                                     apply_rot_plan_host, draw_plan, draw_plan_rot, rotation_of)
from dycon_paper_replication_amd.dataloaders import device_augment as DA
from dycon_paper_replication_amd.dataloaders.brats19 import TwoStreamBatchSampler
from dycon_paper_replication_amd.dataloaders.pancreas import CreateOnehotLabel

ANGLES = range(-20, 20)


@pytest.mark.parametrize("dtype", [np.float32, np.uint8], ids=["f32", "u8"])
@pytest.mark.parametrize("shape", [(7, 5, 3), (13, 9, 2), (12, 12, 2), (40, 33, 2)], ids=lambda s: "x".join(map(str, s)))
def test_rotation_restated_equals_scipy(shape, dtype):
    """rotation_of + the twin's coordinate code against ndimage.rotate, every angle RandomRot can draw"""
    rng = np.random.default_rng(3)
    a = rng.standard_normal(shape).astype(dtype) if dtype == np.float32 else rng.integers(1, 256, shape).astype(dtype)
    cut = 0
    for angle in ANGLES:
        m, off = rotation_of(angle, shape)
        assert m.dtype == np.float64 and m.shape == (2, 2) and off.dtype == np.float64 and off.shape == (2,)
        got = DA.rotate_nearest_host(a, m, off)
        ref = ndimage.rotate(a, angle, order=0, reshape=False)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), angle
        cut += int(np.count_nonzero(got == 0))
    assert cut > 0                                                   # corners did leave the volume


def _cache(cases):
    c = DeviceVolumeCache(cases, device="cpu")
    host = [c.host_case(i) for i in range(len(c))]
    return c, [h[0] for h in host], [h[1] for h in host]


@pytest.mark.parametrize("patch", A.SMALL_PATCHES, ids=["p886", "p885"])
@pytest.mark.parametrize("order", A.ORDERS)
def test_plan_draws_and_host_twin_equal_the_chain(order, patch):
    """seeds 0..39 over the five small shape / patch pairs (the padded case included): images, labels and the np.random end state"""
    shapes = A.small_shapes(patch)
    cases = R.make_cases(shapes, 41, image_dtype=np.float64)
    cache, images, labels = _cache(cases)
    indices = list(range(len(cases))) + [0]
    angles, made = set(), 0
    for seed in range(40):
        np.random.seed(seed)
        ref_i, ref_l, _ = A.chain_rot_batch(cases, indices, A.chain_rot(patch, order))
        ref_state = np.random.get_state()
        np.random.seed(seed)
        plan = draw_plan_rot(cache.shapes, indices, patch, order=order)
        assert R.same_state(np.random.get_state(), ref_state)
        assert plan.dtype == ROT_PLAN_DTYPE
        got = apply_rot_plan_host(plan, images, labels)
        assert got["image"].dtype == np.float32 and got["label"].dtype == np.uint8
        assert np.array_equal(got["image"], ref_i) and np.array_equal(got["label"], ref_l)
        made += A.check_not_trivial(got, plan, cache.shapes, rotation_zero=False)     # four small crops: not every batch has one
        angles |= {int(a) for a in plan["angle"]}
    assert len(angles) >= 30 and min(angles) >= -20 and max(angles) <= 19 and made > 0


def test_plan_is_the_angle_then_draw_plan():
    """the angle first, then exactly what draw_plan draws; the rotation fields are rotation_of's"""
    shapes = A.SMALL
    for order in A.ORDERS:
        for seed in range(10):
            np.random.seed(seed)
            rp = draw_plan_rot(shapes, [1], (8, 8, 6), order=order)
            np.random.seed(seed)
            angle = np.random.randint(-20, 20)
            p = draw_plan(shapes, [1], (8, 8, 6), order=order)
            for f in PLAN_DTYPE.names:
                assert np.array_equal(rp[f], p[f])
            m, off = rotation_of(angle, shapes[1])
            assert rp["angle"][0] == angle and np.array_equal(rp["m"][0], m.reshape(4)) and np.array_equal(rp["off"][0], off)
    np.random.seed(0)
    assert set(draw_plan_rot(shapes, [0] * 50, (8, 8, 6), angle_range=(3, 5))["angle"]) == {3, 4}


def test_host_twin_equals_the_reference_golden():
    """the reference's own RandomRot / RandomCrop / RandomRotFlip / CreateOnehotLabel / ToTensor (make_golden_augment.py)"""
    g = load_golden("augment")
    patch, C = tuple(int(v) for v in g["patch"]), int(g["classes"])
    images, labels = [g[f"case{n}.image"] for n in range(3)], [g[f"case{n}.label"] for n in range(3)]
    shapes = [a.shape for a in images]
    for order in g["orders"]:
        for s, seed in enumerate(g["seeds"]):
            np.random.seed(int(seed))
            plan = draw_plan_rot(shapes, [0, 1, 2], patch, order=str(order))
            assert np.array_equal(np.random.get_state()[1][:8], g[f"{order}.state"][s])
            got = apply_rot_plan_host(plan, images, labels, onehot=C)
            assert np.array_equal(got["image"], g[f"{order}.image"][s])
            assert np.array_equal(got["label"], g[f"{order}.label"][s])
            assert np.array_equal(got["onehot_label"], g[f"{order}.onehot"][s])
    assert g["crop_rotflip.label"].max() == 3 >= C                   # a label without a plane went through


@pytest.mark.parametrize("C", [2, 4])
def test_onehot_planes_equal_create_onehot_label(C):
    cases = R.make_cases(A.SMALL, 42, nlabels=4)
    cache, images, labels = _cache(cases)
    np.random.seed(5)
    plan = draw_plan_rot(cache.shapes, [0, 1, 2, 1], (8, 8, 6))
    got = apply_rot_plan_host(plan, images, labels, onehot=C)
    assert got["onehot_label"].shape == (4, C, 8, 8, 6) and got["onehot_label"].dtype == np.uint8
    for n in range(4):
        ref = CreateOnehotLabel(C)({"image": got["image"][n, 0], "label": got["label"][n]})["onehot_label"]
        assert np.array_equal(got["onehot_label"][n], ref.astype(np.uint8))
    if C == 2:
        assert (got["label"] >= C).any() and (got["onehot_label"].sum(axis=1) == 0).any()     # a label >= C sets no plane
    else:
        assert (got["onehot_label"].sum(axis=1) == 1).all()


def test_malformed_plans_raise():
    cases = R.make_cases(A.SMALL, 43)
    cache, images, labels = _cache(cases)
    np.random.seed(1)
    good = draw_plan_rot(cache.shapes, [0, 1], (8, 8, 6))
    apply_rot_plan_host(good, images, labels)

    def bad(**kw):
        p = good.copy()
        for k, v in kw.items():
            p[k][1] = v
        return p

    for p in (bad(case=3), bad(case=-1), bad(k=4), bad(flip_axis=2), bad(patch=(8, 8, 5)), bad(m=(np.nan, 0, 0, 1)),
              bad(off=(np.inf, 0)), good[:0], good.reshape(1, 2), good[list(good.dtype.names[:-1])]):      # the last: a record without `off`
        with pytest.raises(ValueError):
            apply_rot_plan_host(p, images, labels)
    for onehot in (0, 9, 2.0, "2"):
        with pytest.raises(ValueError):
            apply_rot_plan_host(good, images, labels, onehot=onehot)
    odd = bad(k=1)
    odd["patch"] = (8, 6, 5)
    with pytest.raises(ValueError):
        apply_rot_plan_host(odd, images, labels)
    for kw in (dict(patch_size=(8, 8)), dict(patch_size=(8, 0, 6)), dict(order="crop"), dict(order="rotflip_crop", rot_flip=False),
               dict(angle_range=(5, 5))):
        with pytest.raises(ValueError):
            draw_plan_rot(cache.shapes, [0], **{"patch_size": (8, 8, 6), **kw})
    with pytest.raises(_lib.DyconLibraryError):                      # no host fallback
        DA.assemble_batch_rot(cache, good)
    with pytest.raises(ValueError):
        DA.rotate_nearest(torch.zeros(3, 3, 3), 5)                   # a host tensor


def test_library_rejects_bad_arguments_before_any_launch():
    """the argument checks of the two entry points return before the first HIP call: testable without a device"""
    lib = _lib.load()
    assert DA._ROT_JOB_DTYPE.itemsize == 104
    job = np.zeros(17, dtype=DA._ROT_JOB_DTYPE)
    job["X"], job["Y"], job["Z"], job["rotate"] = 13, 11, 9, 1
    job["m"] = (1, 0, 0, 1)
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def rc(njobs=1, patch=(8, 8, 6), lb=1, hot=None, C=0, hb=0, **kw):
        j = job.copy()
        for k, v in kw.items():
            j[k] = v
        return lib.dycon_assemble_batch_rot(p, p, j.ctypes.data, njobs, *patch, p, p, lb, hot, C, hb, None)

    for bad in (dict(njobs=0), dict(njobs=17), dict(patch=(8, 0, 6)), dict(k=4), dict(flip_axis=-2), dict(patch=(8, 6, 5), k=1),
                dict(lb=4), dict(X=0), dict(m=(np.nan, 0, 0, 1)), dict(off=(0, -np.inf)), dict(hot=p, C=0, hb=8), dict(hot=p, C=9, hb=8),
                dict(hot=p, C=2, hb=2)):
        assert rc(**bad) == -22, bad
        assert b"assemble_batch_rot" in lib.dycon_last_error()

    m, off = (ctypes.c_double * 4)(1, 0, 0, 1), (ctypes.c_double * 2)(0, 0)
    nan = (ctypes.c_double * 4)(float("nan"), 0, 0, 1)
    for args in ((p, p + 32, 2, 2, 2, 2, m, off), (p, p + 32, 4, 0, 2, 2, m, off), (p, p + 32, 4, 2, 2, 2, nan, off),
                 (p, p + 8, 4, 2, 2, 2, m, off), (p, None, 4, 2, 2, 2, m, off), (p, p + 32, 4, 2, 2, 2, None, off)):
        assert lib.dycon_rotate_nearest(*args, None) == -22, args
        assert b"rotate_nearest" in lib.dycon_last_error()


def test_defaults_leave_the_plans_as_they_were():
    """rot=False, onehot=None: the loader's plans are draw_plan's, record for record, and a PLAN_DTYPE plan through the twin is
    apply_plan_host's batch"""
    cases = R.make_cases(A.SMALL + [(12, 12, 12), (9, 14, 10)], 44)
    cache, images, labels = _cache(cases)
    sampler = TwoStreamBatchSampler([0, 1], [2, 3, 4], 3, 2)
    np.random.seed(9)
    got = list(DeviceBatchLoader(cache, sampler, (8, 8, 6)).plans())
    state = np.random.get_state()
    np.random.seed(9)
    ref = [draw_plan(cache.shapes, [int(i) for i in b], (8, 8, 6)) for b in sampler]
    assert R.same_state(np.random.get_state(), state)
    assert len(got) == len(ref) == 2
    for a, b in zip(got, ref):
        assert a.dtype == PLAN_DTYPE and np.array_equal(a, b)
        x, y = apply_rot_plan_host(a, images, labels), apply_plan_host(a, images, labels)
        assert np.array_equal(x["image"], y["image"]) and np.array_equal(x["label"], y["label"])
    np.random.seed(9)
    rot = list(DeviceBatchLoader(cache, sampler, (8, 8, 6), rot=True).plans())
    assert all(p.dtype == ROT_PLAN_DTYPE for p in rot) and len(rot) == 2
