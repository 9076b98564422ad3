"""Host side of the device-resident data path (dataloaders/device_cache.py): the plan draws consume np.random as the transform chain
does, the numpy twin of the kernel equals the chain bit for bit, the cache validates what it stores, the loader's plan sequence
interleaves with the batch samplers as a DataLoader(num_workers=0) does.  Yardstick: the numpy transforms of dataloaders/brats19.py
(tests/device_cache_ref.py); every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import device_cache_ref as R
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.dataloaders import (PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, apply_plan_host, draw_plan)
from dycon_paper_replication_amd.dataloaders import device_cache as DC
from dycon_paper_replication_amd.dataloaders.brats19 import SagittalToAxial, TwoStreamBatchSampler
from dycon_paper_replication_amd.dataloaders.isles22 import ThreeStreamBatchSampler

# (6, 11, 9) under (8, 8, 6): one short axis pads ALL three, by 4, 1 and 1 voxels per side; (8, 12, 10): `<=`, an equal axis pads too
CONFIGS = {
    "p886": ((8, 8, 6), [(13, 11, 9), (20, 17, 16), (6, 11, 9), (8, 12, 10)]),
    "p885": ((8, 8, 5), [(13, 11, 9), (20, 17, 16)]),
}


def _cache_arrays(cases, pre=None):
    c = DeviceVolumeCache(cases, device="cpu", pre=pre)
    return c, [c.host_case(i)[0] for i in range(len(c))], [c.host_case(i)[1] for i in range(len(c))]


def test_pad_rule_of_the_short_case():
    assert DC._pads((6, 11, 9), (8, 8, 6)) == (4, 1, 1)
    assert DC._pads((8, 12, 10), (8, 8, 6)) == (3, 1, 1)
    assert DC._pads((13, 11, 9), (8, 8, 6)) == (0, 0, 0)


@pytest.mark.parametrize("sagittal", [False, True], ids=["plain", "brats"])
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_plan_draws_and_host_twin_equal_the_chain(cfg, sagittal):
    patch, shapes = CONFIGS[cfg]
    cases = R.make_cases(shapes, 11, image_dtype=np.float32 if sagittal else np.float64, sagittal=sagittal)
    cache, images, labels = _cache_arrays(cases, pre=SagittalToAxial() if sagittal else None)
    assert cache.shapes == [tuple(s) for s in shapes]
    tf = R.chain(patch, sagittal=sagittal)
    indices = list(range(len(cases))) + [1, 0]
    seen, padded = set(), False
    for seed in range(200):
        np.random.seed(seed)
        ref_i, ref_l = R.chain_batch(cases, indices, tf)
        ref_state = np.random.get_state()
        np.random.seed(seed)
        plan = draw_plan(cache.shapes, indices, patch)
        assert R.same_state(np.random.get_state(), ref_state)              # the same number of draws with the same bounds
        got = apply_plan_host(plan, images, labels)
        assert got["image"].dtype == np.float32 and got["label"].dtype == np.uint8
        assert np.array_equal(got["image"], ref_i) and np.array_equal(got["label"], ref_l)
        seen |= {(int(k), int(a)) for k, a in zip(plan["k"], plan["flip_axis"])}
        padded |= bool((plan["origin"] < 0).any())
        if len(seen) == 8 and seed >= 3:
            break
    assert seen == {(k, a) for k in range(4) for a in range(2)}
    assert padded == (cfg == "p886")                                         # the pad region was actually sampled


def test_rot_flip_off_draws_the_crop_only():
    patch, shapes = CONFIGS["p886"]
    cases = R.make_cases(shapes, 12)
    cache, images, labels = _cache_arrays(cases)
    np.random.seed(5)
    ref_i, ref_l = R.chain_batch(cases, [2, 0, 3, 1], R.chain(patch, rot_flip=False))
    ref_state = np.random.get_state()
    np.random.seed(5)
    plan = draw_plan(cache.shapes, [2, 0, 3, 1], patch, rot_flip=False)
    assert R.same_state(np.random.get_state(), ref_state)
    assert (plan["k"] == 0).all() and (plan["flip_axis"] == -1).all()
    got = apply_plan_host(plan, images, labels)
    assert np.array_equal(got["image"], ref_i) and np.array_equal(got["label"], ref_l)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_center_plan_equals_center_crop_and_draws_nothing(cfg):
    patch, shapes = CONFIGS[cfg]
    cases = R.make_cases(shapes, 13)
    cache, images, labels = _cache_arrays(cases)
    indices = list(range(len(cases)))
    ref_i, ref_l = R.chain_batch(cases, indices, R.chain(patch, center=True))
    np.random.seed(3)
    before = np.random.get_state()
    plan = draw_plan(cache.shapes, indices, patch, center=True)
    assert R.same_state(np.random.get_state(), before)
    got = apply_plan_host(plan, images, labels)
    assert np.array_equal(got["image"], ref_i) and np.array_equal(got["label"], ref_l)


def test_odd_k_needs_a_square_patch():
    cases = R.make_cases([(13, 11, 9)], 14)
    cache, images, labels = _cache_arrays(cases)
    plan = np.zeros(1, dtype=PLAN_DTYPE)
    plan[0] = (0, (0, 0, 0), 1, 0, (8, 6, 5))
    with pytest.raises(ValueError):
        apply_plan_host(plan, images, labels)
    plan["k"] = 2                                                            # an even k keeps the shape
    assert apply_plan_host(plan, images, labels)["image"].shape == (1, 1, 8, 6, 5)
    with pytest.raises(ValueError):                                          # over enough draws an odd k comes up
        for seed in range(50):
            np.random.seed(seed)
            draw_plan(cache.shapes, [0, 0], (8, 6, 5))


def test_library_rejects_bad_jobs_before_any_launch():
    """the argument checks of dycon_assemble_batch return before the first HIP call: testable without a device"""
    lib = _lib.load()
    job = np.zeros(17, dtype=DC._JOB_DTYPE)
    assert DC._JOB_DTYPE.itemsize == 48
    job["X"], job["Y"], job["Z"] = 13, 11, 9
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def rc(njobs=1, patch=(8, 8, 6), lb=1, **kw):
        j = job.copy()
        for k, v in kw.items():
            j[k] = v
        return lib.dycon_assemble_batch(p, p, j.ctypes.data, njobs, *patch, p, p, lb, None)

    for bad in (dict(njobs=0), dict(njobs=17), dict(patch=(8, 0, 6)), dict(patch=(8, 8, -1)), dict(k=4), dict(k=-1), dict(flip_axis=2),
                dict(flip_axis=-2), dict(patch=(8, 6, 5), k=1), dict(patch=(8, 6, 5), k=3), dict(lb=4), dict(X=0)):
        assert rc(**bad) == -22, bad
        assert b"assemble_batch" in lib.dycon_last_error()


def test_cache_validates_labels_and_layout():
    img = np.zeros((5, 4, 3), dtype=np.float32)
    ok = np.arange(60).reshape(5, 4, 3) % 3
    for lab in (ok.astype(np.int64), ok.astype(np.float64), ok.astype(np.int8), (ok > 0)):       # ISLES: a float64 mask
        c = DeviceVolumeCache([{"image": img, "label": lab}], device="cpu")
        assert np.array_equal(c.host_case(0)[1], lab.astype(np.uint8))
    for bad in (ok + 254, ok - 1, ok * 0.5, np.where(ok > 1, np.nan, 0.0), ok.astype(str)):
        with pytest.raises(ValueError):
            DeviceVolumeCache([{"image": img, "label": bad}], device="cpu")
    with pytest.raises(ValueError):
        DeviceVolumeCache([{"image": img, "label": ok[:4]}], device="cpu")
    with pytest.raises(ValueError):
        DeviceVolumeCache([], device="cpu")
    # layout: 16-byte-aligned case offsets in both arenas, fp32 / uint8 storage, nbytes = the two arenas
    cases = R.make_cases([(5, 3, 3), (7, 3, 1), (2, 2, 2)], 15, image_dtype=np.float64)
    c = DeviceVolumeCache(cases, device="cpu")
    assert len(c) == 3 and c.shapes == [(5, 3, 3), (7, 3, 1), (2, 2, 2)]
    assert list(c._img_off) == [0, 48, 72] and list(c._lab_off) == [0, 48, 80]
    assert c.images.dtype == torch.float32 and c.labels.dtype == torch.uint8
    assert c.nbytes == 4 * c.images.numel() + c.labels.numel() == 4 * 80 + 96
    for i, s in enumerate(cases):
        assert np.array_equal(c.host_case(i)[0], s["image"].astype(np.float32)) and np.array_equal(c.host_case(i)[1], s["label"])
    d = DeviceVolumeCache(R.MemDataset(cases, transform=None), device="cpu")          # a map-style dataset without a transform qualifies
    assert d.shapes == c.shapes and torch.equal(d.images, c.images) and torch.equal(d.labels, c.labels)


def test_max_bytes_raises_before_allocation(monkeypatch):
    cases = R.make_cases([(5, 3, 3), (7, 3, 1)], 16)

    def no_alloc(*a, **k):
        raise AssertionError("allocated before the max_bytes check")
    monkeypatch.setattr(torch, "zeros", no_alloc)
    with pytest.raises(ValueError):
        DeviceVolumeCache(cases, device="cuda:0", max_bytes=4 * 72 + 80 - 1)
    monkeypatch.undo()
    assert DeviceVolumeCache(cases, device="cpu", max_bytes=4 * 72 + 80).nbytes == 4 * 72 + 80


@pytest.mark.parametrize("kind", ["two", "three"])
def test_loader_plans_interleave_with_the_sampler_like_a_dataloader(kind):
    """two epochs: the plans the loader's host side draws name the same cases and the same crops as DataLoader(num_workers=0) over
    the dataset with the transform chain (the volumes are random, so equal batches mean equal cases, crops, rotations and flips)"""
    patch = (8, 8, 6)
    shapes = [(13, 11, 9), (20, 17, 16), (6, 11, 9), (12, 12, 12), (9, 14, 10), (15, 10, 8), (8, 12, 10), (11, 11, 11), (14, 9, 9), (10, 13, 7)]
    cases = R.make_cases(shapes, 17)
    cache, images, labels = _cache_arrays(cases)
    Sampler = TwoStreamBatchSampler if kind == "two" else ThreeStreamBatchSampler
    sampler = Sampler(list(range(4)), list(range(4, 10)), 4, 2)
    np.random.seed(1337)
    ref = R.dataloader_batches(cases, R.chain(patch), sampler, epochs=2)
    ref_state = np.random.get_state()
    loader = DeviceBatchLoader(cache, sampler, patch)
    np.random.seed(1337)
    plans = [p for _ in range(2) for p in loader.plans()]
    assert R.same_state(np.random.get_state(), ref_state)
    assert len(plans) == len(ref) == 2 * len(loader) == 4
    for plan, (ref_i, ref_l) in zip(plans, ref):
        assert len(plan) == (4 if kind == "two" else 6)
        got = apply_plan_host(plan, images, labels)
        assert np.array_equal(got["image"], ref_i) and np.array_equal(got["label"], ref_l)
