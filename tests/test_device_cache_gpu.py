"""dycon_assemble_batch / DeviceBatchLoader on the GPU against the numpy transform chain of dataloaders/brats19.py
(tests/device_cache_ref.py), bit for bit: mixed cases with and without the reference's pad, both label widths, the 16-launch chunking,
the vector store path at odd source offsets, a full-size patch, the whole loader over two epochs, the two-buffer ring and a
trainer fed from the loader."""
import functools

import numpy as np
import pytest
import torch

import device_cache_ref as R
from dycon_paper_replication_amd.dataloaders import DeviceBatchLoader, DeviceVolumeCache, assemble_batch, draw_plan
from dycon_paper_replication_amd.dataloaders.brats19 import SagittalToAxial, TwoStreamBatchSampler
from dycon_paper_replication_amd.dataloaders.isles22 import ThreeStreamBatchSampler

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMALL = [(13, 11, 9), (20, 17, 16), (6, 11, 9)]          # (6, 11, 9) under (8, 8, 6): padded by 4, 1, 1 per side


@functools.lru_cache(maxsize=None)
def _small(patch):
    shapes = SMALL if patch == (8, 8, 6) else SMALL[:2]
    cases = R.make_cases(shapes, 21, image_dtype=np.float64)
    return cases, DeviceVolumeCache(cases, device=DEV)


def _check(cache, cases, indices, patch, seed, label_dtype, tf=None):
    """seeded chain on the host vs seeded plan + one assemble_batch on the device"""
    np.random.seed(seed)
    ref_i, ref_l = R.chain_batch(cases, indices, tf or R.chain(patch))
    np.random.seed(seed)
    plan = draw_plan(cache.shapes, indices, patch)
    out = assemble_batch(cache, plan, label_dtype=label_dtype)
    assert out["image"].dtype == torch.float32 and out["label"].dtype == label_dtype
    assert out["image"].is_contiguous() and out["label"].is_contiguous()
    assert out["image"].device == cache.images.device and out["label"].device == cache.images.device
    assert tuple(out["image"].shape) == ref_i.shape and tuple(out["label"].shape) == ref_l.shape
    assert np.array_equal(out["image"].cpu().numpy(), ref_i)
    assert np.array_equal(out["label"].cpu().numpy(), ref_l.astype(np.uint8 if label_dtype == torch.uint8 else np.int64))
    return plan


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("patch", [(8, 8, 6), (8, 8, 5)], ids=["p886", "p885"])
@pytest.mark.parametrize("B", [5, 18])
def test_assemble_batch_equals_the_chain(B, patch, label_dtype):
    """B = 5 mixes the cases; B = 18 takes two launches (16 + 2).  Element stores: neither 6 nor 5 is a multiple of 4"""
    cases, cache = _small(patch)
    indices = [int(i) for i in np.random.default_rng(B).integers(0, len(cases), B)]
    assert set(indices) == set(range(len(cases)))
    seen = set()
    for seed in (0, 1, 2):
        plan = _check(cache, cases, indices, patch, seed, label_dtype)
        seen |= {(int(k), int(a)) for k, a in zip(plan["k"], plan["flip_axis"])}
    if B == 18:
        assert len(seen) == 8                                   # every rotation with every flip went through the kernel


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
def test_vector_stores_with_odd_source_offsets(label_dtype):
    """patch 16^3 from (40, 33, 21): 16-byte stores, the source runs start at odd oz (and at odd row starts: Z = 21)"""
    cases = R.make_cases([(40, 33, 21), (40, 33, 21)], 22)
    cache = DeviceVolumeCache(cases, device=DEV)
    odd = False
    for seed in range(4):
        plan = _check(cache, cases, [0, 1, 1, 0], (16, 16, 16), seed, label_dtype)
        odd |= bool((plan["origin"][:, 2] % 2 == 1).any())
    assert odd


def test_full_size_patch():
    """96^3, B = 4, from three cases near (128, 120, 110): index width and grid size (3456 blocks' worth of work per launch)"""
    cases = R.make_cases([(128, 120, 110), (126, 121, 109), (130, 118, 111)], 23, nlabels=2)
    cache = DeviceVolumeCache(cases, device=DEV)
    _check(cache, cases, [2, 0, 1, 2], (96, 96, 96), 4, torch.uint8)


def test_a_patch_larger_than_the_case_on_every_axis():
    """all of the output's border comes from the pad that never exists"""
    cases = R.make_cases([(5, 6, 7)], 24)
    cache = DeviceVolumeCache(cases, device=DEV)
    _check(cache, cases, [0, 0, 0], (8, 8, 8), 5, torch.int64)


@pytest.mark.parametrize("variant", ["brats", "plain3"])
def test_loader_equals_dataloader_over_two_epochs(variant):
    """brats: SagittalToAxial in front of the chain / as the cache's `pre`, TwoStreamBatchSampler; plain3: ThreeStreamBatchSampler"""
    patch = (8, 8, 6)
    shapes = [(13, 11, 9), (20, 17, 16), (6, 11, 9), (12, 12, 12), (9, 14, 10), (15, 10, 8), (8, 12, 10), (11, 11, 11)]
    sag = variant == "brats"
    cases = R.make_cases(shapes, 25, sagittal=sag)
    cache = DeviceVolumeCache(cases, device=DEV, pre=SagittalToAxial() if sag else None)
    assert cache.shapes == shapes
    Sampler = TwoStreamBatchSampler if sag else ThreeStreamBatchSampler
    sampler = Sampler(list(range(3)), list(range(3, 8)), 3, 2)
    np.random.seed(99)
    ref = R.dataloader_batches(cases, R.chain(patch, sagittal=sag), sampler, epochs=2)
    ref_state = np.random.get_state()
    loader = DeviceBatchLoader(cache, sampler, patch, label_dtype=torch.int64)
    np.random.seed(99)
    n = 0
    for _ in range(2):
        for b in loader:
            assert b["image"].dtype == torch.float32 and b["label"].dtype == torch.int64
            assert np.array_equal(b["image"].cpu().numpy(), ref[n][0]) and np.array_equal(b["label"].cpu().numpy(), ref[n][1])
            n += 1
    assert n == len(ref) == 2 * len(loader) == 6
    assert R.same_state(np.random.get_state(), ref_state)


def test_ring_keeps_a_batch_until_the_next_but_one():
    cases, cache = _small((8, 8, 6))
    loader = DeviceBatchLoader(cache, TwoStreamBatchSampler([0, 1, 2], [1, 2], 2, 1), (8, 8, 6))      # three batches per epoch
    np.random.seed(7)
    it = iter(loader)
    b0 = next(it)
    keep = {k: v.clone() for k, v in b0.items()}
    b1 = next(it)
    torch.cuda.synchronize()
    assert b1["image"].data_ptr() != b0["image"].data_ptr() and b1["label"].data_ptr() != b0["label"].data_ptr()
    assert torch.equal(b0["image"], keep["image"]) and torch.equal(b0["label"], keep["label"])      # batch n survived batch n + 1
    assert not torch.equal(b1["image"], keep["image"])
    b2 = next(it)
    assert b2["image"].data_ptr() == b0["image"].data_ptr() and b2["label"].data_ptr() == b0["label"].data_ptr()   # n + 2 reuses n's storage


def test_trainer_fed_by_the_loader():
    """five steps of a small V-Net trainer (eager, eager, recorded, replayed, replayed) on loader batches: the tensors handed to
    step() equal the host-built batches of the same seed, every loss is finite, no step is skipped"""
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    patch = (32, 32, 32)
    shapes = [(40, 38, 36), (39, 40, 37), (41, 37, 36), (40, 39, 38), (38, 38, 40), (42, 38, 36), (40, 40, 36), (37, 39, 38)]
    cases = R.make_cases(shapes, 26, nlabels=2)
    cache = DeviceVolumeCache(cases, device=DEV)
    sampler = TwoStreamBatchSampler(list(range(5)), list(range(5, 8)), 2, 1)
    np.random.seed(31)
    ref = R.dataloader_batches(cases, R.chain(patch), sampler, epochs=1)
    assert len(ref) == 5
    tr = DyconTrainer(TrainConfig(model="vnet", labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=3), DEV)
    np.random.seed(31)
    for n, b in enumerate(DeviceBatchLoader(cache, sampler, patch)):
        assert np.array_equal(b["image"].cpu().numpy(), ref[n][0]) and np.array_equal(b["label"].cpu().numpy(), ref[n][1])
        out = tr.step(b["image"], b["label"])
        assert np.isfinite(float(out["loss"])) and not out["skipped"]
    assert n == 4 and tr.iter_num == 5 and tr.skipped_steps == 0 and tr._rp is not None
