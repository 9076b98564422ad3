"""Shared by test_augment_cpu.py / test_augment_gpu.py: the yardstick -- this package's host transforms chained with RandomRot in
front (dataloaders/isles22.py: scipy.ndimage.rotate itself, np.pad, np.rot90, np.flip), which share no code with the plan, the
numpy twin or the kernel -- and the conditions that keep a comparison from passing on zeros."""
import numpy as np
import torch
from torch.utils.data import DataLoader

import device_cache_ref as R
from dycon_paper_replication_amd.dataloaders import isles22 as D

ORDERS = ("crop_rotflip", "rotflip_crop")
SMALL = [(13, 11, 9), (20, 17, 16), (6, 11, 9)]          # (6, 11, 9) under (8, 8, 6): padded by 4, 1, 1 per side
SMALL_PATCHES = [(8, 8, 6), (8, 8, 5)]


def small_shapes(patch):
    """the five small shape / patch pairs: all three cases under (8, 8, 6), the two unpadded ones under (8, 8, 5)"""
    return SMALL if tuple(patch) == (8, 8, 6) else SMALL[:2]


def chain_rot(patch, order="crop_rotflip", onehot=None):
    """RandomRot in front of either training pipeline, CreateOnehotLabel(onehot) in front of ToTensor when asked"""
    mid = [D.RandomCrop(patch), D.RandomRotFlip()] if order == "crop_rotflip" else [D.RandomRotFlip(), D.RandomCrop(patch)]
    return R.Compose([D.RandomRot()] + mid + ([D.CreateOnehotLabel(onehot)] if onehot else []) + [D.ToTensor()])


def chain_rot_batch(cases, indices, tf):
    """-> image (B, 1, w, h, d) float32, label (B, w, h, d) int64, onehot (B, C, w, h, d) int64 or None (numpy)"""
    outs = [tf(dict(cases[i])) for i in indices]
    hot = torch.stack([o["onehot_label"] for o in outs]).numpy() if "onehot_label" in outs[0] else None
    return torch.stack([o["image"] for o in outs]).numpy(), torch.stack([o["label"] for o in outs]).numpy(), hot


def dataloader_batches_rot(cases, tf, sampler, epochs):
    """[{key: numpy}] of `epochs` passes of DataLoader(num_workers=0) over the dataset with the transform chain"""
    dl = DataLoader(R.MemDataset(cases, tf), batch_sampler=sampler, num_workers=0)
    return [{k: v.numpy() for k, v in b.items()} for _ in range(epochs) for b in dl]


def larger_than(shape, patch):
    return all(s > p for s, p in zip(shape, patch))


def check_not_trivial(twin, plan, shapes, min_fill=0.75, rotation_zero=True):
    """The conditions on a batch (from the twin's output): every sample of a case larger than the patch is at least `min_fill`
    non-zero, and (rotation_zero) the batch holds a voxel inside the rotated volume whose source fell outside -- a zero made by
    the rotation, not by the pad.  -> the number of such voxels"""
    patch = tuple(int(v) for v in plan["patch"][0])
    for n, rec in enumerate(plan):
        if larger_than(shapes[int(rec["case"])], patch):
            fill = np.count_nonzero(twin["image"][n]) / twin["image"][n].size
            assert fill >= min_fill, (n, fill)
    made = int(np.count_nonzero(twin["in_volume"] & ~twin["in_source"]))
    assert made > 0 or not rotation_zero
    return made
