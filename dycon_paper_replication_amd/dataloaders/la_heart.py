"""Left-atrium (LA, 2018 Atrial Segmentation Challenge) data path with the reference's names (code/dataloaders/la_heart.py).

    LAHeart(base_dir, split, num, transform)       :91-126   `<base_dir>/train.list|test.list`, `<base_dir>/LA_data/<case>/mri_norm2.h5`
    BaseDataSets(base_dir, split, num, transform)  :15-50    the 2-D slice dataset the module carries along
    random_rot_flip, random_rotate, RandomGenerator          :52-88
    Resize, CenterCrop, RandomCrop(with_sdf), RandomRotFlip, RandomRot, RandomNoise, CreateOnehotLabel, ToTensor   :128-277
    TwoStreamBatchSampler, ThreeStreamBatchSampler, iterate_once, iterate_eternally, grouper                         :280-355

The transform classes and samplers are the ones of dataloaders/brats19.py, pancreas.py and isles22.py: the reference's four loader
modules repeat them with the same ``np.random`` call order (RandomRotFlip: k, then the axis; RandomCrop: three offsets from the padded
shape), so they are re-exported, not restated.  The LA pipelines apply ``RandomRotFlip()`` BEFORE ``RandomCrop(patch)``;
``DeviceBatchLoader(..., order="rotflip_crop")`` (dataloaders/device_cache.py) draws in that order.  h5py, scikit-image and
scipy.ndimage are imported when first needed.  Parity unpinned (see pancreas.py): the reference module cannot be imported here; its
names, parameters and defaults are pinned by tests/golden/test_3d_patch_api.json.
"""
from __future__ import annotations

import itertools
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset

from .brats19 import CenterCrop, RandomCrop, RandomNoise, RandomRotFlip, TwoStreamBatchSampler   # noqa: F401  (re-exported)
from .isles22 import RandomRot, ThreeStreamBatchSampler                                          # noqa: F401
from .pancreas import CreateOnehotLabel, Resize, ToTensor                                       # noqa: F401


class BaseDataSets(Dataset):
    """:15-50 -- `<base_dir>/train_slices.list` with `<base_dir>/data/slices/<case>.h5` (split 'train', transformed) or
    `<base_dir>/val.list` with `<base_dir>/data/<case>.h5` (split 'val'); `num` truncates the training list; samples carry 'case'"""

    def __init__(self, base_dir=None, split="train", num=None, transform=None):
        self._base_dir = base_dir
        self.sample_list = []
        self.split = split
        self.transform = transform
        name = {"train": "/train_slices.list", "val": "/val.list"}.get(split)
        if name is not None:
            with open(self._base_dir + name, "r") as f:
                self.sample_list = [item.replace("\n", "") for item in f.readlines()]
        if num is not None and self.split == "train":
            self.sample_list = self.sample_list[:num]

    def __len__(self):
        return len(self.sample_list)

    def __getitem__(self, idx):
        import h5py   # lazy: absent in the build image
        case = self.sample_list[idx]
        path = "/data/slices/{}.h5" if self.split == "train" else "/data/{}.h5"
        with h5py.File(self._base_dir + path.format(case), "r") as h5f:
            sample = {"image": h5f["image"][:], "label": h5f["label"][:]}
        if self.split == "train":
            sample = self.transform(sample)
        sample["case"] = case
        return sample


def random_rot_flip(image, label):
    """:52-59 -- np.rot90(k) then a flip of axis 0 or 1; draws k, then the axis"""
    k = np.random.randint(0, 4)
    image, label = np.rot90(image, k), np.rot90(label, k)
    axis = np.random.randint(0, 2)
    return np.flip(image, axis=axis).copy(), np.flip(label, axis=axis).copy()


def random_rotate(image, label):
    """:62-66 -- rotation by np.random.randint(-20, 20) degrees, nearest neighbour, shape kept"""
    from scipy import ndimage
    angle = np.random.randint(-20, 20)
    return ndimage.rotate(image, angle, order=0, reshape=False), ndimage.rotate(label, angle, order=0, reshape=False)


class RandomGenerator(object):
    """:69-88 -- the 2-D slice augmentation: rot/flip or a rotation by ``random.random()``, then a nearest-neighbour zoom to
    output_size; image -> (1, x, y) float32 tensor, label -> uint8 tensor"""

    def __init__(self, output_size):
        self.output_size = output_size

    def __call__(self, sample):
        from scipy.ndimage import zoom
        image, label = sample["image"], sample["label"]
        if random.random() > 0.5:
            image, label = random_rot_flip(image, label)
        elif random.random() > 0.5:
            image, label = random_rotate(image, label)
        x, y = image.shape
        image = zoom(image, (self.output_size[0] / x, self.output_size[1] / y), order=0)
        label = zoom(label, (self.output_size[0] / x, self.output_size[1] / y), order=0)
        return {"image": torch.from_numpy(image.astype(np.float32)).unsqueeze(0), "label": torch.from_numpy(label.astype(np.uint8))}


class LAHeart(Dataset):
    """:91-126 -- 'test' and 'val' share test.list; `num` truncates either list"""

    def __init__(self, base_dir=None, split="train", num=None, transform=None):
        self._base_dir = base_dir
        self.transform = transform
        self.sample_list = []
        path = self._base_dir + ("/train.list" if split == "train" else "/test.list")
        with open(path, "r") as f:
            self.image_list = [item.replace("\n", "") for item in f.readlines()]
        if num is not None:
            self.image_list = self.image_list[:num]

    def __len__(self):
        return len(self.image_list)

    def __getitem__(self, idx):
        import h5py   # lazy: absent in the build image
        with h5py.File(os.path.join(self._base_dir, "LA_data", self.image_list[idx], "mri_norm2.h5"), "r") as h5f:
            sample = {"image": h5f["image"][:], "label": h5f["label"][:]}
        return self.transform(sample) if self.transform else sample


def iterate_once(iterable):
    return np.random.permutation(iterable)


def iterate_eternally(indices):
    def infinite_shuffles():
        while True:
            yield np.random.permutation(indices)
    return itertools.chain.from_iterable(infinite_shuffles())


def grouper(iterable, n):
    """grouper('ABCDEFG', 3) --> ABC DEF"""
    args = [iter(iterable)] * n
    return zip(*args)
