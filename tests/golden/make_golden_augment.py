#!/usr/bin/env python3
"""Golden fixture of the reference's loader transforms with RandomRot in the chain (code/dataloaders/isles22.py:24-28, :143-247) by
IMPORTING that module on the CPU (the stub-module recipe of make_golden_preprocess.py).  It imports h5py and skimage.transform at
the top, neither of which is installed and neither of which the transforms used here touch: empty stand-ins go into sys.modules.

Runs, for both orders and seeds 0..7, ``np.random.seed(seed)`` and then the chain over the three cases in turn:
    crop_rotflip   RandomRot() -> RandomCrop(PATCH) -> RandomRotFlip() -> CreateOnehotLabel(CLASSES) -> ToTensor()
    rotflip_crop   RandomRot() -> RandomRotFlip() -> RandomCrop(PATCH) -> CreateOnehotLabel(CLASSES) -> ToTensor()
Cases: shapes (13, 11, 9), (20, 17, 16) and (6, 11, 9) (the last one is padded under PATCH = (8, 8, 6)), images standard normal
kept to half precision's digits (so that the file compresses), labels 0..3 with CLASSES = 3: label 3 sets no one-hot plane.

Stores data only (augment.npz):
  case_seed, seeds, patch, classes, orders       the generating parameters
  case<i>.image (float32), case<i>.label (uint8) the case arrays
  <order>.image   (8, 3, 1, 8, 8, 6) float32     ToTensor's image per seed and case
  <order>.label   (8, 3, 8, 8, 6) uint8          ToTensor's label (int64 there; the values fit)
  <order>.onehot  (8, 3, CLASSES, 8, 8, 6) uint8 ToTensor's onehot_label (int64 there)
  <order>.state   (8, 8) uint32                  the first 8 words of np.random.get_state()[1] after the three cases

    python tests/golden/make_golden_augment.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/code"

h5py, skimage, sk_transform = types.ModuleType("h5py"), types.ModuleType("skimage"), types.ModuleType("skimage.transform")
skimage.transform = sk_transform
sys.modules.update({"h5py": h5py, "skimage": skimage, "skimage.transform": sk_transform})
sys.path.insert(0, REF)
ref = importlib.import_module("dataloaders.isles22")

CASE_SEED, SEEDS, PATCH, CLASSES = 31, list(range(8)), (8, 8, 6), 3
SHAPES = [(13, 11, 9), (20, 17, 16), (6, 11, 9)]
ORDERS = ("crop_rotflip", "rotflip_crop")

rng = np.random.default_rng(CASE_SEED)
cases = [{"image": rng.standard_normal(s).astype(np.float16).astype(np.float32), "label": rng.integers(0, 4, s).astype(np.uint8)}
         for s in SHAPES]


def chain(order):
    mid = [ref.RandomCrop(PATCH), ref.RandomRotFlip()] if order == "crop_rotflip" else [ref.RandomRotFlip(), ref.RandomCrop(PATCH)]
    return [ref.RandomRot()] + mid + [ref.CreateOnehotLabel(CLASSES), ref.ToTensor()]


out = {"case_seed": np.int64(CASE_SEED), "seeds": np.asarray(SEEDS), "patch": np.asarray(PATCH), "classes": np.int64(CLASSES),
       "orders": np.array(ORDERS)}
for n, c in enumerate(cases):
    out[f"case{n}.image"], out[f"case{n}.label"] = c["image"], c["label"]
for order in ORDERS:
    images, labels, onehots, states = [], [], [], []
    for seed in SEEDS:
        np.random.seed(seed)
        res = []
        for c in cases:
            s = dict(c)
            for t in chain(order):
                s = t(s)
            res.append(s)
        images.append(np.stack([r["image"].numpy() for r in res]))
        labels.append(np.stack([r["label"].numpy() for r in res]))
        onehots.append(np.stack([r["onehot_label"].numpy() for r in res]))
        states.append(np.random.get_state()[1][:8].copy())
    assert images[0].dtype == np.float32 and labels[0].dtype == np.int64 and onehots[0].dtype == np.int64
    assert max(int(a.max()) for a in labels) == 3 and min(int(a.min()) for a in labels) == 0
    out[f"{order}.image"] = np.stack(images)
    out[f"{order}.label"] = np.stack(labels).astype(np.uint8)
    out[f"{order}.onehot"] = np.stack(onehots).astype(np.uint8)
    out[f"{order}.state"] = np.stack(states).astype(np.uint32)

path = os.path.join(HERE, "augment.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path))
