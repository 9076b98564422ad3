#!/usr/bin/env python3
"""Golden fixture of the reference's code/utils/util.py by IMPORTING it on the CPU (make_golden_gambling.py's stub-package recipe).
The module cannot be imported as it stands here: it does `import networks` (unused by what is recorded: an empty stand-in), it
imports skimage.segmentation, which is not installed, and compute_sdf spells `np.bool`, which this numpy no longer has
(`np.bool = bool` for the run).  The stand-in for skimage's find_boundaries(mode="inner") is sdf_ref.inner_boundary, a scipy
expression.

Stores data only (sdf.npz):
  sdf.<name>.img_gt, sdf.<name>.out_shape, sdf.<name>.sdf   the masks of sdf_ref.golden_batches() and the reference compute_sdf's
                                                            float64 outputs                        (code/utils/util.py:205-236)
  sampler.indexes         UnifLabelSampler(SAMPLER_N, SAMPLER_LISTS).indexes after np.random.seed(HELPER_SEED)        (:130-161)
  lr.values               the groups' lr after learning_rate_decay(optimizer, t, LR_0), t in LR_STEPS, (steps, groups) (:183-186)
  meter.trace             (val, sum, count, avg) of an AverageMeter after each of METER_UPDATES                       (:164-180)

What this pins: the reference's arithmetic on the two scipy distance transforms -- the order of the operations, the normalisation by
each transform's own minimum and maximum, the zeroing of the boundary, the empty-mask branch, the 0 / 0 of a mask without
background.  What it does not pin: skimage's boundary rule itself, which is restated, not run.

    python tests/golden/make_golden_sdf.py
"""
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/code"

import sdf_ref as R  # noqa: E402

m = types.ModuleType("utils")
m.__path__ = [f"{REF}/utils"]
sys.modules["utils"] = m
sys.modules["networks"] = types.ModuleType("networks")
skimage, seg = types.ModuleType("skimage"), types.ModuleType("skimage.segmentation")


def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
    assert mode == "inner" and connectivity == 1 and background == 0
    return R.inner_boundary(label_img)


seg.find_boundaries = find_boundaries
skimage.segmentation = seg
sys.modules["skimage"], sys.modules["skimage.segmentation"] = skimage, seg
if not hasattr(np, "bool"):
    np.bool = bool
ref = importlib.import_module("utils.util")

out = {}
for name, (img_gt, out_shape) in R.golden_batches().items():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # the 0 / 0 of the sample without background
        sdf = ref.compute_sdf(img_gt, out_shape)
    assert sdf.dtype == np.float64 and sdf.shape == tuple(out_shape)
    out[f"sdf.{name}.img_gt"], out[f"sdf.{name}.out_shape"], out[f"sdf.{name}.sdf"] = img_gt, np.array(out_shape), sdf

np.random.seed(R.HELPER_SEED)
out["sampler.indexes"] = np.asarray(ref.UnifLabelSampler(R.SAMPLER_N, R.SAMPLER_LISTS).indexes, np.int64)

groups = [{"params": [torch.nn.Parameter(torch.zeros(1))], "weight_decay": wd} for wd in R.LR_WEIGHT_DECAYS]
opt = torch.optim.SGD(groups, lr=R.LR_0)
lrs = []
for t in R.LR_STEPS:
    ref.learning_rate_decay(opt, t, R.LR_0)
    lrs.append([float(g["lr"]) for g in opt.param_groups])
out["lr.values"] = np.array(lrs, np.float64)

meter, trace = ref.AverageMeter(), []
for val, n in R.METER_UPDATES:
    meter.update(val, n)
    trace.append([meter.val, meter.sum, meter.count, meter.avg])
out["meter.trace"] = np.array(trace, np.float64)

path = os.path.join(HERE, "sdf.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path))
