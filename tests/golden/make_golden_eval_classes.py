#!/usr/bin/env python3
"""Golden fixture of the reference's metric callables by IMPORTING code/utils/metrics.py on the CPU (make_golden_gambling.py's
stub-package recipe; `medpy`, which the module imports and these callables do not use, is an empty stand-in).

Stores data only (eval_classes.npz), fp64 copies of the reference's float32 results, for the inputs that
tests/test_eval_classes_cpu.py rebuilds from seeds:
  dice.cases, dice.ignore_index : the names of DICE_CASES (bool arrays, float tensors, a multi-valued target, two empty masks) and
                                  the ignore_index recorded for each
  dice.plain, dice.ignored      : dice(input, target) and dice(input, target, ignore_index=k)      (code/utils/metrics.py:39-75)
  batch.dice, batch.jaccard     : compute_dice / compute_jaccard on binary_batch()                 (:79-103), the cross-check of
                                  class_dice_from_logits at two classes

The reference's cal_dice (:14-27) cannot run under this numpy (`np.float` is gone), so nothing of it is recorded: the device
cal_dice is held to the package's own numpy cal_dice, which restates it, in tests/test_eval_classes_gpu.py.

    python tests/golden/make_golden_eval_classes.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/code"

m = types.ModuleType("utils")
m.__path__ = [f"{REF}/utils"]
sys.modules["utils"] = m
medpy, medpy_metric = types.ModuleType("medpy"), types.ModuleType("medpy.metric")
medpy.metric, medpy_metric.hd95 = medpy_metric, None
sys.modules["medpy"], sys.modules["medpy.metric"] = medpy, medpy_metric
ref = importlib.import_module("utils.metrics")

from test_eval_classes_cpu import DICE_CASES, binary_batch, dice_case  # noqa: E402

out = {"dice.cases": np.array(DICE_CASES), "dice.ignore_index": np.zeros(len(DICE_CASES), np.int64),
       "dice.plain": np.zeros(len(DICE_CASES)), "dice.ignored": np.zeros(len(DICE_CASES))}
for i, name in enumerate(DICE_CASES):
    inp, tgt, k = dice_case(name)
    out["dice.ignore_index"][i] = k
    out["dice.plain"][i] = float(ref.dice(inp, tgt))
    out["dice.ignored"][i] = float(ref.dice(inp, tgt, ignore_index=k))
o, l = binary_batch()
out["batch.dice"] = ref.compute_dice(o, l).double().numpy()
out["batch.jaccard"] = ref.compute_jaccard(o, l).double().numpy()
np.savez_compressed(os.path.join(HERE, "eval_classes.npz"), **out)
print({k_: v for k_, v in out.items()}, os.path.getsize(os.path.join(HERE, "eval_classes.npz")))
