#!/usr/bin/env python3
"""Golden fixture for the C-class one-pass voxel losses, by IMPORTING the reference on CPU (the stub-package recipe of
make_golden_nclasses.py, whose module objects are reused).  Stores data only:

  voxel_losses_nc.npz   make_golden.gen_voxel_losses' recipe per class count.  Cases (`cases`): c3, c4, c5, c8 with logits a, b of
                        shape (3, C, 6, 8, 10) at scale 2.0 and integer labels in [0, C); c4_absent, the same with class 2 absent
                        from the labels (Y_2 = 0); c5_large with (3, 5, 56, 56, 56), more voxels than one pass of a 2048 x 256 grid.

    per case   {case}.seed / .shape / .label (uint8; not for c5_large) / .a_stats / .b_stats / .label_counts
    per term   ce, dice (class 1), dice_mc (DiceLoss(C)) on the labelled split [:LB], LB = 1;
               cons_mse, cons_kl (on PROBABILITIES, as the step calls them) and uncl0, uncl1 (UnCLoss at `betas`) on all 3 samples:
               {case}.{term} (fp32 value), {case}.{term}.f64 (fp64 twin), {case}.{term}.fp32_dist (see below),
               {case}.{term}_grad.f64 (gradient w.r.t. a of the fp64 twin)
               c5_large instead: {term}_grad_stats / .f64 (sum, abs sum, square sum) and {term}_grad_sub.f64 (every 8th voxel per axis)

Inputs are NOT stored: a test rebuilds them with `draw(seed, shape, classes)` below (default_rng(seed): a, then b, then the labels)
and checks `a_stats` / `b_stats` first.

Size: the file has to stay under 1 MB, and the gradients of seven terms in two precisions do not fit.  The fp64 twin's gradients are
therefore stored ROUNDED to float32 (6e-8 relative, three orders below the tightest gradient tolerance) and of the reference's own
fp32 gradients only what a test needs: their distance to the twin, `fp32_dist` = [value distance, gradient distance], each the
smallest rtol at which numpy.testing.assert_allclose(fp32, fp64, rtol, atol) passes with the atol of TOL below.

Condition checked here: every fp32 value and gradient of the reference lies within HALF of TOL's rtol of its fp64 twin, i.e. the
reference alone stays inside the bound a kernel is held to.  A term that misses is listed in `{case}.loose` and a test uses twice its
stored distance (the rule of tests/test_engine_gpu.py::within_budget).

    python tests/golden/make_golden_trainer_nc.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_nclasses import ref_dycon, ref_losses, save, stats  # noqa: E402

torch.set_num_threads(8)

LB, BETAS = 1, (0.5, 5.0)
# (value rtol, value atol, gradient rtol, gradient atol): tests/test_ops_gpu.py::test_voxel_losses_golden / test_uncl_golden
TOL = {"ce": (1e-5, 1e-6, 1e-4, 1e-8), "dice": (1e-5, 1e-6, 1e-4, 1e-8), "dice_mc": (1e-5, 1e-6, 1e-4, 1e-8),
       "cons_mse": (1e-5, 1e-7, 1e-4, 1e-9), "cons_kl": (1e-4, 1e-7, 1e-4, 1e-9),
       "uncl0": (1e-5, 1e-6, 1e-4, 1e-8), "uncl1": (1e-5, 1e-6, 1e-4, 1e-8)}
CASES = (("c3", 3, (6, 8, 10), 4103, None), ("c4", 4, (6, 8, 10), 4104, None), ("c5", 5, (6, 8, 10), 4105, None),
         ("c8", 8, (6, 8, 10), 4108, None), ("c4_absent", 4, (6, 8, 10), 4114, 2), ("c5_large", 5, (56, 56, 56), 4125, None))


def draw(seed, shape, classes, absent=None):
    """a, b (3, C, *shape) float32 at scale 2.0 and labels (3, *shape) int64 in [0, C) without `absent`"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((3, classes) + tuple(shape)) * 2.0).astype(np.float32)
    b = (rng.standard_normal((3, classes) + tuple(shape)) * 2.0).astype(np.float32)
    present = np.array([c for c in range(classes) if c != absent])
    lab = present[rng.integers(0, len(present), (3,) + tuple(shape))].astype(np.int64)
    return a, b, lab


def rtol_needed(x, ref, atol):
    """smallest rtol with |x - ref| <= atol + rtol |ref| everywhere"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    excess = np.maximum(np.abs(x - ref) - atol, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(excess > 0, excess / np.abs(ref), 0.0)
    return float(np.max(r))


def terms(a, b, lab, C, dtype):
    """{term: (value, gradient w.r.t. a)} with the reference's callables, in `dtype`"""
    a, b = torch.from_numpy(a).to(dtype), torch.from_numpy(b).to(dtype)
    lab = torch.from_numpy(lab)
    uncl = ref_dycon.UnCLoss()
    fns = {
        "ce": lambda x: nn.CrossEntropyLoss()(x[:LB], lab[:LB].long()),
        "dice": lambda x: ref_losses.dice_loss(F.softmax(x, 1)[:LB, 1], lab[:LB] == 1),
        "dice_mc": lambda x: ref_losses.DiceLoss(C)(F.softmax(x, 1)[:LB], lab[:LB].unsqueeze(1)),
        "cons_mse": lambda x: ref_losses.softmax_mse_loss(F.softmax(x, 1), F.softmax(b, 1)).mean(),
        "cons_kl": lambda x: ref_losses.softmax_kl_loss(F.softmax(x, 1), F.softmax(b, 1)),
        "uncl0": lambda x: uncl(x, b, BETAS[0]),
        "uncl1": lambda x: uncl(x, b, BETAS[1]),
    }
    out = {}
    for k, fn in fns.items():
        x = a.clone().requires_grad_(True)
        v = fn(x)
        out[k] = (v.detach(), torch.autograd.grad(v, x)[0])
    return out


def gen():
    out = {"cases": np.array([c[0] for c in CASES]), "terms": np.array(list(TOL)), "betas": np.array(BETAS), "LB": np.array(LB),
           "draw_order": np.array("default_rng(seed): a (3,C,*shape) * 2.0 -> float32, b likewise, integers(0, #present, (3,*shape))")}
    missed = []
    for tag, C, shape, seed, absent in CASES:
        a, b, lab = draw(seed, shape, C, absent)
        large = tag.endswith("_large")
        counts = np.bincount(lab.reshape(-1), minlength=C)
        assert all((counts[c] > 0) != (c == absent) for c in range(C))
        out.update({f"{tag}.seed": np.array(seed), f"{tag}.classes": np.array(C), f"{tag}.shape": np.array(shape),
                    f"{tag}.absent": np.array(-1 if absent is None else absent), f"{tag}.label_counts": counts,
                    f"{tag}.a_stats": stats(torch.from_numpy(a)), f"{tag}.b_stats": stats(torch.from_numpy(b))})
        if not large:
            out[f"{tag}.label"] = lab.astype(np.uint8)
        r32, r64 = terms(a, b, lab, C, torch.float32), terms(a, b, lab, C, torch.float64)
        loose = []
        for k, (vr, va, gr, ga) in TOL.items():
            (v32, g32), (v64, g64) = r32[k], r64[k]
            dv, dg = rtol_needed(v32.numpy(), v64.numpy(), va), rtol_needed(g32.numpy(), g64.numpy(), ga)
            print(f"  {tag:10s} {k:9s} value {float(v64):.9g}  fp32 distance {dv:.2e} (bound {vr:.0e})   gradient {dg:.2e} (bound {gr:.0e})")
            if dv > 0.5 * vr or dg > 0.5 * gr:
                loose.append(k)
            out.update({f"{tag}.{k}": v32.numpy(), f"{tag}.{k}.f64": v64.numpy(), f"{tag}.{k}.fp32_dist": np.array([dv, dg])})
            if large:
                out.update({f"{tag}.{k}_grad_stats": stats(g32), f"{tag}.{k}_grad_stats.f64": stats(g64),
                            f"{tag}.{k}_grad_sub.f64": g64[..., ::8, ::8, ::8].numpy().astype(np.float32)})
            else:
                out[f"{tag}.{k}_grad.f64"] = g64.numpy().astype(np.float32)
        out[f"{tag}.loose"] = np.array(loose, dtype="U16")
        missed += [f"{tag}.{k}" for k in loose]
    save("voxel_losses_nc", **out)
    size = os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "voxel_losses_nc.npz"))
    assert size < 1_000_000, f"voxel_losses_nc.npz is {size} bytes"
    if missed:
        print("the reference's own fp32 is further than half the tolerance from its fp64 twin in:", ", ".join(missed))
        print("(their distances are stored; a test holds a kernel to twice that)")
    return missed


if __name__ == "__main__":
    sys.exit(1 if gen() else 0)      # the fixture is written either way; a miss must not pass unnoticed
