"""Surface distances on the device: HD95 / ASD (medpy.metric.binary.hd95 / asd, restated in `test_3d_patch._surface_distances`) between
the borders of binary pairs, with medpy's `voxelspacing` and `connectivity`.

    surface_hists(a, b, classes=None)            -> (hist (S, 2, nbins) int32, nborder (S, 2) int32) device tensors; unit spacing only
    surface_metrics(a, b, classes=None, q=95.0, voxelspacing=None, connectivity=1)
                                                 -> (S, 5) float64 device tensor, no host sync
    metrics_from_hists(hist, nborder, q=95.0)    -> the same (S, 5) in numpy fp64, usable without a GPU
    metrics_from_distances(d_ab, d_ba, q=95.0)   -> one such row from the two directions' distances, numpy fp64, no GPU

`a` (prediction) and `b` (ground truth) are numpy arrays or CUDA tensors of one shape, (X, Y, Z) or (n_vol, X, Y, Z), every axis at
most 512.  With `classes=None` a voxel belongs to its mask when it is non-zero and there is one pair per volume.  With
`classes=(lo, n)`, lo >= 1, the inputs are label maps and pair v * n + k compares `a[v] == lo + k` with `b[v] == lo + k`: all classes
of a case share one set of launches.  A row of the result is (percentile q of both directions, mean a -> b, mean b -> a,
|border(a)|, |border(b)|); the first three are NaN when either border is empty.  hist[s, 0, d] counts the border voxels of a whose
squared distance to the border of b is d, hist[s, 1] the other direction.

Two paths.  `voxelspacing=None` with `connectivity=1` is the histogram path (csrc/surface.hip): everything up to the final square
root is integer arithmetic, so the histograms are exact and the same on every run.  Anything else -- a spacing, `(1, 1, 1)` given
explicitly included, or connectivity 2 or 3 (18 or 26 neighbours in the erosion that defines the border) -- is the weighted path
(csrc/surface_spacing.hip): an fp64 transform whose value is the exact minimum of the cost
fl(fl(fl(wz dz^2) + fl(wy dy^2)) + fl(wx dx^2)), w = spacing^2, a radix select for the percentile and fixed-order sums for the means;
also the same bits on every run.  `voxelspacing` is None, one positive number for all axes, or one per axis (X, Y, Z), as medpy
normalises it; one spacing serves every volume of a call.  Not covered: 2-D inputs, a spacing per volume within one call.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .. import _lib

MAX_AXIS = 512
MIN_SPACING, MAX_SPACING = 1e-150, 1e150      # the squares stay normal fp64 numbers
WORKSPACE_BUDGET = 1 << 30        # bytes of distance-transform workspace per launch sequence; more pairs go in chunks


def nbins_of(shape):
    """number of squared-distance bins of an (X, Y, Z) volume: the largest squared distance between two voxels, plus one"""
    return int(sum((int(n) - 1) ** 2 for n in shape)) + 1


def _operands(a, b):
    ta = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    tb = b if torch.is_tensor(b) else torch.as_tensor(np.asarray(b))
    if ta.shape != tb.shape:
        raise ValueError(f"prediction {tuple(ta.shape)} and ground truth {tuple(tb.shape)} differ in shape")
    if ta.dim() == 3:
        ta, tb = ta[None], tb[None]
    if ta.dim() != 4:
        raise ValueError(f"expected (X, Y, Z) or (n_vol, X, Y, Z) volumes, got {tuple(a.shape)}")
    if ta.shape[0] < 1 or not all(1 <= n <= MAX_AXIS for n in ta.shape[1:]):
        raise ValueError(f"every axis of the volume must be in 1..{MAX_AXIS}, got {tuple(ta.shape[1:])}")
    dev = ta.device if ta.is_cuda else tb.device if tb.is_cuda else torch.device("cuda:0")
    return ta.to(dev), tb.to(dev)


def _class_range(classes):
    if classes is None:
        return 0, 1
    lo, n = (int(v) for v in classes)
    if lo < 1 or n < 1 or lo + n > 256:
        raise ValueError(f"classes = (lo, n) takes lo >= 1, n >= 1 and lo + n <= 256, got {classes}")
    return lo, n


def _kernel_inputs(a, b, lo):
    """the prediction as uint8 and the ground truth as uint8 or int64, contiguous, on one device"""
    ta, tb = _operands(a, b)
    if lo == 0:                                   # membership is voxel != 0
        ta = ta if ta.dtype == torch.uint8 else ta.ne(0).to(torch.uint8)
        tb = tb if tb.dtype in (torch.uint8, torch.int64) else tb.ne(0).to(torch.uint8)
    else:                                         # label maps: keep a value outside uint8 out of every class
        if ta.dtype != torch.uint8:
            ta = torch.where((ta < 0) | (ta > 255), 0, ta).to(torch.uint8)
        tb = tb if tb.dtype in (torch.uint8, torch.int64) else tb.to(torch.int64)
    return ta.contiguous(), tb.contiguous()


def surface_hists(a, b, classes=None):
    """(hist (S, 2, nbins), nborder (S, 2)) as int32 device tensors (the kernels' unsigned counts; none reaches 2^31).  No host sync.
    Unit voxel spacing and 6-neighbour borders only."""
    lo, n_cls = _class_range(classes)
    ta, tb = _kernel_inputs(a, b, lo)
    n_vol, X, Y, Z = ta.shape
    nbins = nbins_of((X, Y, Z))
    hist = torch.empty((n_vol * n_cls, 2, nbins), dtype=torch.int32, device=ta.device)
    nborder = torch.empty((n_vol * n_cls, 2), dtype=torch.int32, device=ta.device)
    per_vol = int(_lib.query("dycon_surface_workspace", n_cls, X, Y, Z))
    step = max(1, min(n_vol, WORKSPACE_BUDGET // per_vol, 32767 // n_cls))
    ws = torch.empty(step * per_vol, dtype=torch.uint8, device=ta.device)
    stream = torch.cuda.current_stream(ta.device).cuda_stream
    for v0 in range(0, n_vol, step):
        nv = min(step, n_vol - v0)
        _lib.call("dycon_surface_hist", ta[v0:].data_ptr(), 1, tb[v0:].data_ptr(), tb.element_size(), nv, lo, n_cls, X, Y, Z,
                  hist[v0 * n_cls:].data_ptr(), nborder[v0 * n_cls:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return hist, nborder


def _metrics_of(hist, nborder, q):
    out = torch.empty((hist.shape[0], 5), dtype=torch.float64, device=hist.device)
    _lib.call("dycon_surface_metrics", hist.data_ptr(), nborder.data_ptr(), hist.shape[0], hist.shape[2], float(q), out.data_ptr(),
              torch.cuda.current_stream(hist.device).cuda_stream)
    return out


def normalise_spacing(voxelspacing, connectivity=1):
    """medpy's normalisation of `voxelspacing` for a 3-D volume: None -> None, a number -> that number for the three axes, a sequence
    -> its three numbers; each finite and > 0.  connectivity must be 1, 2 or 3.  Returns (None or a 3-tuple of floats, connectivity).
    Raises ValueError before anything touches the GPU."""
    if isinstance(connectivity, bool) or connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours), got {connectivity!r}")
    if voxelspacing is None:
        return None, int(connectivity)
    sp = np.asarray(voxelspacing, dtype=np.float64)
    if sp.ndim == 0:
        sp = np.repeat(sp, 3)
    if sp.shape != (3,):
        raise ValueError(f"voxelspacing takes one number or one per axis (X, Y, Z), got {voxelspacing!r}")
    if not (np.isfinite(sp).all() and (sp > 0).all() and (sp >= MIN_SPACING).all() and (sp <= MAX_SPACING).all()):
        raise ValueError(f"every voxel spacing must be finite, > 0 and within {MIN_SPACING:g}..{MAX_SPACING:g}, got {voxelspacing!r}")
    return tuple(float(v) for v in sp), int(connectivity)


def _spaced_metrics(a, b, classes, q, spacing, connectivity):
    lo, n_cls = _class_range(classes)
    ta, tb = _kernel_inputs(a, b, lo)
    n_vol, X, Y, Z = ta.shape
    out = torch.empty((n_vol * n_cls, 5), dtype=torch.float64, device=ta.device)
    per_vol = int(_lib.query("dycon_surface_spaced_workspace", n_cls, X, Y, Z))
    step = max(1, min(n_vol, WORKSPACE_BUDGET // per_vol, 32767 // n_cls))
    ws = torch.empty(step * per_vol // 8, dtype=torch.float64, device=ta.device)
    sp = (ctypes.c_double * 3)(*spacing)
    stream = torch.cuda.current_stream(ta.device).cuda_stream
    for v0 in range(0, n_vol, step):
        nv = min(step, n_vol - v0)
        _lib.call("dycon_surface_spaced_metrics", ta[v0:].data_ptr(), 1, tb[v0:].data_ptr(), tb.element_size(), nv, lo, n_cls, X, Y, Z,
                  sp, connectivity, float(q), out[v0 * n_cls:].data_ptr(), ws.data_ptr(), ws.numel() * 8, stream)
    return out


def surface_metrics(a, b, classes=None, q=95.0, voxelspacing=None, connectivity=1):
    """(S, 5) float64 device tensor: percentile q of both directions, mean a -> b, mean b -> a, |border(a)|, |border(b)|.  No host
    sync.  voxelspacing=None with connectivity=1 is the histogram path; anything else the weighted path (module docstring)."""
    if not 0.0 <= float(q) <= 100.0:
        raise ValueError(f"percentile {q} outside [0, 100]")
    spacing, connectivity = normalise_spacing(voxelspacing, connectivity)
    if spacing is None and connectivity == 1:
        hist, nborder = surface_hists(a, b, classes)
        return _metrics_of(hist, nborder, q)
    return _spaced_metrics(a, b, classes, q, spacing or (1.0, 1.0, 1.0), connectivity)


def metrics_from_distances(d_ab, d_ba, q=95.0):
    """The finalise step of the weighted path in numpy fp64: the distances of the border voxels of a to the border of b and of b to a
    -> (5,) = percentile q of their union (np.percentile's default rule, evaluated from the two order statistics as the kernel
    does), mean a -> b, mean b -> a, the two counts; the first three NaN when either is empty.  The kernel adds the means in a fixed
    order of its own: the two agree to rounding."""
    d_ab, d_ba = np.asarray(d_ab, np.float64).ravel(), np.asarray(d_ba, np.float64).ravel()
    na, nb = d_ab.size, d_ba.size
    out = np.array([np.nan, np.nan, np.nan, na, nb])
    if na == 0 or nb == 0:
        return out
    n = na + nb
    vi = (n - 1) * (float(q) / 100.0)
    gamma = vi - np.floor(vi)
    lo, hi = int(np.floor(vi)), int(np.floor(vi)) + 1
    if vi >= n - 1:
        lo = hi = n - 1
    if vi < 0:
        lo = hi = 0
    both = np.partition(np.hstack((d_ab, d_ba)), (lo, hi))
    v0, v1 = both[lo], both[hi]
    diff = v1 - v0
    out[0] = v1 - diff * (1.0 - gamma) if gamma >= 0.5 else v0 + diff * gamma
    out[1], out[2] = d_ab.sum() / na, d_ba.sum() / nb
    return out


def metrics_from_hists(hist, nborder, q=95.0):
    """The finalise kernel in numpy fp64: hist (S, 2, nbins) and nborder (S, 2) counts (arrays or tensors) -> (S, 5).  The percentile is
    np.percentile's default rule on the sorted union of both directions, taken from the cumulative counts; the means are
    sum(count * sqrt(bin)) / n (the kernel adds them in a fixed order of its own: the two agree to rounding)."""
    hist = np.asarray(hist.cpu() if torch.is_tensor(hist) else hist).astype(np.int64)
    nborder = np.asarray(nborder.cpu() if torch.is_tensor(nborder) else nborder).astype(np.int64)
    if hist.ndim == 2:
        hist, nborder = hist[None], nborder[None]
    roots = np.sqrt(np.arange(hist.shape[2], dtype=np.float64))
    out = np.full((hist.shape[0], 5), np.nan)
    p = float(q) / 100.0
    for s in range(hist.shape[0]):
        na, nb = int(nborder[s, 0]), int(nborder[s, 1])
        out[s, 3:] = na, nb
        if na == 0 or nb == 0:
            continue
        cum = np.cumsum(hist[s, 0] + hist[s, 1])
        n = na + nb
        vi = (n - 1) * p                                         # numpy's virtual index of the "linear" method
        gamma = vi - np.floor(vi)
        lo, hi = int(np.floor(vi)), int(np.floor(vi)) + 1
        if vi >= n - 1:
            lo = hi = n - 1
        if vi < 0:
            lo = hi = 0
        v0, v1 = (roots[min(int(np.searchsorted(cum, r, side="right")), len(roots) - 1)] for r in (lo, hi))
        diff = v1 - v0
        out[s, 0] = v1 - diff * (1.0 - gamma) if gamma >= 0.5 else v0 + diff * gamma
        out[s, 1] = float(np.dot(hist[s, 0].astype(np.float64), roots)) / na
        out[s, 2] = float(np.dot(hist[s, 1].astype(np.float64), roots)) / nb
    return out
