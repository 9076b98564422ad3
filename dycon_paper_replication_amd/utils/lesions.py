"""Lesion-wise scores of a prediction against a ground truth on the device (csrc/lesions.hip on the roots of csrc/components.hip):
what stroke segmentation is judged by next to Dice -- lesion-wise F1, the absolute lesion-count difference and the absolute volume
difference -- without the copy of the label map to the host, the two scipy.ndimage.label calls and the loop over lesions.

    lesion_counts(pred, gt, connectivity=3, min_voxels=1)                    -> int64 counts (n_vol, 8), COUNT_FIELDS
    metrics_from_counts(counts, voxel_volume=1.0, empty_value=1.0)           -> dict of fp64 arrays (host)
    lesion_metrics(pred, gt, voxelspacing=None, connectivity=3, min_voxels=1, empty_value=1.0)
    lesion_table(pred, gt, of="gt", connectivity=3, min_voxels=1)            -> per volume (n, 3) int64: label, size, overlap

`pred` and `gt` are numpy arrays or CUDA tensors of one shape, (X, Y, Z) or (n_vol, X, Y, Z), foreground = non-zero; the operand
rules are those of utils/components.py.  A lesion is a connected component (`connectivity` 1, 2, 3 = 6, 18, 26 neighbours).  With
`min_voxels` > 1 every component of fewer voxels is removed from its own mask first, on both sides: a removed predicted lesion is
no false positive and lends no overlap, a removed ground-truth lesion is no false negative.  Two lesions overlap when they share a
voxel; touching is not overlap.

    n_gt, n_pred             components of the two masks
    tp, fn                   ground-truth lesions with / without a shared voxel (fn = n_gt - tp)
    fp                       predicted lesions without a shared voxel
    vox_gt, vox_pred, vox_and  voxels of the two masks and of their intersection

Everything on the device is an integer and the same on every run.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import surface
from .components import _connectivity, _operand, _pieces, _roots

COUNT_FIELDS = ("n_gt", "n_pred", "tp", "fn", "fp", "vox_gt", "vox_pred", "vox_and")


def _min_voxels(min_voxels):
    try:
        m = int(min_voxels)
    except (TypeError, ValueError):
        m = 0
    if isinstance(min_voxels, bool) or m != min_voxels or m < 1:
        raise ValueError(f"min_voxels must be an integer >= 1, got {min_voxels!r}")
    return min(m, (1 << 31) - 1)                      # no component has more voxels than that


def _pair(pred, gt):
    p, squeeze = _operand(pred, False)
    g, squeeze_g = _operand(gt, False)
    if p.shape != g.shape or squeeze != squeeze_g:
        raise ValueError(f"prediction and ground truth must have one shape, got {tuple(np.shape(pred))} and {tuple(np.shape(gt))}")
    if p.device != g.device:
        raise ValueError(f"prediction and ground truth must be on one device, got {p.device} and {g.device}")
    return p, g, squeeze


def _sections(ws, nv, shape):
    """the four per-lesion arrays of a call over `nv` volumes as (nv, X*Y*Z) int32 views of its workspace: size and overlap of the
    prediction's lesions, size and overlap of the ground truth's, each addressed by root - 1 (include/dycon_hip.h)"""
    X, Y, Z = shape
    section = int(_lib.query("dycon_lesion_workspace", nv, X, Y, Z)) // 4
    return [ws[k * section:k * section + 4 * nv * X * Y * Z].view(torch.int32).view(nv, X * Y * Z) for k in range(4)]


def _run(p, g, conn, min_voxels, per_piece=None):
    """counts (n_vol, 8) of the pair; `per_piece(v0, nv, sections)` sees the workspace of each launch sequence before the next reuses
    it"""
    n_vol, X, Y, Z = p.shape
    with torch.cuda.device(p.device):
        stream = torch.cuda.current_stream().cuda_stream
        counts = torch.empty((n_vol, len(COUNT_FIELDS)), dtype=torch.int64, device=p.device)
        pieces, ws = _pieces(p, "dycon_lesion_workspace", root_maps=2)
        root_p, root_g = (torch.empty((pieces[0][1], X, Y, Z), dtype=torch.int32, device=p.device) for _ in range(2))
        for v0, nv in pieces:
            _roots(p, v0, nv, conn, False, root_p, stream)
            _roots(g, v0, nv, conn, False, root_g, stream)
            _lib.call("dycon_lesion_counts", root_p.data_ptr(), root_g.data_ptr(), nv, X, Y, Z, min_voxels, counts[v0:].data_ptr(),
                      ws.data_ptr(), ws.numel(), stream)
            if per_piece is not None:
                per_piece(v0, nv, _sections(ws, nv, (X, Y, Z)))
    return counts


def lesion_counts(pred, gt, connectivity=3, min_voxels=1):
    """int64 device tensor (n_vol, 8), or (8,) for one (X, Y, Z) pair, columns COUNT_FIELDS; on the current stream, no host
    synchronisation."""
    conn, m = _connectivity(connectivity), _min_voxels(min_voxels)
    p, g, squeeze = _pair(pred, gt)
    counts = _run(p, g, conn, m)
    return counts[0] if squeeze else counts


def metrics_from_counts(counts, voxel_volume=1.0, empty_value=1.0):
    """counts (..., 8) integers, columns COUNT_FIELDS -> dict of float64 arrays of shape (...): lesion_f1, lesion_recall,
    lesion_precision, lesion_count_diff, abs_volume_diff, dice.  A ratio whose denominator is zero is `empty_value`.  Host code."""
    c = np.asarray(counts)
    if c.shape[-1:] != (len(COUNT_FIELDS),):
        raise ValueError(f"counts must have {len(COUNT_FIELDS)} columns {COUNT_FIELDS}, got shape {c.shape}")
    f = {name: c[..., k].astype(np.float64) for k, name in enumerate(COUNT_FIELDS)}
    empty = float(empty_value)

    def ratio(num, den):
        return np.where(den > 0, num / np.where(den > 0, den, 1.0), empty)

    return {
        "lesion_f1": ratio(f["tp"], f["tp"] + (f["fp"] + f["fn"]) / 2.0),
        "lesion_recall": ratio(f["tp"], f["n_gt"]),
        "lesion_precision": ratio(f["n_pred"] - f["fp"], f["n_pred"]),
        "lesion_count_diff": np.abs(f["n_pred"] - f["n_gt"]),
        "abs_volume_diff": np.abs(f["vox_pred"] - f["vox_gt"]) * float(voxel_volume),
        "dice": ratio(2.0 * f["vox_and"], f["vox_pred"] + f["vox_gt"]),
    }


def lesion_metrics(pred, gt, voxelspacing=None, connectivity=3, min_voxels=1, empty_value=1.0):
    """`metrics_from_counts` of `lesion_counts`: one read-back of 8 integers per volume.  abs_volume_diff is in the units of
    `voxelspacing` cubed (medpy's normalisation of the argument, utils/surface.py), in voxels without one."""
    spacing, _ = surface.normalise_spacing(voxelspacing)
    counts = lesion_counts(pred, gt, connectivity, min_voxels).cpu().numpy()
    return metrics_from_counts(counts, float(np.prod(spacing)) if spacing is not None else 1.0, empty_value)


def lesion_table(pred, gt, of="gt", connectivity=3, min_voxels=1):
    """Per volume an int64 array (n, 3) of (label, size, overlap) for the surviving lesions of one side, `of` = "gt" or "pred": label
    1..n by root, which is scipy.ndimage.label's numbering of the filtered mask; size in voxels; overlap = its voxels that are
    foreground in the other filtered mask.  One array for an (X, Y, Z) pair, a list of n_vol arrays otherwise.  A reporting helper:
    it synchronises."""
    if of not in ("gt", "pred"):
        raise ValueError(f'of must be "gt" or "pred", got {of!r}')
    conn, m = _connectivity(connectivity), _min_voxels(min_voxels)
    p, g, squeeze = _pair(pred, gt)
    tables = []

    def per_piece(v0, nv, sections):
        size, overlap = sections[2:] if of == "gt" else sections[:2]
        for v in range(nv):
            at = torch.nonzero(size[v] >= m).flatten()             # ascending: the order of the roots
            label = torch.arange(1, at.numel() + 1, dtype=torch.int64, device=at.device)
            tables.append(torch.stack([label, size[v][at].long(), overlap[v][at].long()], 1).cpu().numpy())

    _run(p, g, conn, m, per_piece)
    return tables[0] if squeeze else tables
