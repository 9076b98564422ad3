"""3-D connected components on the device (csrc/components.hip): the `nms` step of the reference's test scripts
(code/utils/test_3d_patch.py:19-26, `getLargestCC`) without a host round trip.

    component_roots(vol, connectivity=3, by_value=False)                  -> int32 roots
    label_components(vol, connectivity=3, by_value=False)                 -> (int32 labels, int32 ncomp (n_vol,))
    largest_component(vol, connectivity=3, return_size=False)             -> uint8 mask [, int32 size (n_vol,)]
    largest_component_per_class(label_map, num_classes, connectivity=3)   -> uint8 label map

`vol` is a numpy array or a CUDA tensor of shape (X, Y, Z) or (n_vol, X, Y, Z), every axis at most 512; the results are device
tensors of the input's shape on the current stream, without a host synchronisation.  `connectivity` 1, 2, 3 means 6, 18, 26
neighbours (skimage's sense).  With `by_value=False` a voxel is foreground when it is non-zero; with `by_value=True` two neighbours
are connected only when their values are equal and lie in 1..255 (skimage.measure.label on an integer map; any other value is
background, as utils/surface.py treats it).

    root    0 for background, else 1 + the smallest linear index (x*Y + y)*Z + z among the voxels of the component
    labels  1..n in raster order of each component's first voxel: what scipy.ndimage.label returns
    largest the component with the most voxels, the one with the smallest root among equals:
            np.argmax(np.bincount(labels.flat)[1:]) + 1

Everything is an integer and the same on every run.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib

MAX_AXIS = 512
WORKSPACE_BUDGET = 1 << 30        # bytes of roots + workspace per launch sequence; more volumes go in chunks
MAX_VOXELS = (1 << 31) - 1        # of one launch sequence


def _operand(vol, by_value):
    if torch.is_tensor(vol):
        if not vol.is_cuda:
            raise ValueError(f"expected a numpy array or a CUDA tensor, got a tensor on {vol.device}")
        t = vol
    else:
        t = torch.as_tensor(np.asarray(vol))
    squeeze = t.dim() == 3
    if squeeze:
        t = t[None]
    if t.dim() != 4:
        raise ValueError(f"expected (X, Y, Z) or (n_vol, X, Y, Z) volumes, got {tuple(t.shape)}")
    if t.shape[0] < 1 or not all(1 <= n <= MAX_AXIS for n in t.shape[1:]):
        raise ValueError(f"every axis of the volume must be in 1..{MAX_AXIS}, got {tuple(t.shape[1:])}")
    if not t.is_cuda:
        t = t.to(torch.device("cuda", torch.cuda.current_device()))
    if t.dtype not in (torch.uint8, torch.int64):
        if not by_value:
            t = t.ne(0).to(torch.uint8)
        elif t.dtype.is_floating_point:
            raise ValueError(f"a label map must hold integers, got {t.dtype}")
        else:
            t = t.to(torch.int64)
    return t.contiguous(), squeeze


def _connectivity(connectivity):
    c = int(connectivity)
    if c != connectivity or not 1 <= c <= 3:
        raise ValueError(f"connectivity must be 1, 2 or 3 (6, 18 or 26 neighbours), got {connectivity!r}")
    return c


def _pieces(t, workspace="dycon_cc_workspace", root_maps=1):
    """(first volume, volume count) of the launch sequences of one call, with the workspace they share: `workspace` names the size
    query, `root_maps` int32 root maps are held next to it"""
    n_vol, X, Y, Z = t.shape
    per_vol = int(_lib.query(workspace, 1, X, Y, Z)) + 4 * root_maps * X * Y * Z
    step = max(1, min(n_vol, WORKSPACE_BUDGET // per_vol, MAX_VOXELS // (X * Y * Z), 65535))
    ws = torch.empty(int(_lib.query(workspace, step, X, Y, Z)), dtype=torch.uint8, device=t.device)
    return [(v0, min(step, n_vol - v0)) for v0 in range(0, n_vol, step)], ws


def _roots(t, v0, nv, connectivity, by_value, root, stream):
    _, X, Y, Z = t.shape
    _lib.call("dycon_cc_roots", t[v0:].data_ptr(), t.element_size(), nv, X, Y, Z, connectivity, int(bool(by_value)), root.data_ptr(),
              stream)


def component_roots(vol, connectivity=3, by_value=False):
    """int32 device tensor of the input's shape: 0 for background, else 1 + the smallest linear index of the voxel's component."""
    conn = _connectivity(connectivity)
    t, squeeze = _operand(vol, by_value)
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream().cuda_stream
        root = torch.empty(t.shape, dtype=torch.int32, device=t.device)
        step = max(1, min(t.shape[0], MAX_VOXELS // t[0].numel(), 65535))
        for v0 in range(0, t.shape[0], step):
            _roots(t, v0, min(step, t.shape[0] - v0), conn, by_value, root[v0:], stream)
    return root[0] if squeeze else root


def label_components(vol, connectivity=3, by_value=False):
    """(labels int32 of the input's shape, ncomp int32 (n_vol,)): consecutive labels 1..ncomp per volume in raster order of each
    component's first voxel, as scipy.ndimage.label numbers them (for by_value: all values' components numbered together)."""
    conn = _connectivity(connectivity)
    t, squeeze = _operand(vol, by_value)
    n_vol, X, Y, Z = t.shape
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream().cuda_stream
        labels = torch.empty(t.shape, dtype=torch.int32, device=t.device)
        ncomp = torch.empty(n_vol, dtype=torch.int32, device=t.device)
        pieces, ws = _pieces(t)
        root = torch.empty((pieces[0][1], X, Y, Z), dtype=torch.int32, device=t.device)
        for v0, nv in pieces:
            _roots(t, v0, nv, conn, by_value, root, stream)
            _lib.call("dycon_cc_labels", root.data_ptr(), nv, X, Y, Z, labels[v0:].data_ptr(), ncomp[v0:].data_ptr(), ws.data_ptr(),
                      ws.numel(), stream)
    return (labels[0] if squeeze else labels), ncomp


def _largest(t, conn, n_cls):
    n_vol, X, Y, Z = t.shape
    slots = max(n_cls, 1)
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream().cuda_stream
        out = torch.empty(t.shape, dtype=torch.uint8, device=t.device)
        size = torch.empty((n_vol, slots), dtype=torch.int32, device=t.device)
        win = torch.empty((n_vol, slots), dtype=torch.int32, device=t.device)
        pieces, ws = _pieces(t)
        root = torch.empty((pieces[0][1], X, Y, Z), dtype=torch.int32, device=t.device)
        for v0, nv in pieces:
            _roots(t, v0, nv, conn, n_cls > 0, root, stream)
            _lib.call("dycon_cc_largest", t[v0:].data_ptr(), t.element_size(), root.data_ptr(), nv, X, Y, Z, n_cls, out[v0:].data_ptr(),
                      size[v0:].data_ptr(), win[v0:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    return out, size


def largest_component(vol, connectivity=3, return_size=False):
    """uint8 mask of the input's shape, 1 on the largest component of `vol != 0` and 0 elsewhere: what `test_3d_patch.getLargestCC`
    keeps (26 neighbours by default; among components of equal size the first in raster order; an empty map stays empty).  With
    return_size also its voxel count per volume, int32 (n_vol,), 0 for an empty volume."""
    conn = _connectivity(connectivity)
    t, squeeze = _operand(vol, False)
    out, size = _largest(t, conn, 0)
    out = out[0] if squeeze else out
    return (out, size[:, 0]) if return_size else out


def largest_component_per_class(label_map, num_classes, connectivity=3):
    """uint8 label map of the input's shape that keeps, for each value 1..num_classes-1, that value's largest component and is 0
    elsewhere (values outside 1..num_classes-1 included)."""
    conn = _connectivity(connectivity)
    C = int(num_classes)
    if not 2 <= C <= 256:
        raise ValueError(f"num_classes must be in 2..256, got {num_classes}")
    t, squeeze = _operand(label_map, True)
    out, _ = _largest(t, conn, C - 1)
    return out[0] if squeeze else out
