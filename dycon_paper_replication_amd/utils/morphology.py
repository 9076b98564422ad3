"""Post-processing of a predicted mask on the device (csrc/morphology.hip on the roots of csrc/components.hip): what
``scipy.ndimage`` returns, bit for bit, without the copy of the label map to the host and back.

    binary_erosion(mask, connectivity=1, iterations=1)         ndimage.binary_erosion(mask, generate_binary_structure(3, c), n)
    binary_dilation(mask, connectivity=1, iterations=1)        ndimage.binary_dilation
    binary_opening(mask, connectivity=1, iterations=1)         n erosions, then n dilations: ndimage.binary_opening(..., iterations=n)
    binary_closing(mask, connectivity=1, iterations=1)         n dilations, then n erosions: ndimage.binary_closing
    binary_fill_holes(mask, connectivity=1)                    ndimage.binary_fill_holes(mask, generate_binary_structure(3, c))
    remove_small_components(mask, min_voxels, connectivity=3)  the components of at least min_voxels voxels

    PostProcess(*steps)           steps: Erosion, Dilation, Opening, Closing, FillHoles, MinSize, Largest
        pp(mask)                                the steps in order on `mask != 0`
        pp.per_class(label_map, num_classes)    the steps on each class 1..C-1 of a label map, recombined

`mask` is a numpy array or a CUDA tensor of shape (X, Y, Z) or (n_vol, X, Y, Z), every axis in 1..512, foreground = non-zero: the
operand rules of utils/components.py.  Results are uint8 CUDA tensors of the input's shape on the current stream, without a host
synchronisation.  `connectivity` 1, 2, 3 means 6, 18, 26 neighbours plus the centre; `iterations` is 1..64.  Voxels outside the
volume are background for erosion and dilation alike (scipy's border_value=0): a mask that touches a face is eaten there by the
erosion half of a closing, as scipy does it.

The stencil operations and the hole filling work on bit-packed masks (64 voxels along z per word); a run of them inside a
`PostProcess` packs once and unpacks once.  Everything is an integer and the same on every run.
"""
from __future__ import annotations

import dataclasses

import torch

from .. import _lib
from . import components
from .components import MAX_VOXELS, WORKSPACE_BUDGET, _connectivity, _operand
from .lesions import _min_voxels

ERODE, DILATE = 0, 1                                  # DYCON_MORPH_ERODE, DYCON_MORPH_DILATE
MAX_ITERATIONS = 64


def _iterations(iterations):
    try:
        n = int(iterations)
    except (TypeError, ValueError):
        n = 0
    if isinstance(iterations, bool) or n != iterations or not 1 <= n <= MAX_ITERATIONS:
        raise ValueError(f"iterations must be an integer in 1..{MAX_ITERATIONS} (repeat-until-stable, iterations < 1, is not "
                         f"supported), got {iterations!r}")
    return n


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _steps(shape, per_voxel_bytes=0):
    """(first volume, volume count) of the launch sequences of one call over a batch of this shape: at most 65535 volumes and
    2^31 - 1 voxels each, and `per_voxel_bytes` of workspace per voxel within the budget of utils/components.py"""
    n_vol, V = shape[0], shape[1] * shape[2] * shape[3]
    step = min(n_vol, MAX_VOXELS // V, 65535)
    if per_voxel_bytes:
        step = min(step, WORKSPACE_BUDGET // (per_voxel_bytes * V))
    step = max(1, step)
    return [(v0, min(step, n_vol - v0)) for v0 in range(0, n_vol, step)]


class _Mask:
    """A batch of masks (n_vol, X, Y, Z) on the device in one or more of its forms; the form a step needs is made when it asks.

        source   the caller's uint8 / int64 volume: foreground = non-zero, or == `value` (one class of a label map)
        words    int64 (n_vol, X, Y, ceil(Z / 64)), bit-packed
        mask01   uint8, 0 / 1
    """

    def __init__(self, shape, source=None, value=None, words=None, mask01=None):
        self.shape, self.source, self.value, self.words, self.mask01 = tuple(shape), source, value, words, mask01

    def packed(self):
        if self.words is None:
            n_vol, X, Y, Z = self.shape
            t, by_value = (self.mask01, False) if self.mask01 is not None else (self.source, self.value is not None)
            self.words = torch.empty((n_vol, X, Y, (Z + 63) // 64), dtype=torch.int64, device=t.device)
            for v0, nv in _steps(self.shape):
                _lib.call("dycon_morph_pack", t[v0:].data_ptr(), t.element_size(), nv, X, Y, Z, int(by_value),
                          int(self.value) if by_value else 0, self.words[v0:].data_ptr(), _stream())
        return self.words

    def unpacked(self):
        if self.mask01 is None:
            n_vol, X, Y, Z = self.shape
            words = self.packed()
            self.mask01 = torch.empty(self.shape, dtype=torch.uint8, device=words.device)
            for v0, nv in _steps(self.shape):
                _lib.call("dycon_morph_unpack", words[v0:].data_ptr(), nv, X, Y, Z, self.mask01[v0:].data_ptr(), _stream())
        return self.mask01

    def labelable(self):
        """a volume whose non-zero voxels are the mask: what dycon_cc_roots takes"""
        if self.mask01 is None and self.words is None and self.value is None:
            return self.source
        return self.unpacked()


def _stencil(m, conn, op, n):
    n_vol, X, Y, Z = m.shape
    src = m.packed()
    out = torch.empty_like(src)
    scratch = torch.empty_like(src) if n > 1 else None
    for v0, nv in _steps(m.shape):
        _lib.call("dycon_morph_stencil", src[v0:].data_ptr(), out[v0:].data_ptr(), scratch[v0:].data_ptr() if n > 1 else None, nv, X, Y,
                  Z, conn, op, n, _stream())
    return _Mask(m.shape, words=out)


def _fill(m, conn):
    n_vol, X, Y, Z = m.shape
    src = m.packed()
    out = torch.empty_like(src)
    pieces = _steps(m.shape, per_voxel_bytes=5)
    ws = torch.empty(int(_lib.query("dycon_morph_fill_workspace", pieces[0][1], X, Y, Z)), dtype=torch.uint8, device=src.device)
    for v0, nv in pieces:
        _lib.call("dycon_morph_fill_holes", src[v0:].data_ptr(), nv, X, Y, Z, conn, out[v0:].data_ptr(), ws.data_ptr(), ws.numel(),
                  _stream())
    return _Mask(m.shape, words=out)


def _min_size(m, min_voxels, conn):
    n_vol, X, Y, Z = m.shape
    t = m.labelable()
    out = torch.empty(m.shape, dtype=torch.uint8, device=t.device)
    pieces = _steps(m.shape, per_voxel_bytes=8)
    root = torch.empty((pieces[0][1], X, Y, Z), dtype=torch.int32, device=t.device)
    ws = torch.empty(int(_lib.query("dycon_cc_min_size_workspace", pieces[0][1], X, Y, Z)), dtype=torch.uint8, device=t.device)
    for v0, nv in pieces:
        components._roots(t, v0, nv, conn, False, root, _stream())
        _lib.call("dycon_cc_keep_min_size", root.data_ptr(), nv, X, Y, Z, min_voxels, out[v0:].data_ptr(), ws.data_ptr(), ws.numel(),
                  _stream())
    return _Mask(m.shape, mask01=out)


def _largest(m, conn):
    return _Mask(m.shape, mask01=components._largest(m.labelable(), conn, 0)[0])


# ------------------------------------------------------------------------------------------------------------------- steps
@dataclasses.dataclass(frozen=True)
class _Stencil:
    connectivity: int = 1
    iterations: int = 1

    def __post_init__(self):
        object.__setattr__(self, "connectivity", _connectivity(self.connectivity))
        object.__setattr__(self, "iterations", _iterations(self.iterations))

    def _apply(self, m):
        for op in self._ops:
            m = _stencil(m, self.connectivity, op, self.iterations)
        return m


@dataclasses.dataclass(frozen=True)
class Erosion(_Stencil):
    """`iterations` erosions by generate_binary_structure(3, connectivity)"""
    _ops = (ERODE,)


@dataclasses.dataclass(frozen=True)
class Dilation(_Stencil):
    """`iterations` dilations by generate_binary_structure(3, connectivity)"""
    _ops = (DILATE,)


@dataclasses.dataclass(frozen=True)
class Opening(_Stencil):
    """`iterations` erosions, then as many dilations"""
    _ops = (ERODE, DILATE)


@dataclasses.dataclass(frozen=True)
class Closing(_Stencil):
    """`iterations` dilations, then as many erosions"""
    _ops = (DILATE, ERODE)


@dataclasses.dataclass(frozen=True)
class FillHoles:
    """the background components (at `connectivity`) that touch no face of the volume become foreground"""
    connectivity: int = 1

    def __post_init__(self):
        object.__setattr__(self, "connectivity", _connectivity(self.connectivity))

    def _apply(self, m):
        return _fill(m, self.connectivity)


@dataclasses.dataclass(frozen=True)
class MinSize:
    """the components (at `connectivity`) of fewer than `min_voxels` voxels are removed"""
    min_voxels: int
    connectivity: int = 3

    def __post_init__(self):
        object.__setattr__(self, "min_voxels", _min_voxels(self.min_voxels))
        object.__setattr__(self, "connectivity", _connectivity(self.connectivity))

    def _apply(self, m):
        return _min_size(m, self.min_voxels, self.connectivity)


@dataclasses.dataclass(frozen=True)
class Largest:
    """only the largest component stays: `components.largest_component`"""
    connectivity: int = 3

    def __post_init__(self):
        object.__setattr__(self, "connectivity", _connectivity(self.connectivity))

    def _apply(self, m):
        return _largest(m, self.connectivity)


STEPS = (Erosion, Dilation, Opening, Closing, FillHoles, MinSize, Largest)


def _run(steps, vol, value=None):
    """uint8 0 / 1 tensor of the shape of `vol`: the steps in order on vol != 0, or on vol == value"""
    t, squeeze = _operand(vol, value is not None)
    with torch.cuda.device(t.device):
        m = _Mask(t.shape, source=t, value=value)
        for s in steps:
            m = s._apply(m)
        out = m.unpacked()
    return out[0] if squeeze else out


class PostProcess:
    """A fixed sequence of post-processing steps.  `pp(mask)` runs them in order on `mask != 0`; consecutive Erosion / Dilation /
    Opening / Closing / FillHoles steps hand the bit-packed mask on, so a run of them packs once and unpacks once."""

    def __init__(self, *steps):
        for s in steps:
            if not isinstance(s, STEPS):
                raise TypeError(f"a PostProcess takes {', '.join(c.__name__ for c in STEPS)} steps, got {s!r}")
        self.steps = tuple(steps)

    def __repr__(self):
        return f"PostProcess({', '.join(repr(s) for s in self.steps)})"

    def __eq__(self, other):
        return isinstance(other, PostProcess) and self.steps == other.steps

    def __hash__(self):
        return hash(self.steps)

    def __call__(self, mask):
        return _run(self.steps, mask)

    def per_class(self, label_map, num_classes):
        """uint8 label map of the input's shape: every class 1..num_classes-1 goes through the steps as a mask of its own; a voxel keeps
        its value v when class v's processed mask still holds it, otherwise it takes the smallest class whose processed mask holds
        it, or 0.  Steps that only shrink a mask never make two classes claim one voxel."""
        C = int(num_classes)
        if not 2 <= C <= 256:
            raise ValueError(f"num_classes must be in 2..256, got {num_classes}")
        t, squeeze = _operand(label_map, True)
        with torch.cuda.device(t.device):
            out = torch.zeros(t.shape, dtype=torch.uint8, device=t.device)
            for c in range(C - 1, 0, -1):                     # descending: the last writer of a contested voxel is the smallest class
                mask = _run(self.steps, t, value=c)
                _lib.call("dycon_morph_merge_class", t.data_ptr(), t.element_size(), mask.data_ptr(), c, t.numel(), out.data_ptr(),
                          _stream())
        return out[0] if squeeze else out


def check_postprocess(postprocess):
    """the `postprocess` argument of the evaluators: None or a PostProcess"""
    if postprocess is not None and not isinstance(postprocess, PostProcess):
        raise TypeError(f"postprocess must be None or a morphology.PostProcess, got {postprocess!r}")
    return postprocess


# ------------------------------------------------------------------------------------------------------------------- functions
def binary_erosion(mask, connectivity=1, iterations=1):
    return _run((Erosion(connectivity, iterations),), mask)


def binary_dilation(mask, connectivity=1, iterations=1):
    return _run((Dilation(connectivity, iterations),), mask)


def binary_opening(mask, connectivity=1, iterations=1):
    return _run((Opening(connectivity, iterations),), mask)


def binary_closing(mask, connectivity=1, iterations=1):
    return _run((Closing(connectivity, iterations),), mask)


def binary_fill_holes(mask, connectivity=1):
    return _run((FillHoles(connectivity),), mask)


def remove_small_components(mask, min_voxels, connectivity=3):
    return _run((MinSize(min_voxels, connectivity),), mask)
