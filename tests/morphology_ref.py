"""scipy.ndimage calls the morphology kernels (csrc/morphology.hip) are held to, independent restatements of the two identities the
kernels are built on, and the inputs their tests share.

    erosion / dilation / opening / closing(m, c, n)   ndimage.binary_*(m, generate_binary_structure(3, c), iterations=n)
    fill_holes(m, c)                                  ndimage.binary_fill_holes(m, generate_binary_structure(3, c))
    min_size(m, k, c)                                 the components of at least k voxels: ndimage.label + bincount
    largest(m, c)                                     components_ref.largest
    chain(m, steps)                                   a list of (name, args) applied in order

    erosion_shifted / dilation_shifted(m, c, n)       AND / OR of the mask shifted by every offset of the structure, zero fill
    fill_holes_components(m, c)                       mask | the background components that touch no face
    per_class(label_map, C, fn)                       the recombination rule of PostProcess.per_class in numpy

All masks are uint8 0 / 1.
"""
import itertools

import numpy as np
from scipy import ndimage

import components_ref as CR

SHAPES = CR.SHAPES                                           # (17, 33, 70), (24, 40, 72), (5, 7, 130)
BOUNDARY_SHAPES = [(3, 1, 65), (2, 3, 64), (4, 5, 63), (6, 6, 129), (3, 4, 128), (2, 2, 1), (1, 1, 1)]     # Z around the 64-bit word
LONG_ROW = (16, 16, 512)                                     # 8 words per row
DENSITIES = (0.35, 0.7, 0.93)


def structure(c):
    return ndimage.generate_binary_structure(3, c)


def _u8(a):
    return np.asarray(a).astype(np.uint8)


def erosion(m, c=1, n=1):
    return _u8(ndimage.binary_erosion(np.asarray(m) != 0, structure(c), iterations=n))


def dilation(m, c=1, n=1):
    return _u8(ndimage.binary_dilation(np.asarray(m) != 0, structure(c), iterations=n))


def opening(m, c=1, n=1):
    return _u8(ndimage.binary_opening(np.asarray(m) != 0, structure(c), iterations=n))


def closing(m, c=1, n=1):
    return _u8(ndimage.binary_closing(np.asarray(m) != 0, structure(c), iterations=n))


def fill_holes(m, c=1):
    return _u8(ndimage.binary_fill_holes(np.asarray(m) != 0, structure(c)))


def min_size(m, k, c=3):
    labels, n = ndimage.label(np.asarray(m) != 0, structure(c))
    keep = np.bincount(labels.ravel(), minlength=n + 1) >= k
    keep[0] = False
    return _u8(keep[labels])


def largest(m, c=3):
    return CR.largest(m, c)[0]


OPS = {"erosion": erosion, "dilation": dilation, "opening": opening, "closing": closing, "fill_holes": fill_holes, "min_size": min_size,
       "largest": largest}


def chain(m, steps):
    for name, args in steps:
        m = OPS[name](m, *args)
    return _u8(m)


# ------------------------------------------------------------------------------------------------------------------- restatements
def shifted(m, d):
    """out[p] = m[p + d], 0 where p + d lies outside the volume"""
    out = np.zeros_like(m)
    src = tuple(slice(max(k, 0), s + min(k, 0)) for k, s in zip(d, m.shape))
    dst = tuple(slice(max(-k, 0), s + min(-k, 0)) for k, s in zip(d, m.shape))
    out[dst] = m[src]
    return out


def offsets(c):
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if sum(map(abs, d)) <= c]


def erosion_shifted(m, c=1, n=1):
    m = _u8(np.asarray(m) != 0)
    for _ in range(n):
        m = np.bitwise_and.reduce([shifted(m, d) for d in offsets(c)])
    return m


def dilation_shifted(m, c=1, n=1):
    m = _u8(np.asarray(m) != 0)
    for _ in range(n):
        m = np.bitwise_or.reduce([shifted(m, d) for d in offsets(c)])
    return m


def fill_holes_components(m, c=1):
    m = np.asarray(m) != 0
    labels, n = ndimage.label(~m, structure(c))
    face = np.zeros(m.shape, bool)
    for axis in range(3):
        for side in (0, -1):
            idx = [slice(None)] * 3
            idx[axis] = side
            face[tuple(idx)] = True
    open_ = np.zeros(n + 1, bool)
    open_[np.unique(labels[face])] = True
    open_[0] = True                                          # label 0 is the mask itself
    return _u8(m | ~open_[labels])


def per_class(label_map, num_classes, fn):
    """fn(mask) -> mask per class 1..C-1; a voxel keeps its value when that class's processed mask holds it, else it takes the
    smallest class whose processed mask holds it, else 0"""
    label_map = np.asarray(label_map)
    masks = {c: fn(_u8(label_map == c)) != 0 for c in range(1, num_classes)}
    out = np.zeros(label_map.shape, np.uint8)
    for c in range(num_classes - 1, 0, -1):
        out[masks[c]] = c                                    # descending: the smallest class is written last
    for c in range(1, num_classes):
        own = masks[c] & (label_map == c)
        out[own] = c
    return out


# ------------------------------------------------------------------------------------------------------------------- inputs
def smooth_mask(shape, density, seed):
    """Gaussian-smoothed noise (sigma 1.5) thresholded to `density`, plus 2 % speckle"""
    rng = np.random.default_rng(seed)
    x = ndimage.gaussian_filter(rng.standard_normal(shape), 1.5, mode="nearest")
    m = x >= np.quantile(x, 1.0 - density)
    return _u8(m | (rng.random(shape) < 0.02))


def random_batch(shape):
    """one volume per density of DENSITIES"""
    return np.stack([smooth_mask(shape, d, 1000 * i + sum(shape)) for i, d in enumerate(DENSITIES)])


def corners(shape):
    m = np.zeros(shape, np.uint8)
    for c in itertools.product((0, -1), repeat=3):
        m[c] = 1
    return m


def box(shape, zlo=None, zhi=None):
    """(lo, hi) per axis of the solid box the hollow cases are cut from: one voxel off every x / y face, z in [zlo, zhi)"""
    X, Y, Z = shape
    zlo = 2 if zlo is None else zlo
    zhi = min(Z - 2, zlo + 9) if zhi is None else zhi
    assert X >= 5 and Y >= 5 and zhi - zlo >= 3 and zlo >= 2 and zhi <= Z - 1
    return (1, 1, zlo), (X - 1, Y - 1, zhi)


def solid_box(shape, zlo=None, zhi=None):
    lo, hi = box(shape, zlo, zhi)
    m = np.zeros(shape, np.uint8)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = 1
    return m


def hollow_box(shape, zlo=None, zhi=None):
    """a one-voxel shell around a cavity: filled at every connectivity"""
    lo, hi = box(shape, zlo, zhi)
    m = solid_box(shape, zlo, zhi)
    m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = 0
    return m


def hollow_box_tunnel(shape):
    """the cavity reaches the face z = 0 through a straight one-voxel tunnel: not filled at any connectivity"""
    lo, _ = box(shape)
    m = hollow_box(shape)
    m[lo[0] + 1, lo[1] + 1, :lo[2] + 1] = 0
    return m


def hollow_box_diagonal(shape):
    """the only opening is the shell's edge voxel diagonally (in x and y) off the cavity's first voxel: the cavity is closed under
    connectivity 1 (filled) and open under 2 and 3 (not filled)"""
    lo, _ = box(shape)
    m = hollow_box(shape)
    m[lo[0], lo[1], lo[2] + 1] = 0
    return m


def straddle(shape):
    """a cavity across z = 63 / 64, the boundary of two words"""
    assert shape[2] >= 70
    return hollow_box(shape, 60, 68)


def two_blobs(shape, k):
    """a line of k - 1 voxels and a line of k voxels along z, apart"""
    X, Y, Z = shape
    assert k + 1 <= Z and X >= 3
    m = np.zeros(shape, np.uint8)
    m[0, 0, 1:k] = 1
    m[X - 1, Y - 1, Z - k:] = 1
    return m


def face_block(shape):
    """two blocks one voxel apart that touch the faces x = 0, y = 0 and z = Z - 1: a closing bridges the gap and loses the layers on
    the faces to its erosion half"""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    m[0:min(4, X), 0:min(5, Y), Z - 8:Z - 5] = 1
    m[0:min(4, X), 0:min(5, Y), Z - 4:Z] = 1
    return m


def named_batch(shape):
    """full then empty, corner then frame (components_ref), the eight corners"""
    n = CR.named(shape)
    return np.stack([n["full"], n["empty"], n["corner"], n["frame"], corners(shape)])


HOLE_NAMES = ["hollow_box", "hollow_box_tunnel", "hollow_box_diagonal", "straddle", "face_block"]


def hole_batch(shape):
    """HOLE_NAMES in order; `straddle` is the plain hollow box again where Z is too short for it"""
    return np.stack([hollow_box(shape), hollow_box_tunnel(shape), hollow_box_diagonal(shape),
                     straddle(shape) if shape[2] >= 70 else hollow_box(shape), face_block(shape)])
