"""scipy restatements of the component kernels (csrc/components.hip) and the named inputs their tests share.

    label(vol, connectivity)            (labels int32, n): scipy.ndimage.label with generate_binary_structure(3, connectivity)
    roots(labels, n)                    int32 volume: 0 for background, else 1 + the smallest linear index of the voxel's component
    label_by_value(vol, connectivity)   (labels, n, roots) of an integer map: every value 1..255 labelled on its own, all components
                                        numbered together by their roots (skimage.measure.label's numbering on an integer map)
    flood_by_value(vol, connectivity)   the same partition by a brute-force flood fill, for small maps
    largest(vol, connectivity)          (mask uint8, size) of the largest component of vol != 0, the first in raster order among equals
    largest_per_class(vol, C, conn)     uint8 map keeping the largest component of each value 1..C-1
    named(shape)                        name -> binary uint8 volume
"""
import itertools

import numpy as np
from scipy import ndimage

SHAPES = [(17, 33, 70), (24, 40, 72), (5, 7, 130)]          # odd sizes, no multiple of the 64-wide z segment, more than one segment


def structure(connectivity):
    return ndimage.generate_binary_structure(3, connectivity)


def label(vol, connectivity):
    labels, n = ndimage.label(np.asarray(vol) != 0, structure(connectivity))
    return labels.astype(np.int32), int(n)


def roots(labels, n):
    labels = np.asarray(labels)
    out = np.zeros(labels.shape, np.int32)
    if n:
        first = np.asarray(ndimage.minimum(np.arange(labels.size).reshape(labels.shape), labels, np.arange(1, n + 1)))
        out[labels > 0] = first[labels[labels > 0] - 1] + 1
    return out


def label_by_value(vol, connectivity):
    vol = np.asarray(vol)
    root = np.zeros(vol.shape, np.int32)
    for v in np.unique(vol):
        if 1 <= v <= 255:
            lab, n = label(vol == v, connectivity)
            root += roots(lab, n)                             # the values' supports are disjoint
    order = np.unique(root[root > 0])                        # a component's root is its first voxel in raster order
    labels = np.zeros(vol.shape, np.int32)
    labels[root > 0] = np.searchsorted(order, root[root > 0]) + 1
    return labels, len(order), root


def neighbours(connectivity):
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(map(abs, d)) <= connectivity]


def flood_by_value(vol, connectivity):
    """labels in raster order of each component's first voxel: a stack-based flood fill from every unlabelled foreground voxel"""
    vol = np.asarray(vol)
    labels = np.zeros(vol.shape, np.int32)
    offs = neighbours(connectivity)
    n = 0
    for start in np.ndindex(vol.shape):
        if not 1 <= vol[start] <= 255 or labels[start]:
            continue
        n += 1
        labels[start] = n
        stack = [start]
        while stack:
            p = stack.pop()
            for d in offs:
                q = tuple(a + b for a, b in zip(p, d))
                if all(0 <= c < s for c, s in zip(q, vol.shape)) and vol[q] == vol[start] and not labels[q]:
                    labels[q] = n
                    stack.append(q)
    return labels, n


def largest(vol, connectivity=3):
    labels, n = label(vol, connectivity)
    if n == 0:
        return np.zeros(labels.shape, np.uint8), 0
    counts = np.bincount(labels.ravel())[1:]
    return (labels == np.argmax(counts) + 1).astype(np.uint8), int(counts.max())


def largest_per_class(vol, num_classes, connectivity=3):
    vol = np.asarray(vol)
    out = np.zeros(vol.shape, np.uint8)
    for c in range(1, num_classes):
        out[largest(vol == c, connectivity)[0] != 0] = c
    return out


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def serpentine(shape):
    """one-voxel-wide lines through the whole volume, one component under connectivity 1: every second row of every second x plane,
    consecutive rows linked by one voxel at alternating z ends, consecutive planes by one voxel at alternating y ends"""
    X, Y, Z = shape
    m = np.zeros(shape, np.uint8)
    for i, x in enumerate(range(0, X, 2)):
        for j, y in enumerate(range(0, Y, 2)):
            m[x, y, :] = 1
            if y + 2 < Y:
                m[x, y + 1, -1 if j % 2 == 0 else 0] = 1
        if x + 2 < X:
            last_y = ((Y - 1) // 2) * 2
            m[x + 1, last_y if i % 2 == 0 else 0, 0] = 1
    return m


def frame(shape):
    """the twelve edges of the volume"""
    m = np.zeros(shape, np.uint8)
    for a in (0, -1):
        for b in (0, -1):
            m[a, b, :] = 1
            m[a, :, b] = 1
            m[:, a, b] = 1
    return m


def two_cubes(shape, edge=3):
    """two cubes of equal size, far apart: the earlier in raster order wins the tie"""
    m = np.zeros(shape, np.uint8)
    m[1:1 + edge, 1:1 + edge, 2:2 + edge] = 1
    m[-1 - edge:-1, -1 - edge:-1, -2 - edge:-2] = 1
    return m


def pairs(shape, offset):
    """voxel pairs offset by `offset`, the pairs far from each other"""
    m = np.zeros(shape, np.uint8)
    for base in ((1, 1, 1), (1, 1, 62), (1, 1, 66), (shape[0] - 3, shape[1] - 3, shape[2] - 3)):
        m[base] = 1
        m[tuple(b + o for b, o in zip(base, offset))] = 1
    return m


def checkerboard(shape):
    x, y, z = np.indices(shape)
    return ((x + y + z) % 2 == 0).astype(np.uint8)


def faces(shape):
    """the planes z = 0 and z = Z - 1, two components: the end of a row and the start of the next are neighbours in memory, as are
    the last voxel of a volume and the first of the next in a batch, so a wrap around a face or a leak between volumes joins them"""
    m = np.zeros(shape, np.uint8)
    m[:, :, 0] = 1
    m[:, :, -1] = 1
    return m


def named(shape):
    corner = np.zeros(shape, np.uint8)
    corner[-1, -1, -1] = 1
    return {
        "pair_110": pairs(shape, (1, 1, 0)), "pair_111": pairs(shape, (1, 1, 1)), "checkerboard": checkerboard(shape),
        "serpentine": serpentine(shape), "full": np.ones(shape, np.uint8), "empty": np.zeros(shape, np.uint8), "corner": corner,
        "frame": frame(shape), "two_cubes": two_cubes(shape), "faces": faces(shape),
    }


NAMES = ["pair_110", "pair_111", "checkerboard", "serpentine", "full", "empty", "corner", "frame", "two_cubes", "faces"]
