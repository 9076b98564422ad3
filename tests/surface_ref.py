"""numpy restatements of the surface-distance kernels (csrc/surface.hip) and the input set their tests share.

    border6(m)            m & ~erode6(m), the outside of the volume counting as background
    edt2_separable(b)     exact integer squared Euclidean distance to the nearest voxel of b, three separable brute-force passes
    hists(a, b)           (hist (2, nbins) int64, nborder (2,) int64) of one binary pair
    cases(shape)          the named (a, b) mask pairs of one shape
"""
import numpy as np

FAR = 1 << 29            # the kernels' sentinel: + 2 * 511^2 stays below 2^31

SHAPES = [(17, 33, 70), (24, 40, 72), (5, 7, 130),          # odd sizes, no multiple of the 64-wide z tile, more than one tile
          (3, 5, 300), (4, 300, 3), (300, 4, 3),            # each axis in turn longer than a 256-lane workgroup and a 64-lane wave
          (1, 1, 9)]


def border6(m):
    m = np.asarray(m).astype(bool)
    inner = m.copy()
    for ax in range(m.ndim):
        pad = [(0, 0)] * m.ndim
        pad[ax] = (1, 1)
        p = np.pad(m, pad, constant_values=False)
        n = m.shape[ax]
        inner &= np.take(p, np.arange(0, n), axis=ax) & np.take(p, np.arange(2, n + 2), axis=ax)
    return m & ~inner


def edt2_separable(border):
    """int64 squared distance of every voxel to the nearest True voxel of `border`; >= FAR everywhere when there is none"""
    d = np.where(np.asarray(border).astype(bool), 0, FAR).astype(np.int64)
    for ax in range(d.ndim - 1, -1, -1):                     # innermost axis first, as the kernels
        g = np.moveaxis(d, ax, 0)
        n = g.shape[0]
        idx = np.arange(n).reshape((n,) + (1,) * (g.ndim - 1))
        out = g.copy()
        for j in range(n):
            np.minimum(out, g[j][None] + (idx - j) ** 2, out=out)
        d = np.moveaxis(out, 0, ax)
    return d


def nbins_of(shape):
    return int(sum((n - 1) ** 2 for n in shape)) + 1


def hists(a, b):
    a, b = np.asarray(a).astype(bool), np.asarray(b).astype(bool)
    ba, bb = border6(a), border6(b)
    nbins = nbins_of(a.shape)
    hist = np.zeros((2, nbins), np.int64)
    if ba.any() and bb.any():
        hist[0] = np.bincount(edt2_separable(bb)[ba], minlength=nbins)
        hist[1] = np.bincount(edt2_separable(ba)[bb], minlength=nbins)
    return hist, np.array([ba.sum(), bb.sum()], np.int64)


def _blobs(shape, seed):
    """seeded smoothed noise, the top 15 % of the voxels"""
    from scipy import ndimage
    x = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 2.0, mode="nearest")
    return x >= np.quantile(x, 0.85)


def cases(shape):
    """name -> (a, b) boolean masks of `shape`, both non-empty"""
    seed = sum(n * k for n, k in zip(shape, (1, 1000, 1000000)))
    a, b = _blobs(shape, seed), _blobs(shape, seed + 1)
    out = {"blobs": (a, b)}
    fa, fb = a.copy(), b.copy()
    fa[0], fb[..., -1] = True, True                          # a whole face of the volume: the border_value = 0 rule
    out["face"] = (fa, fb)
    ca, cb = np.zeros(shape, bool), np.zeros(shape, bool)
    ca[0, 0, 0], cb[-1, -1, -1] = True, True                 # opposite corners: the last bin
    out["corners"] = (ca, cb)
    one = np.zeros(shape, bool)
    one[shape[0] // 2, shape[1] // 3, (2 * shape[2]) // 3] = True
    out["full_vs_voxel"] = (np.ones(shape, bool), one)
    out["identical"] = (a, a.copy())                         # everything in bin 0
    pa, pb = np.zeros(shape, bool), np.zeros(shape, bool)
    pa[:, :, shape[2] // 3], pb[shape[0] // 2] = True, True  # 1-voxel-thick plates
    out["plates"] = (pa, pb)
    return out


ALL_CASES = [(shape, name) for shape in SHAPES for name in ("blobs", "face", "corners", "full_vs_voxel", "identical", "plates")]
