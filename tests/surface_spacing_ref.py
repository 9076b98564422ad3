"""numpy restatement of the weighted surface-distance kernels (csrc/surface_spacing.hip); inputs and shapes are those of surface_ref.

    border(m, connectivity)               m ^ erode(m) with 6, 18 or 26 neighbours, the outside of the volume counting as background
    cost_separable(b, spacing)            fp64 min over the voxels of b of fl(fl(fl(wz dz^2) + fl(wy dy^2)) + fl(wx dx^2)), w = s * s
    distances(a, b, spacing, conn)        (d_ab, d_ba): sqrt(cost) from the border voxels of a to the border of b, and back
    metrics(a, b, spacing, conn, q)       the (5,) row of surface.surface_metrics
"""
import numpy as np


def normalise(spacing):
    if spacing is None:
        return (1.0, 1.0, 1.0)
    sp = np.asarray(spacing, np.float64)
    return tuple(float(v) for v in (np.repeat(sp, 3) if sp.ndim == 0 else sp))


def border(m, connectivity=1):
    m = np.asarray(m).astype(bool)
    p = np.pad(m, 1, constant_values=False)
    inner = m.copy()
    X, Y, Z = m.shape
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if 1 <= abs(dx) + abs(dy) + abs(dz) <= connectivity:
                    inner &= p[1 + dx:1 + dx + X, 1 + dy:1 + dy + Y, 1 + dz:1 + dz + Z]
    return m & ~inner


def cost_separable(b, spacing):
    """three separable brute-force passes, innermost axis first as the kernels; numpy rounds every product and sum to fp64 and fuses
    nothing, so the value is the cost formula's; +inf everywhere when b is empty"""
    d = np.where(np.asarray(b).astype(bool), 0.0, np.inf)
    for ax in (2, 1, 0):
        w = np.float64(spacing[ax]) * np.float64(spacing[ax])
        g = np.moveaxis(d, ax, 0)
        n = g.shape[0]
        idx = np.arange(n).reshape((n, 1, 1))
        out = g.copy()
        for j in range(n):
            np.minimum(out, g[j][None] + w * ((idx - j) ** 2).astype(np.float64), out=out)
        d = np.moveaxis(out, 0, ax)
    return d


def distances(a, b, spacing=None, connectivity=1):
    sp = normalise(spacing)
    ba, bb = border(a, connectivity), border(b, connectivity)
    return np.sqrt(cost_separable(bb, sp)[ba]), np.sqrt(cost_separable(ba, sp)[bb])


def metrics(a, b, spacing=None, connectivity=1, q=95.0):
    d_ab, d_ba = distances(a, b, spacing, connectivity)
    out = np.array([np.nan, np.nan, np.nan, d_ab.size, d_ba.size])
    if d_ab.size and d_ba.size:
        out[:3] = np.percentile(np.hstack((d_ab, d_ba)), q), d_ab.mean(), d_ba.mean()
    return out
