"""numpy restatement of the preprocessing kernels (csrc/resample.hip, preprocessing.py) and the inputs their tests share.

    axis_coords(n_in, n_out)             source coordinate of every output index along one axis, as scipy.ndimage.zoom takes it with
                                         grid_mode=False: double(i) * (double(n_in - 1) / double(n_out - 1)), 0 when n_out == 1
    zoom(x, target, order, norm, out_dtype)   scipy.ndimage.zoom(x, [t / s], order, mode="constant", cval=0) for order 0 and 1 over the
                                         last three axes; norm: a record of norm_record, applied to every tap value on load
    volume_stats(x)                      what dycon_volume_stats returns for one volume, from numpy fp64
    device_stats(x)                      the same with the kernels' order of additions: mean and std bit for bit
    norm_record(stats)                   (apply_z, mean32, std32, apply_mm, lo32, hi32): normalize_image's scalars without a second
                                         reduction, the edge rules included
    normalize_apply(x, rec)              the reference's two fp32 expressions
    normalize_image(x)                   normalize_apply(x, norm_record(volume_stats(x)))
    normalize_image64(x)                 the reference function with every operation in fp64 (the tolerance's yardstick)
    preprocess(image, label, target, thr)   (image fp32, label uint8) of process_brats_case (thr 0) / process_isles_bids_case (thr 0.5)
    golden_volumes(), SPLIT_NAMES, SHAPE_PAIRS

Order 0 is scipy bit for bit; order 1 differs from scipy by its summation order only (tests/test_preprocess_cpu.py measures it); the
device path is held to these functions bit for bit (tests/test_preprocess_gpu.py).
"""
import numpy as np

#: (input shape, output shape) of the zoom tests, CPU and GPU: ties at x.5 (4 -> 11), mixed up- and down-sampling, identity, unit axes
SHAPE_PAIRS = (((4, 11, 6), (11, 4, 16)), ((5, 7, 4), (9, 11, 6)), ((13, 9, 11), (7, 6, 5)), ((24, 24, 31), (19, 19, 13)),
               ((12, 10, 7), (9, 13, 10)), ((31, 17, 9), (12, 33, 8)), ((2, 2, 2), (7, 5, 3)), ((9, 9, 9), (2, 2, 2)),
               ((6, 7, 13), (6, 7, 13)), ((5, 1, 4), (9, 1, 6)), ((5, 6, 4), (1, 6, 4)), ((1, 6, 4), (3, 6, 4)))
#: three more for the CPU comparison with scipy (15 in all): a long axis, a prime pair, 2 -> 1
EXTRA_PAIRS = (((3, 5, 40), (8, 2, 64)), ((17, 19, 23), (29, 13, 31)), ((2, 3, 2), (1, 7, 1)))


def zoom_input(shape, seed=0):
    """the volumes the zoom tests resample: unit-normal float64, cast by the test"""
    return np.random.default_rng([seed, *shape]).standard_normal(shape)


def axis_coords(n_in, n_out):
    if n_out == 1:
        return np.zeros(1, np.float64)
    return np.arange(n_out, dtype=np.float64) * (np.float64(n_in - 1) / np.float64(n_out - 1))


def axis_nearest(n_in, n_out):
    """order 0: floor(c + 0.5), clamped to the last voxel"""
    return np.minimum(np.floor(axis_coords(n_in, n_out) + 0.5).astype(np.int64), n_in - 1)


def axis_linear(n_in, n_out):
    """order 1: (i0, i1, w0, w1) with f = floor(c), t = c - f, w0 = 1 - t, w1 = t; a tap beyond the last voxel is clamped"""
    c = axis_coords(n_in, n_out)
    f = np.floor(c)
    t = c - f
    i0 = np.minimum(f.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), 1.0 - t, t


def normalize_apply(x, rec):
    """x fp32 -> fp32, every operation rounded in fp32 as numpy does on float32 arrays"""
    apply_z, mean32, std32, apply_mm, lo32, hi32 = rec
    x = np.asarray(x, dtype=np.float32)
    if apply_z:
        with np.errstate(all="ignore"):
            x = np.where(x > 0, (x - np.float32(mean32)) / np.float32(std32), np.float32(0))
    if apply_mm:
        x = (x - np.float32(lo32)) / (np.float32(hi32) - np.float32(lo32))
    return x.astype(np.float32)


def volume_stats(x):
    x = np.asarray(x, dtype=np.float32)
    pos = x[x > 0].astype(np.float64)
    n = pos.size
    mean = pos.sum() / n if n else 0.0
    std = np.sqrt(((pos - mean) ** 2).sum() / n) if n else 0.0
    return {"n_pos": n, "mean": float(mean), "std": float(std), "min_pos": np.float32(pos.min() if n else 0),
            "max_pos": np.float32(pos.max() if n else 0), "min_all": np.float32(x.min()), "max_all": np.float32(x.max()),
            "any_nonpos": int(n < x.size)}


STATS_THREADS, STATS_MAX_GROUPS, STATS_GROUP_VOXELS = 256, 1024, 4096      # RS_THREADS, RS_MAX_GROUPS, RS_GROUP_VOXELS


def _device_sum(terms):
    """the fp64 sum of one value per voxel (0.0 where the voxel does not count: adding it changes nothing) in the order of
    csrc/resample.hip: workgroup g, thread t takes the quads g * 256 + t, + G * 256, ... and adds their voxels one by one; a
    64-lane xor butterfly (32, 16, ..., 1); the four waves in order.  The G partials are summed the same way by one workgroup: thread
    t adds partials t, t + 256, ... in index order, then the butterfly and the waves"""
    V = terms.size
    G = int(min(max(-(-V // STATS_GROUP_VOXELS), 1), STATS_MAX_GROUPS))
    lanes = G * STATS_THREADS
    K = -(-V // (4 * lanes))
    a = np.zeros(K * lanes * 4, np.float64)
    a[:V] = terms
    a = a.reshape(K, lanes, 4)
    acc = np.zeros(lanes, np.float64)
    for k in range(K):
        for e in range(4):
            acc = acc + a[k, :, e]
    part = _group_sums(acc.reshape(G, STATS_THREADS))
    padded = np.zeros(-(-G // STATS_THREADS) * STATS_THREADS, np.float64)
    padded[:G] = part
    acc = np.zeros(STATS_THREADS, np.float64)
    for row in padded.reshape(-1, STATS_THREADS):
        acc = acc + row
    return _group_sums(acc[None])[0]


def _group_sums(v):
    """(groups, 256) per-thread values -> the workgroups' sums: a 64-lane xor butterfly per wave, then the four waves in order"""
    v = v.reshape(len(v), STATS_THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ o]
    out = np.zeros(len(v), np.float64)
    for w in range(STATS_THREADS // 64):
        out = out + v[:, w, 0]
    return out


def device_stats(x):
    st = volume_stats(x)
    if st["n_pos"]:
        x = np.asarray(x, dtype=np.float32).reshape(-1)
        pos, n = x > 0, np.float64(st["n_pos"])
        mean = _device_sum(np.where(pos, x.astype(np.float64), 0.0)) / n
        d = x.astype(np.float64) - mean
        st["mean"], st["std"] = float(mean), float(np.sqrt(_device_sum(np.where(pos, d * d, 0.0)) / n))
    return st


def norm_record(st):
    mean32, std32 = np.float32(st["mean"]), np.float32(st["std"])
    apply_z = int(st["n_pos"] > 0 and std32 > 0)
    if apply_z:
        lo32, hi32 = ((np.float32(st[k]) - mean32) / std32 for k in ("min_pos", "max_pos"))
        if st["any_nonpos"]:
            lo32, hi32 = min(lo32, np.float32(0)), max(hi32, np.float32(0))
    else:
        lo32, hi32 = np.float32(st["min_all"]), np.float32(st["max_all"])
    return (apply_z, mean32, std32, int(hi32 > lo32), np.float32(lo32), np.float32(hi32))


def normalize_image(x):
    x = np.asarray(x, dtype=np.float32)
    return normalize_apply(x, norm_record(volume_stats(x)))


def normalize_image64(x):
    """the reference's normalize_image, its branches and order of operations, with fp64 arithmetic on the float32-cast input"""
    image = np.asarray(x, dtype=np.float32).astype(np.float64)
    if np.all(image == 0):
        return image
    mask = image > 0
    if np.any(mask):
        mean, std = image[mask].mean(), image[mask].std()
        if std > 0:
            image = np.where(mask, (image - mean) / std, 0.0)
    lo, hi = image.min(), image.max()
    if hi > lo:
        image = (image - lo) / (hi - lo)
    return image


def zoom(x, target, order, norm=None, out_dtype=None):
    """x: (..., X, Y, Z); the last three axes are resampled to `target`.  order 0 keeps the dtype (fp32 with a norm record); order 1
    accumulates the eight taps in fp64 in the order x, y, z with z fastest, each weight (wx * wy) * wz, and rounds once to
    out_dtype (default: the input's float dtype, as scipy does)"""
    x = np.asarray(x)
    load = (lambda v: normalize_apply(v, norm)) if norm is not None else (lambda v: v)
    (X, Y, Z), (Xo, Yo, Zo) = x.shape[-3:], target
    if order == 0:
        ix, iy, iz = axis_nearest(X, Xo), axis_nearest(Y, Yo), axis_nearest(Z, Zo)
        return load(x[..., ix[:, None, None], iy[None, :, None], iz[None, None, :]])
    assert order == 1
    ax, ay, az = axis_linear(X, Xo), axis_linear(Y, Yo), axis_linear(Z, Zo)
    acc = np.zeros(x.shape[:-3] + tuple(target), np.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                w = (ax[2 + dx][:, None, None] * ay[2 + dy][None, :, None]) * az[2 + dz][None, None, :]
                v = load(x[..., ax[dx][:, None, None], ay[dy][None, :, None], az[dz][None, None, :]])
                acc = acc + w * v.astype(np.float64)
    return acc.astype(out_dtype if out_dtype is not None else (x.dtype if x.dtype.kind == "f" else np.float64))


def preprocess(image, label, target, thr):
    """normalise, binarise the label (> thr), zoom the image with order 1 and the label with order 0, `> 0.5`"""
    image = np.asarray(image, dtype=np.float32)
    lab = (np.asarray(label) > thr).astype(np.uint8)
    st = volume_stats(image)
    return zoom(image, target, 1, norm=norm_record(st)), (zoom(lab, target, 0) > 0.5).astype(np.uint8)


# ------------------------------------------------------------------ the inputs of tests/golden/preprocess.npz
GOLDEN_TARGET = (19, 16, 6)
SPLIT_NAMES = tuple(f"sub-strokecase{n:04d}" for n in (1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 250))


def golden_volumes():
    """name -> (image float64 as nibabel's get_fdata hands it over, label float64).  mri: a positive blob in a zero background, the
    ordinary case; zero: all zero (returned unchanged); nopos: no positive voxel (the z-score is skipped, the raw values are
    min-maxed); const: one positive value and zeros (std == 0: likewise); flat: one positive value everywhere (hi == lo: the min-max
    is skipped too)"""
    rng = np.random.default_rng(2019)
    shape = (24, 20, 13)
    g = np.stack(np.meshgrid(*(np.linspace(-1, 1, n) for n in shape), indexing="ij"))
    head = (g ** 2).sum(0) < 0.8
    mri = np.where(head, np.round(400 + 150 * rng.standard_normal(shape)).clip(1, None), 0.0)
    seg = np.where(((g - 0.2) ** 2).sum(0) < 0.15, rng.choice([1.0, 2.0, 4.0], size=shape), 0.0)
    const = np.where(head, 3.0, 0.0)
    return {"mri": (mri, seg), "zero": (np.zeros(shape), seg), "nopos": (0.0 - np.abs(np.round(rng.standard_normal(shape), 2)), seg),
            "const": (const, seg), "flat": (np.full(shape, 3.0), (seg > 1).astype(np.float64))}


def stats_volumes():
    """name -> fp32 volume of the statistics tests: three sizes (the last one larger than one workgroup's share of 4096 voxels) with
    about half the voxels > 0, and the value patterns that take normalize_image's edge rules"""
    rng = np.random.default_rng(22)
    out = {f"normal{'x'.join(map(str, s))}": (100 * rng.standard_normal(s) + 30).astype(np.float32) for s in ((5, 7, 4), (17, 9, 33), (40, 40, 30))}
    out["brain"] = np.where(rng.random((40, 40, 30)) < 0.4, np.round(400 + 150 * rng.standard_normal((40, 40, 30))).clip(1, None), 0).astype(np.float32)
    small = (5, 7, 4)
    one = np.zeros(small, np.float32)
    one[2, 3, 1] = 7.5
    out.update(zero=np.zeros(small, np.float32), nopos=(0.0 - np.abs(rng.standard_normal(small))).astype(np.float32), one=one,
               equal=np.full((17, 9, 33), 0.1, np.float32))
    return out
