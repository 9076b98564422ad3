"""Shared cases of the warp / filter tests (test_warp_cpu.py, test_warp_gpu.py, test_filters_*.py, test_guard_warp_gpu.py): the
small cache, hand-built plans that cover every rot90 count with every flip, and the bit-level comparisons."""
import numpy as np

import device_cache_ref as R
from dycon_paper_replication_amd.dataloaders.device_warp import WARP_PLAN_DTYPE, affine_of

SHAPES = [(11, 10, 9), (20, 17, 12), (8, 8, 5)]      # the last case is smaller than the patch
PATCH = (8, 8, 6)
KINDS = ("shift", "scale", "general", "general_disp")
K_FLIP = [(k, f) for k in range(4) for f in (-1, 0, 1)]      # every rot90 count with every flip: 12 samples

# (modes, shape, sigma) of the Gaussian cases: radius above the axis lengths 9 and 7; an axis of length 1 and a row longer than a
# wave; a skipped axis, ragged tiles and a row over 128; the largest radius (64: sigma 16 at truncate 4) on axes shorter than it
GAUSS_CASES = [((2, 13, 9, 7), (0.7, 1.3, 2.1)), ((2, 13, 9, 7), (3.0, 0.5, 1.5)), ((1, 1, 5, 70), (1, 1, 2)),
               ((1, 33, 34, 130), (2.5, 0, 2.5)), ((1, 5, 40, 3), (16, 1, 16))]
GAUSS_MODES = ("reflect", "constant", "nearest")


def cases(seed=31):
    return R.make_cases(SHAPES, seed, image_dtype=np.float32)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def ulp_distance(a, b):
    """distance in float32 steps between two finite float32 arrays"""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def make_plan(kind, seed, B=len(K_FLIP)):
    """-> (plan, displacement or None): B hand-built records, sample n with (k, flip) = K_FLIP[n % 12] and case n % 3.
    shift: the identity with an integer shift of the crop; scale: a diagonal matrix, 0.8..1.25 per axis; general: scale 0.8..1.25
    and rotations up to 20 degrees about all three axes; general_disp: the same with a displacement of a few voxels, read by two
    records out of three"""
    rng = np.random.default_rng(seed)
    plan = np.zeros(B, dtype=WARP_PLAN_DTYPE)
    P = np.asarray(PATCH)
    for n in range(B):
        rec = plan[n]
        case = n % len(SHAPES)
        shape = np.asarray(SHAPES[case])
        origin = rng.integers(np.minimum(shape - P, 0) - 1, np.maximum(shape - P, 0) + 2)
        rec["case"], rec["origin"], rec["patch"] = case, origin, PATCH
        rec["k"], rec["flip_axis"] = K_FLIP[n % len(K_FLIP)]
        rec["warp"], rec["scale"], rec["gain"], rec["gamma"] = 1, 1.0, 1.0, 1.0
        if kind == "shift":
            rec["m"], rec["off"] = np.eye(3).reshape(9), origin
        elif kind == "scale":
            m = np.diag(rng.uniform(0.8, 1.25, 3))
            ctr = (P - 1) / 2
            rec["m"], rec["off"] = m.reshape(9), (origin + ctr) - m @ ctr
        else:
            scale, angles = rng.uniform(0.8, 1.25), rng.uniform(-20, 20, 3)
            m, off = affine_of(scale, angles, origin, PATCH)
            rec["m"], rec["off"], rec["scale"], rec["angles"] = m.reshape(9), off, scale, angles
            if kind == "general_disp":
                rec["elastic"] = int(n % 3 != 2)
    disp = None
    if kind == "general_disp":
        disp = (2.0 * rng.standard_normal((B, 3) + PATCH)).astype(np.float32)
    return plan, disp


def check_band(out):
    """a case is neither all zeros nor all interior: at least 20 % of its output voxels inside the source, at least 5 % outside"""
    frac = float(out["in_source"].mean())
    assert 0.20 <= frac <= 0.95, frac
    assert np.count_nonzero(out["image"]) >= 0.20 * out["image"].size
    return frac
