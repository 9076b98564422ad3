"""Interpolating augmentations on the device-resident data path: affine and elastic warps, Gaussian blur, gain / bias / gamma.

    Warp(p_affine, scale, angles_deg, p_elastic, alpha, sigma)       what to draw for the geometry
    Intensity(p_gain, gain, p_bias, bias, p_gamma, gamma, p_blur, blur_sigma, range)   what to draw for the values
    affine_of(scale, angles_deg, origin, patch)                       host: the fp64 matrix and offset of one sample
    draw_plan_warp(shapes, indices, patch_size, warp, intensity, ...) host: draw_plan plus the draws of Warp and Intensity
    warp_volume_host(a, matrix, offset, output_shape, order, displacement)    host: numpy twin of `warp_volume`
    apply_warp_plan_host(plan, images, labels, displacement, onehot)  host: numpy twin of `assemble_batch_warp`
    intensity_host(x, gain, bias, gamma, lo, hi)                      host: numpy twin of `intensity_augment`
    assemble_batch_warp(cache, plan, out, displacement, ...)          device: dycon_assemble_batch_warp, one launch per 16 samples
    elastic_field(B, patch, alpha, sigma, seed, offset)               device: smoothed Philox noise, (B, 3, w, h, d)
    warp_volume(t, matrix, offset, output_shape, order, displacement) device: affine_transform / map_coordinates of one volume
    intensity_augment(x, gain, bias, gamma, lo, hi, samples, out)     device: dycon_intensity_augment
    DeviceBatchLoader(..., warp, intensity, aug_seed)                 (device_cache.py) routes here

None of this is in the reference, whose loaders move voxels only; these are the usual augmentations of 3-D segmentation training,
computed as scipy computes them.

What is equal to what.  `warp_volume` is ``scipy.ndimage.affine_transform(a, matrix, offset, output_shape, order=order,
mode='constant', cval=0)`` and, with a displacement, ``map_coordinates(a, coordinates, order=order, mode='constant')`` at the
coordinates `source_coordinates` returns, bit for bit (order 1: fp32 and fp64; order 0 moves values).  The arithmetic is restated
operation by operation -- the coordinate ``c_d = (((0.0 + i0 * M[d,0]) + i1 * M[d,1]) + i2 * M[d,2]) + off_d`` in fp64, the inside
test ``0 <= c_d <= n_d - 1`` before any rounding, the weights ``w0 = 1 - t``, ``w1 = 1 - w0``, the eight corners summed from 0.0 as
``((v * wx) * wy) * wz`` -- which holds for the scipy this was checked against (1.15; fp64 outputs show every one of these choices,
fp32 outputs hide most of them behind their rounding); tests/test_warp_cpu.py compares the twins with the installed scipy directly and
tests/test_warp_gpu.py the kernels with the twins.  `assemble_batch_warp` applies the same rule to the crop of a plan record: the
image with order 1, the label with order 0, the patch index (a, b, z) behind the flip and the rot90 as the output index, so with
the identity it gives `assemble_batch`'s bits (but for a stored -0.0, which scipy's sum from 0.0 turns into +0.0).  The Gaussian
blur is `utils.filters.gaussian_filter` (scipy's bits); gain, bias and gamma are the fp64 expression of `intensity_host` rounded to fp32, bit for bit when gamma == 1 and within one fp32 ulp otherwise
(the device's ``pow`` is not libm's).  The elastic field is smoothed noise from the library's counter-based Philox stream, NOT
``np.random``'s: it is reproducible from (seed, offset) and equal to a host-drawn field in distribution only.

Draw order (`draw_plan_warp`), per sample, from ``np.random``: what `draw_plan` draws (crop, k, flip axis); with a Warp: random() for
p_affine, uniform(scale), three uniform(-angle, angle) for the axes 0, 1, 2, random() for p_elastic, uniform(alpha), uniform(sigma);
with an Intensity: random() and uniform() for gain, bias, gamma and the blur, in that order.  Every draw is made whether or not its
coin shows, so a sample always consumes the same number.

Out of scope: spline orders above 1, boundary modes other than 'constant', spacing-aware (millimetre) transforms, 2-D inputs,
different views for student and teacher.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib, ops
from ..utils.filters import gaussian_filter, workspace_bytes
from .device_augment import MAX_ONEHOT_CLASSES, ONEHOT_DTYPES
from .device_cache import JOBS_PER_LAUNCH, PLAN_DTYPE, _draw_record, _plan_args


@dataclass(frozen=True)
class Warp:
    """Geometry: with probability p_affine an isotropic scale drawn from `scale` (source voxels per output voxel: > 1 zooms out)
    and rotations by uniform(-a, a) degrees about the axes 0, 1, 2 for a in `angles_deg`, about the patch centre; with probability
    p_elastic a displacement field `elastic_field(alpha, sigma)` drawn from the two ranges (voxels)."""
    p_affine: float = 0.5
    scale: tuple = (0.8, 1.25)
    angles_deg: tuple = (15.0, 15.0, 15.0)
    p_elastic: float = 0.0
    alpha: tuple = (0.0, 200.0)
    sigma: tuple = (9.0, 13.0)

    def __post_init__(self):
        _prob(self.p_affine, "p_affine"), _prob(self.p_elastic, "p_elastic")
        _range(self.scale, "scale", positive=True), _range(self.alpha, "alpha"), _range(self.sigma, "sigma", positive=True)
        if len(self.angles_deg) != 3 or not all(np.isfinite(a) and a >= 0 for a in self.angles_deg):
            raise ValueError(f"angles_deg must be three non-negative angles, got {self.angles_deg}")
        if self.alpha[0] < 0:
            raise ValueError(f"alpha must be non-negative, got {self.alpha}")


@dataclass(frozen=True)
class Intensity:
    """Values: each with its own probability, a gain (contrast) and a bias (brightness) applied as x * gain + bias, a gamma applied
    to the result scaled into `range` (which it is clipped to), and a Gaussian blur of sigma drawn from `blur_sigma` (voxels)."""
    p_gain: float = 0.0
    gain: tuple = (0.75, 1.25)
    p_bias: float = 0.0
    bias: tuple = (-0.1, 0.1)
    p_gamma: float = 0.0
    gamma: tuple = (0.7, 1.5)
    p_blur: float = 0.0
    blur_sigma: tuple = (0.5, 1.0)
    range: tuple = (0.0, 1.0)

    def __post_init__(self):
        for n in ("p_gain", "p_bias", "p_gamma", "p_blur"):
            _prob(getattr(self, n), n)
        _range(self.gain, "gain"), _range(self.bias, "bias"), _range(self.gamma, "gamma", positive=True)
        _range(self.blur_sigma, "blur_sigma", positive=True)
        if not (len(self.range) == 2 and np.isfinite(self.range).all() and self.range[0] < self.range[1]):
            raise ValueError(f"range must be (lo, hi) with lo < hi, got {self.range}")


def _prob(p, name):
    if not 0 <= p <= 1:
        raise ValueError(f"{name} must be a probability, got {p}")


def _range(r, name, positive=False):
    if not (len(r) == 2 and np.isfinite(r).all() and r[0] <= r[1] and (not positive or r[0] > 0)):
        raise ValueError(f"{name} must be (low, high) with {'0 < ' if positive else ''}low <= high, got {r}")


#: PLAN_DTYPE's fields, then the geometry (warp: the sample is transformed by m row-major and off; scale, angles: what they were
#: formed from; elastic, alpha, sigma: the displacement field) and the values (identity: gain 1, bias 0, gamma 1, blur_sigma 0)
WARP_PLAN_DTYPE = np.dtype(PLAN_DTYPE.descr + [
    ("warp", "<i4"), ("m", "<f8", (9,)), ("off", "<f8", (3,)), ("scale", "<f8"), ("angles", "<f8", (3,)),
    ("elastic", "<i4"), ("alpha", "<f8"), ("sigma", "<f8"),
    ("gain", "<f8"), ("bias", "<f8"), ("gamma", "<f8"), ("blur_sigma", "<f8")])

# dycon_warp_job_t (include/dycon_hip.h), field for field
_WARP_JOB_DTYPE = np.dtype([("image_off", "<i8"), ("label_off", "<i8"), ("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"),
                            ("ox", "<i4"), ("oy", "<i4"), ("oz", "<i4"), ("k", "<i4"), ("flip_axis", "<i4"),
                            ("m", "<f8", (9,)), ("off", "<f8", (3,)), ("warp", "<i4"), ("elastic", "<i4")], align=True)


def affine_of(scale, angles_deg, origin, patch):
    """(m, off) of one sample: m = scale * Rz @ Ry @ Rx (rotations about the axes 2, 1, 0 by the angles in degrees), the map from a
    patch index to a stored coordinate, and off = (origin + (P - 1) / 2) - m @ ((P - 1) / 2) in fp64, so that the patch centre stays
    where the crop put it.  scale 1 and angles 0 give the identity and off = origin exactly."""
    ax, ay, az = (np.deg2rad(float(a)) for a in angles_deg)
    rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    rz = np.array([[np.cos(az), -np.sin(az), 0], [np.sin(az), np.cos(az), 0], [0, 0, 1]])
    m = float(scale) * (rz @ ry @ rx)
    ctr = (np.asarray(patch, dtype=np.float64) - 1) / 2
    off = (np.asarray(origin, dtype=np.float64) + ctr) - m @ ctr
    return m, off


def draw_plan_warp(shapes, indices, patch_size, warp=None, intensity=None, rot_flip=True, order="crop_rotflip"):
    """The plan of one batch with the draws of `warp` (a Warp or None) and `intensity` (an Intensity or None): a WARP_PLAN_DTYPE
    record per entry of `indices`.  Pure host code; consumes ``np.random`` in the order the module docstring gives.  With both None
    the draws are `draw_plan`'s and the records are identities."""
    patch = _plan_args(patch_size, rot_flip, False, order)
    plan = np.zeros(len(indices), dtype=WARP_PLAN_DTYPE)
    for n, idx in enumerate(indices):
        origin, k, axis = _draw_record(shapes[idx], patch, rot_flip, False, order)
        rec = plan[n]
        rec["case"], rec["origin"], rec["k"], rec["flip_axis"], rec["patch"] = idx, origin, k, axis, patch
        rec["scale"], rec["gain"], rec["gamma"] = 1.0, 1.0, 1.0
        rec["m"], rec["off"] = np.eye(3).reshape(9), origin
        if warp is not None:
            coin, scale = np.random.random(), np.random.uniform(*warp.scale)
            angles = [np.random.uniform(-a, a) for a in warp.angles_deg]
            if coin < warp.p_affine:
                m, off = affine_of(scale, angles, origin, patch)
                rec["warp"], rec["m"], rec["off"], rec["scale"], rec["angles"] = 1, m.reshape(9), off, scale, angles
            coin, alpha, sigma = np.random.random(), np.random.uniform(*warp.alpha), np.random.uniform(*warp.sigma)
            if coin < warp.p_elastic:
                rec["warp"], rec["elastic"], rec["alpha"], rec["sigma"] = 1, 1, alpha, sigma
        if intensity is not None:
            for name, p, rng in (("gain", intensity.p_gain, intensity.gain), ("bias", intensity.p_bias, intensity.bias),
                                 ("gamma", intensity.p_gamma, intensity.gamma),
                                 ("blur_sigma", intensity.p_blur, intensity.blur_sigma)):
                coin, value = np.random.random(), np.random.uniform(*rng)
                if coin < p:
                    rec[name] = value
    return plan


def _check_warp_plan(plan, ncases, onehot=None):
    """-> the patch of a well-formed WARP_PLAN_DTYPE plan; ValueError otherwise"""
    plan = np.asarray(plan)
    if plan.dtype != WARP_PLAN_DTYPE or plan.ndim != 1 or len(plan) == 0:
        raise ValueError("a plan is a non-empty 1-D array of WARP_PLAN_DTYPE records (draw_plan_warp)")
    patch = tuple(int(v) for v in plan["patch"][0])
    if (plan["patch"] != plan["patch"][0]).any() or min(patch) <= 0:
        raise ValueError("all samples of a batch share one positive patch size")
    if plan["case"].min() < 0 or plan["case"].max() >= ncases:
        raise ValueError(f"plan names case {plan['case'].max()} of {ncases}")
    if plan["k"].min() < 0 or plan["k"].max() > 3 or plan["flip_axis"].min() < -1 or plan["flip_axis"].max() > 1:
        raise ValueError("k must be in 0..3 and flip_axis in {-1, 0, 1}")
    if patch[0] != patch[1] and (plan["k"] & 1).any():
        raise ValueError(f"an odd k needs a square patch in the first two axes, got {patch[0]} x {patch[1]}")
    if not (np.isfinite(plan["m"]).all() and np.isfinite(plan["off"]).all()):
        raise ValueError("the transform of a plan record holds a NaN or an infinity")
    if ((plan["elastic"] != 0) & (plan["warp"] == 0)).any():
        raise ValueError("a record with elastic set needs warp set")
    if onehot is not None and not (isinstance(onehot, (int, np.integer)) and 1 <= onehot <= MAX_ONEHOT_CLASSES):
        raise ValueError(f"onehot must be None or a class count in 1..{MAX_ONEHOT_CLASSES}, got {onehot!r}")
    return patch


# ------------------------------------------------------------------------------------------------------------------ host twins
def source_coordinates(matrix, offset, output_shape, displacement=None):
    """(3, O0, O1, O2) fp64: the source coordinate of every output index, the sums in the kernel's order, one rounding per
    operation; `displacement` (3, O0, O1, O2) float32 is added last, in fp64.  With a displacement these are the coordinates to
    give ``scipy.ndimage.map_coordinates``."""
    m = np.asarray(matrix, dtype=np.float64).reshape(3, 3)
    off = np.asarray(offset, dtype=np.float64).reshape(3)
    i0, i1, i2 = np.meshgrid(*[np.arange(int(s), dtype=np.float64) for s in output_shape], indexing="ij")
    c = np.stack([(((0.0 + i0 * m[d, 0]) + i1 * m[d, 1]) + i2 * m[d, 2]) + off[d] for d in range(3)])
    if displacement is not None:
        disp = np.asarray(displacement)
        if disp.dtype != np.float32 or disp.shape != c.shape:
            raise ValueError(f"displacement: float32 of shape {c.shape}, got {disp.dtype} {disp.shape}")
        c = c + disp.astype(np.float64)
    return c


def _sample(a, c, order):
    """the order-0 / order-1 rule at the coordinates c (3, ...) of the 3-D array a -> (values of a's dtype, inside)"""
    n = a.shape
    inside = np.ones(c.shape[1:], dtype=bool)
    for d in range(3):
        inside &= (c[d] >= 0) & (c[d] <= n[d] - 1)
    cc = np.where(inside, c, 0.0)
    if order == 0:
        i = np.floor(cc + 0.5).astype(np.int64)
        return np.where(inside, a[i[0], i[1], i[2]], 0).astype(a.dtype), inside
    f = np.floor(cc)
    lo = 1.0 - (cc - f)                                                         # scipy: the last spline weight is one minus the others
    hi = 1.0 - lo
    f = f.astype(np.int64)
    ap = np.pad(a.astype(np.float64), ((0, 1), (0, 1), (0, 1)))                # a corner at index n reads 0
    acc = np.zeros(c.shape[1:], dtype=np.float64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                wx, wy, wz = (hi[0] if dx else lo[0]), (hi[1] if dy else lo[1]), (hi[2] if dz else lo[2])
                acc = acc + ((ap[f[0] + dx, f[1] + dy, f[2] + dz] * wx) * wy) * wz
    return np.where(inside, acc, 0.0).astype(a.dtype), inside


def warp_volume_host(a, matrix, offset, output_shape, order=1, displacement=None):
    """``affine_transform(a, matrix, offset, output_shape=output_shape, order=order, mode='constant', cval=0)`` of a 3-D host array
    (order 1: float32 or float64; order 0: any dtype), or with a displacement ``map_coordinates`` at `source_coordinates`, in numpy,
    operation for operation what the kernel does"""
    a = np.asarray(a)
    if a.ndim != 3 or order not in (0, 1) or (order == 1 and a.dtype not in (np.float32, np.float64)):
        raise ValueError("warp_volume_host takes a 3-D array and order 0, or order 1 with a float32 / float64 array")
    return _sample(a, source_coordinates(matrix, offset, output_shape, displacement), order)[0]


def apply_warp_plan_host(plan, images, labels, displacement=None, onehot=None):
    """What the kernel does with a plan, in numpy: images / labels are the per-case host arrays in the CACHED orientation,
    displacement None or (B, 3, w, h, d) float32 (read by the records with elastic set).
    -> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8, ["onehot_label": (B, onehot, w, h, d) uint8,]
        "in_source": (B, w, h, d) bool -- the voxel's source coordinate lies inside the stored case (outside: 0)}"""
    P0, P1, P2 = patch = _check_warp_plan(plan, len(images), onehot)
    B = len(plan)
    if displacement is not None:
        displacement = np.asarray(displacement)
        if displacement.dtype != np.float32 or displacement.shape != (B, 3, P0, P1, P2):
            raise ValueError(f"displacement: float32 of shape {(B, 3, P0, P1, P2)}")
    elif (plan["elastic"] != 0).any():
        raise ValueError("a record has elastic set: a displacement is needed")
    out_i = np.zeros((B, 1, P0, P1, P2), dtype=np.float32)
    out_l = np.zeros((B, P0, P1, P2), dtype=np.uint8)
    in_src = np.zeros((B, P0, P1, P2), dtype=bool)
    i, j = np.meshgrid(np.arange(P0), np.arange(P1), indexing="ij")
    for n, rec in enumerate(plan):
        img = np.asarray(images[rec["case"]], dtype=np.float32)
        lab = np.asarray(labels[rec["case"]], dtype=np.uint8)
        # the patch in index order (a, b, z) ...
        if rec["warp"]:
            c = source_coordinates(rec["m"], rec["off"], patch, displacement[n] if rec["elastic"] else None)
        else:
            c = np.stack(np.meshgrid(*[rec["origin"][d] + np.arange(patch[d], dtype=np.float64) for d in range(3)], indexing="ij"))
        pi, inside = _sample(img, c, 1 if rec["warp"] else 0)
        pl, _ = _sample(lab, c, 0)
        # ... and the output voxel (i, j) reads index (a, b): undo the flip, then the rot90
        fi = P0 - 1 - i if rec["flip_axis"] == 0 else i
        fj = P1 - 1 - j if rec["flip_axis"] == 1 else j
        a, b = {0: (fi, fj), 1: (fj, P1 - 1 - fi), 2: (P0 - 1 - fi, P1 - 1 - fj), 3: (P0 - 1 - fj, fi)}[int(rec["k"])]
        out_i[n, 0], out_l[n], in_src[n] = pi[a, b], pl[a, b], inside[a, b]
    out = {"image": out_i, "label": out_l, "in_source": in_src}
    if onehot is not None:
        out["onehot_label"] = np.stack([out_l == c for c in range(int(onehot))], axis=1).astype(np.uint8)
    return out


def intensity_host(x, gain=1.0, bias=0.0, gamma=1.0, lo=0.0, hi=1.0):
    """the pointwise value map of one sample in numpy fp64, rounded to float32: ``v = clip(x * gain + bias, lo, hi)``,
    ``u = (v - lo) / (hi - lo)``, ``u ** gamma`` unless gamma == 1, ``u * (hi - lo) + lo``"""
    gain, bias, gamma, lo, hi = (np.float64(v) for v in (gain, bias, gamma, lo, hi))
    v = np.clip(np.asarray(x, dtype=np.float32).astype(np.float64) * gain + bias, lo, hi)
    u = (v - lo) / (hi - lo)
    if gamma != 1.0:
        u = np.power(u, gamma)
    return (u * (hi - lo) + lo).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------- device
def assemble_batch_warp(cache, plan, out=None, displacement=None, label_dtype=torch.uint8, onehot=None, onehot_dtype=torch.int64):
    """`assemble_batch` for a plan of `draw_plan_warp`: -> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8 | int64
    [, "onehot_label": (B, onehot, w, h, d) onehot_dtype]} on the cache's device, enqueued on the current stream: one launch of
    dycon_assemble_batch_warp per 16 samples writes all of them, no allocation when `out` is given, no host synchronisation.
    displacement: None or a contiguous (B, 3, w, h, d) float32 tensor on the device (`elastic_field`), read by the records with
    elastic set.  Only the geometry of a record is applied here (blur, gain, bias and gamma are `DeviceBatchLoader`'s next steps).
    There is no host fallback: a cache that is not on a GPU raises."""
    P0, P1, P2 = _check_warp_plan(plan, len(cache), onehot)
    if label_dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"label_dtype must be torch.uint8 or torch.int64, got {label_dtype}")
    if onehot is not None and onehot_dtype not in ONEHOT_DTYPES:
        raise ValueError(f"onehot_dtype must be one of {ONEHOT_DTYPES}, got {onehot_dtype}")
    if cache.device.type != "cuda":
        raise _lib.DyconLibraryError("assemble_batch_warp runs on the GPU only (the cache is on %s)" % cache.device)
    B, C, dev = len(plan), int(onehot or 0), cache.images.device
    if displacement is not None:
        if not (torch.is_tensor(displacement) and tuple(displacement.shape) == (B, 3, P0, P1, P2) and displacement.device == dev
                and displacement.dtype == torch.float32 and displacement.is_contiguous()):
            raise ValueError("displacement: a contiguous (B, 3, w, h, d) float32 tensor on the cache's device")
    elif (plan["elastic"] != 0).any():
        raise ValueError("a record has elastic set: a displacement is needed")
    if out is None:
        out = {"image": torch.empty((B, 1, P0, P1, P2), dtype=torch.float32, device=dev),
               "label": torch.empty((B, P0, P1, P2), dtype=label_dtype, device=dev)}
        if C:
            out["onehot_label"] = torch.empty((B, C, P0, P1, P2), dtype=onehot_dtype, device=dev)
    image, label, hot = out["image"], out["label"], out.get("onehot_label") if C else None
    if not (tuple(image.shape) == (B, 1, P0, P1, P2) and image.dtype == torch.float32 and tuple(label.shape) == (B, P0, P1, P2)
            and label.dtype == label_dtype and image.is_contiguous() and label.is_contiguous()
            and image.device == dev and label.device == dev):
        raise ValueError("out: contiguous (B, 1, w, h, d) float32 and (B, w, h, d) label_dtype tensors on the cache's device")
    if C and not (hot is not None and tuple(hot.shape) == (B, C, P0, P1, P2) and hot.dtype == onehot_dtype and hot.is_contiguous()
                  and hot.device == dev):
        raise ValueError("out: a contiguous (B, onehot, w, h, d) onehot_dtype tensor 'onehot_label' on the cache's device")
    case = plan["case"]
    jobs = np.zeros(B, dtype=_WARP_JOB_DTYPE)
    jobs["image_off"], jobs["label_off"] = cache._img_off[case], cache._lab_off[case]
    jobs["X"], jobs["Y"], jobs["Z"] = cache._shape_arr[case].T
    jobs["ox"], jobs["oy"], jobs["oz"] = plan["origin"].T
    jobs["k"], jobs["flip_axis"] = plan["k"], plan["flip_axis"]
    jobs["m"], jobs["off"], jobs["warp"], jobs["elastic"] = plan["m"], plan["off"], plan["warp"], plan["elastic"]
    vox, lb, hb = P0 * P1 * P2, label.element_size(), hot.element_size() if C else 0
    stream = ops._s()
    for n0 in range(0, B, JOBS_PER_LAUNCH):
        n = min(JOBS_PER_LAUNCH, B - n0)
        _lib.call("dycon_assemble_batch_warp", cache.images.data_ptr(), cache.labels.data_ptr(),
                  jobs.ctypes.data + n0 * _WARP_JOB_DTYPE.itemsize, n,
                  displacement.data_ptr() + 4 * 3 * vox * n0 if displacement is not None else None, P0, P1, P2,
                  image.data_ptr() + 4 * vox * n0, label.data_ptr() + lb * vox * n0, lb,
                  hot.data_ptr() + hb * C * vox * n0 if C else None, C, hb, stream)
    return out


def elastic_noise(B, patch, seed, offset, out=None, zeros=None, device="cuda"):
    """(B, 3, w, h, d) standard normal deviates on `device`: the library's Philox noise launch (`ops.add_noise`, unit sigma, no
    clipping) on a zero buffer, from (seed, offset)"""
    shape = (int(B), 3) + tuple(int(v) for v in patch)
    if zeros is None:
        zeros = torch.zeros(shape, dtype=torch.float32, device=device)
    if out is None:
        out = torch.empty_like(zeros)
    _lib.call("dycon_add_noise", zeros.data_ptr(), None, out.data_ptr(), _lib.F32, zeros.numel(), 1.0, float("inf"), int(seed),
              int(offset), ops._s())
    return out


def elastic_field(B, patch, alpha, sigma, seed=0, offset=0, out=None, samples=None, device="cuda", _buffers=None):
    """The displacement field of an elastic deformation, (B, 3, w, h, d) float32 in voxels on `device` (a GPU): standard
    normal deviates (`elastic_noise`), smoothed per sample by ``gaussian_filter(sigma, mode="constant")`` and multiplied by
    float32(alpha) -- ``alpha[n] * gaussian_filter(noise[n], sigma[n], mode="constant")`` bit for bit.  alpha, sigma: a number or
    one per sample.  samples: the sample numbers to fill (default all; the rest of `out` is left as it is).  The deviates are the
    library's counter-based Philox stream, not ``np.random``'s: the field is reproducible from (seed, offset) and equal to a
    host-drawn one in distribution only."""
    patch = tuple(int(v) for v in patch)
    alpha, sigma = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (B,)), np.broadcast_to(np.asarray(sigma, dtype=np.float64), (B,))
    if len(patch) != 3 or min(patch) <= 0 or B <= 0 or not (np.isfinite(alpha).all() and (sigma > 0).all()):
        raise ValueError("elastic_field: B > 0, a positive 3-D patch, finite alpha and positive sigma")
    zeros, noise, ws = _buffers if _buffers is not None else (None, None, None)
    noise = elastic_noise(B, patch, seed, offset, out=noise, zeros=zeros, device=device)
    if out is None:
        out = torch.zeros_like(noise)
    elif not (tuple(out.shape) == tuple(noise.shape) and out.dtype == torch.float32 and out.is_cuda and out.is_contiguous()):
        raise ValueError("out: a contiguous (B, 3, w, h, d) float32 CUDA tensor")
    for n in (range(B) if samples is None else samples):
        gaussian_filter(noise[n], float(sigma[n]), mode="constant", out=out[n], scale=float(np.float32(alpha[n])), workspace=ws)
    return out


_ORDER0_DTYPES = (torch.uint8, torch.bool, torch.float32, torch.float64, torch.int64)      # rotate_nearest's


def warp_volume(t, matrix, offset, output_shape=None, order=1, displacement=None):
    """``scipy.ndimage.affine_transform(t, matrix, offset, output_shape=output_shape, order=order, mode='constant', cval=0)`` of a
    3-D CUDA tensor on the current stream, bit for bit; with `displacement` ((3,) + output_shape, float32, added to the coordinates
    in fp64) ``map_coordinates(t, source_coordinates(...), order=order, mode='constant')``.  order 1: float32 or float64; order 0:
    uint8, bool, float32, float64 or int64 (values are moved).  matrix: 3 x 3; offset: 3.  -> a new tensor of output_shape."""
    if order not in (0, 1):
        raise ValueError(f"order must be 0 or 1, got {order}")
    ok = (torch.float32, torch.float64) if order == 1 else _ORDER0_DTYPES
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in ok and t.numel() > 0):
        raise ValueError(f"warp_volume(order={order}) takes a non-empty 3-D CUDA tensor of dtype {ok}")
    shape = tuple(int(v) for v in (t.shape if output_shape is None else output_shape))
    if len(shape) != 3 or min(shape) <= 0:
        raise ValueError(f"output_shape must be three positive sizes, got {output_shape}")
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).reshape(-1))
    off = np.ascontiguousarray(np.asarray(offset, dtype=np.float64).reshape(-1))
    if m.shape != (9,) or off.shape != (3,) or not (np.isfinite(m).all() and np.isfinite(off).all()):
        raise ValueError("matrix must be a finite 3 x 3 and offset a finite 3-vector")
    if displacement is not None and not (torch.is_tensor(displacement) and tuple(displacement.shape) == (3,) + shape
                                         and displacement.dtype == torch.float32 and displacement.device == t.device
                                         and displacement.is_contiguous()):
        raise ValueError("displacement: a contiguous (3,) + output_shape float32 tensor on t's device")
    t = t.contiguous()
    out = torch.empty(shape, dtype=t.dtype, device=t.device)
    _lib.call("dycon_warp_volume", t.data_ptr(), *t.shape, out.data_ptr(), *shape, order, t.element_size(), m.ctypes.data,
              off.ctypes.data, displacement.data_ptr() if displacement is not None else None, ops._s())
    return out


def intensity_augment(x, gain=1.0, bias=0.0, gamma=1.0, lo=0.0, hi=1.0, samples=None, out=None):
    """`intensity_host` of the samples of a CUDA float32 tensor (B, ...) on the current stream: bit for bit when gamma == 1, within
    one fp32 ulp otherwise.  gain, bias, gamma, lo, hi: a number or one per processed sample.  samples: the sample numbers to
    process (default all); the others are not touched.  out: default a new tensor (a copy of x when `samples` is given); x itself
    works in place.  -> out"""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() >= 2 and x.numel() > 0 and x.is_contiguous()):
        raise ValueError("intensity_augment takes a non-empty contiguous CUDA float32 tensor (B, ...)")
    B = int(x.shape[0])
    sel = np.arange(B, dtype=np.int64) if samples is None else np.ascontiguousarray(samples, dtype=np.int64).reshape(-1)
    if len(sel) == 0 or sel.min() < 0 or sel.max() >= B:
        raise ValueError(f"samples must name samples in 0..{B - 1}")
    par = np.ascontiguousarray(np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), sel.shape)
                                         for v in (gain, bias, gamma, lo, hi)], axis=1))
    if not (np.isfinite(par).all() and (par[:, 2] > 0).all() and (par[:, 3] < par[:, 4]).all()):
        raise ValueError("gain, bias, gamma, lo, hi must be finite with gamma > 0 and lo < hi")
    if out is None:
        out = torch.empty_like(x) if samples is None else x.clone()
    elif not (out.shape == x.shape and out.dtype == torch.float32 and out.device == x.device and out.is_contiguous()):
        raise ValueError("out: a contiguous float32 tensor of x's shape on its device")
    _lib.call("dycon_intensity_augment", x.data_ptr(), out.data_ptr(), x.numel() // B, sel.ctypes.data, par.ctypes.data, len(sel), ops._s())
    return out


class LoaderAugment:
    """The state `DeviceBatchLoader` keeps for `warp` / `intensity`: the buffers of the elastic field and the filter workspace,
    allocated with the first batch and kept, so that later batches allocate nothing and nothing synchronises with the host."""

    def __init__(self, seed, device):
        self.seed, self.device, self._field, self._ws = int(seed), device, None, None

    def field(self, plan, n):
        """the displacement of batch number n for the records of `plan` with elastic set (None when there is none)"""
        sel = np.flatnonzero(plan["elastic"])
        if len(sel) == 0:
            return None
        B, patch = len(plan), tuple(int(v) for v in plan["patch"][0])
        if self._field is None or self._field[0].shape[0] != B:
            zeros = torch.zeros((B, 3) + patch, dtype=torch.float32, device=self.device)
            self._field = (zeros, torch.empty_like(zeros), torch.zeros_like(zeros))
        zeros, noise, out = self._field
        return elastic_field(B, patch, np.where(plan["elastic"] != 0, plan["alpha"], 0.0), np.where(plan["elastic"] != 0, plan["sigma"], 1.0),
                             self.seed, n << 32, out=out, samples=sel, _buffers=(zeros, noise, self._workspace(3, patch)))

    def _workspace(self, N, patch):
        need = max(workspace_bytes(N, patch, 3, False), workspace_bytes(1, patch, 3, True), 1)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._ws

    def values(self, plan, image, lo, hi):
        """blur, then gain / bias / gamma, in place on the samples of `image` (B, 1, w, h, d) whose record asks for them"""
        patch = tuple(int(v) for v in plan["patch"][0])
        for n in np.flatnonzero(plan["blur_sigma"] > 0):
            gaussian_filter(image[n, 0], float(plan["blur_sigma"][n]), out=image[n, 0], workspace=self._workspace(3, patch))
        sel = np.flatnonzero((plan["gain"] != 1) | (plan["bias"] != 0) | (plan["gamma"] != 1))
        if len(sel):
            intensity_augment(image, plan["gain"][sel], plan["bias"][sel], plan["gamma"][sel], lo, hi, samples=sel, out=image)
