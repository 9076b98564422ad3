"""The reference's remaining loader augmentations on the device-resident data path: RandomRot, CreateOnehotLabel, RandomNoise.

    rotation_of(angle, shape)                                 host: the fp64 matrix and offset scipy.ndimage.rotate uses
    draw_plan_rot(shapes, indices, patch_size, ...)           host: draw_plan with RandomRot() in front of either chain
    apply_rot_plan_host(plan, images, labels, onehot)         host: numpy restatement of the kernel (the CPU-testable twin)
    assemble_batch_rot(cache, plan, out, label_dtype, onehot, onehot_dtype)   device: dycon_assemble_batch_rot, one launch per 16
    rotate_nearest(t, angle)                                  device: ndimage.rotate(order=0, reshape=False) of one CUDA volume
    DeviceBatchLoader(..., rot, onehot, onehot_dtype, noise_sigma, noise_seed)   (device_cache.py) routes here

`RandomRot` (code/dataloaders/isles22.py:24-28, :198-209; la_heart.py, brats19.py and pancreas.py define it again) is
``scipy.ndimage.rotate(x, np.random.randint(-20, 20), order=0, reshape=False)``: a nearest-neighbour rotation about the last axis that
keeps the shape.  It is the only augmentation of the reference that is not a permutation of voxels, but it is a gather: scipy maps
an output index (rx, ry) to the source coordinate ``M @ (rx, ry) + off`` in fp64, drops it when it lies outside ``[0, n - 1]`` on
either axis (mode='constant': the test comes BEFORE the rounding) and reads the voxel at ``floor(c + 0.5)``.  So the rotated volume
never has to exist.  The crop origin, the rot90 count and the flip of a plan record address the rotated volume (of the stored shape)
exactly as they address the stored one without RandomRot, and the kernel (csrc/augment.hip) follows each output voxel through both
maps to one source voxel of the cached case.

What is equal to what.  For a seeded ``np.random`` and ``rot=True`` the loader yields, bit for bit, what
``DataLoader(dataset, batch_sampler=..., num_workers=0)`` yields with ``Compose([RandomRot(), RandomCrop(p), RandomRotFlip(),
[CreateOnehotLabel(C),] ToTensor()])`` of dataloaders/isles22.py (order="rotflip_crop": ``RandomRot(), RandomRotFlip(),
RandomCrop(p)``), i.e. what scipy computes on the host; the one-hot planes equal CreateOnehotLabel's (a label >= C sets no plane).
The source coordinates are restated operation by operation (`_source`), which holds for the scipy this was checked against
(1.15); tests/test_augment_cpu.py compares with the installed scipy directly.  The noise is NOT ``np.random.randn``'s stream: see
DeviceBatchLoader.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops
from .device_cache import JOBS_PER_LAUNCH, PLAN_DTYPE, _draw_record, _plan_args

#: PLAN_DTYPE's fields, then the drawn angle (degrees) and the rotation scipy derives from it (`rotation_of`): m row-major
ROT_PLAN_DTYPE = np.dtype(PLAN_DTYPE.descr + [("angle", "<i4"), ("m", "<f8", (4,)), ("off", "<f8", (2,))])

# dycon_rot_job_t (include/dycon_hip.h), field for field
_ROT_JOB_DTYPE = np.dtype([("image_off", "<i8"), ("label_off", "<i8"), ("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"),
                           ("ox", "<i4"), ("oy", "<i4"), ("oz", "<i4"), ("k", "<i4"), ("flip_axis", "<i4"),
                           ("m", "<f8", (4,)), ("off", "<f8", (2,)), ("rotate", "<i4"), ("reserved", "<i4")], align=True)
ONEHOT_DTYPES = (torch.uint8, torch.float32, torch.int64)
MAX_ONEHOT_CLASSES = 8


def rotation_of(angle, shape):
    """(m, off) of ``scipy.ndimage.rotate(x, angle, reshape=False)`` for x of shape (X, Y, ...): the 2 x 2 fp64 matrix
    [[c, s], [-s, c]] with c, s = cosdg, sindg(angle) and the offset ctr - m @ ctr, ctr = ([X, Y] - 1) / 2, formed by the
    expressions scipy itself uses."""
    from scipy import special   # lazy, as RandomRot imports scipy
    c, s = special.cosdg(angle), special.sindg(angle)
    m = np.array([[c, s], [-s, c]])
    plane = np.asarray([int(shape[0]), int(shape[1])])
    off = (plane - 1) / 2 - m @ ((plane - 1) / 2)
    return m, off


def draw_plan_rot(shapes, indices, patch_size, angle_range=(-20, 20), rot_flip=True, order="crop_rotflip"):
    """The plan of one batch with ``RandomRot()`` in front of the chain: a ROT_PLAN_DTYPE record per entry of `indices`.

    Pure host code.  Consumes ``np.random`` as RandomRot followed by either chain does for each index in order: the angle
    (``np.random.randint(*angle_range)``) first, then what `draw_plan` draws for that order (its drawing code is shared).  The
    rotation keeps the shape, so pad, crop bounds, k and axis come from the stored shape as without it; an odd k still needs a
    square patch."""
    patch = _plan_args(patch_size, rot_flip, False, order)
    lo, hi = (int(v) for v in angle_range)
    if not lo < hi:
        raise ValueError(f"angle_range must be (low, high) with low < high, got {angle_range}")
    plan = np.zeros(len(indices), dtype=ROT_PLAN_DTYPE)
    for n, idx in enumerate(indices):
        angle = int(np.random.randint(lo, hi))
        origin, k, axis = _draw_record(shapes[idx], patch, rot_flip, False, order)
        m, off = rotation_of(angle, shapes[idx])
        plan[n] = (idx, origin, k, axis, patch, angle, m.reshape(4), off)
    return plan


def _check_rot_plan(plan, ncases, onehot=None):
    """-> (patch, rotate) of a well-formed plan: ROT_PLAN_DTYPE records (rotate) or PLAN_DTYPE records (no rotation)"""
    plan = np.asarray(plan)
    if plan.dtype not in (ROT_PLAN_DTYPE, PLAN_DTYPE) or plan.ndim != 1 or len(plan) == 0:
        raise ValueError("a plan is a non-empty 1-D array of ROT_PLAN_DTYPE (draw_plan_rot) or PLAN_DTYPE (draw_plan) records")
    patch = tuple(int(v) for v in plan["patch"][0])
    if (plan["patch"] != plan["patch"][0]).any() or min(patch) <= 0:
        raise ValueError("all samples of a batch share one positive patch size")
    if plan["case"].min() < 0 or plan["case"].max() >= ncases:
        raise ValueError(f"plan names case {plan['case'].max()} of {ncases}")
    if plan["k"].min() < 0 or plan["k"].max() > 3 or plan["flip_axis"].min() < -1 or plan["flip_axis"].max() > 1:
        raise ValueError("k must be in 0..3 and flip_axis in {-1, 0, 1}")
    if patch[0] != patch[1] and (plan["k"] & 1).any():
        raise ValueError(f"an odd k needs a square patch in the first two axes, got {patch[0]} x {patch[1]}")
    rotate = plan.dtype == ROT_PLAN_DTYPE
    if rotate and not (np.isfinite(plan["m"]).all() and np.isfinite(plan["off"]).all()):
        raise ValueError("the rotation of a plan record holds a NaN or an infinity")
    if onehot is not None and not (isinstance(onehot, (int, np.integer)) and 1 <= onehot <= MAX_ONEHOT_CLASSES):
        raise ValueError(f"onehot must be None or a class count in 1..{MAX_ONEHOT_CLASSES}, got {onehot!r}")
    return patch, rotate


def _source(rx, ry, X, Y, m, off):
    """scipy's source of the indices (rx, ry) of a rotated (X, Y) plane -> (inside, sx, sy): the coordinate sums in scipy's order,
    one rounding per operation; sx, sy are meaningful where `inside`."""
    x, y = rx.astype(np.float64), ry.astype(np.float64)
    cx = ((0.0 + x * m[0]) + y * m[1]) + off[0]
    cy = ((0.0 + x * m[2]) + y * m[3]) + off[1]
    inside = (cx >= 0) & (cx <= X - 1) & (cy >= 0) & (cy <= Y - 1)
    sx = np.where(inside, np.floor(cx + 0.5), 0).astype(np.int64)
    sy = np.where(inside, np.floor(cy + 0.5), 0).astype(np.int64)
    return inside, sx, sy


def rotate_nearest_host(a, m, off):
    """``ndimage.rotate(a, angle, order=0, reshape=False)`` of a 3-D host array from (m, off) = rotation_of(angle, a.shape)"""
    a = np.asarray(a)
    X, Y = a.shape[:2]
    rx, ry = np.meshgrid(np.arange(X), np.arange(Y), indexing="ij")
    inside, sx, sy = _source(rx, ry, X, Y, np.asarray(m, dtype=np.float64).reshape(4), off)
    return np.where(inside[:, :, None], a[sx, sy], 0).astype(a.dtype)


def apply_rot_plan_host(plan, images, labels, onehot=None):
    """What the kernel does with a plan, in numpy: images / labels are the per-case host arrays in the CACHED orientation.
    -> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8, ["onehot_label": (B, onehot, w, h, d) uint8,]
        "in_volume": (B, w, h, d) bool -- the voxel's index lies inside the rotated volume (outside: the reference's zero pad),
        "in_source": (B, w, h, d) bool -- ... and its source coordinate inside the stored one (in_volume & ~in_source: a zero the
                                           rotation made)}"""
    (P0, P1, P2), rotate = _check_rot_plan(plan, len(images), onehot)
    B = len(plan)
    out_i = np.zeros((B, 1, P0, P1, P2), dtype=np.float32)
    out_l = np.zeros((B, P0, P1, P2), dtype=np.uint8)
    in_vol, in_src = np.zeros((B, P0, P1, P2), dtype=bool), np.zeros((B, P0, P1, P2), dtype=bool)
    i, j = np.meshgrid(np.arange(P0), np.arange(P1), indexing="ij")
    z = np.arange(P2)
    for n, rec in enumerate(plan):
        img, lab = np.asarray(images[rec["case"]]), np.asarray(labels[rec["case"]])
        X, Y, Z = img.shape
        fi = P0 - 1 - i if rec["flip_axis"] == 0 else i          # undo the flip ...
        fj = P1 - 1 - j if rec["flip_axis"] == 1 else j
        a, b = {0: (fi, fj), 1: (fj, P1 - 1 - fi), 2: (P0 - 1 - fi, P1 - 1 - fj), 3: (P0 - 1 - fj, fi)}[int(rec["k"])]   # ... and the rot90
        rx, ry, rz = rec["origin"][0] + a, rec["origin"][1] + b, rec["origin"][2] + z
        okz = (rz >= 0) & (rz < Z)
        vol = (rx >= 0) & (rx < X) & (ry >= 0) & (ry < Y)
        if rotate:
            src, sx, sy = _source(rx, ry, X, Y, rec["m"], rec["off"])
            src &= vol
        else:
            src, sx, sy = vol, rx, ry
        in_vol[n] = vol[:, :, None] & okz[None, None, :]
        in_src[n] = ok = src[:, :, None] & okz[None, None, :]
        cx, cy, cz = np.clip(sx, 0, X - 1)[:, :, None], np.clip(sy, 0, Y - 1)[:, :, None], np.clip(rz, 0, Z - 1)[None, None, :]
        out_i[n, 0] = np.where(ok, img[cx, cy, cz], 0).astype(np.float32)
        out_l[n] = np.where(ok, lab[cx, cy, cz], 0).astype(np.uint8)
    out = {"image": out_i, "label": out_l, "in_volume": in_vol, "in_source": in_src}
    if onehot is not None:
        out["onehot_label"] = np.stack([out_l == c for c in range(int(onehot))], axis=1).astype(np.uint8)
    return out


def assemble_batch_rot(cache, plan, out=None, label_dtype=torch.uint8, onehot=None, onehot_dtype=torch.int64):
    """`assemble_batch` for a plan of `draw_plan_rot`: -> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8 | int64
    [, "onehot_label": (B, onehot, w, h, d) onehot_dtype]} on the cache's device, enqueued on the current stream: one launch of
    dycon_assemble_batch_rot per 16 samples writes all of them, no allocation when `out` (a dict of such tensors) is given, no
    host synchronisation.  onehot: None or the class count C in 1..8 (plane c holds label == c, as CreateOnehotLabel; ToTensor
    makes it int64, uint8 and float32 are offered for consumers that want less traffic).  A PLAN_DTYPE plan (draw_plan) is taken
    as well and not rotated: the bits are assemble_batch's.  There is no host fallback: a cache that is not on a GPU raises."""
    (P0, P1, P2), rotate = _check_rot_plan(plan, len(cache), onehot)
    if label_dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"label_dtype must be torch.uint8 or torch.int64, got {label_dtype}")
    if onehot is not None and onehot_dtype not in ONEHOT_DTYPES:
        raise ValueError(f"onehot_dtype must be one of {ONEHOT_DTYPES}, got {onehot_dtype}")
    if cache.device.type != "cuda":
        raise _lib.DyconLibraryError("assemble_batch_rot runs on the GPU only (the cache is on %s)" % cache.device)
    B, C, dev = len(plan), int(onehot or 0), cache.images.device
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
    jobs = np.zeros(B, dtype=_ROT_JOB_DTYPE)
    jobs["image_off"], jobs["label_off"] = cache._img_off[case], cache._lab_off[case]
    jobs["X"], jobs["Y"], jobs["Z"] = cache._shape_arr[case].T
    jobs["ox"], jobs["oy"], jobs["oz"] = plan["origin"].T
    jobs["k"], jobs["flip_axis"] = plan["k"], plan["flip_axis"]
    if rotate:
        jobs["m"], jobs["off"], jobs["rotate"] = plan["m"], plan["off"], 1
    vox, lb, hb = P0 * P1 * P2, label.element_size(), hot.element_size() if C else 0
    stream = ops._s()
    for n0 in range(0, B, JOBS_PER_LAUNCH):
        n = min(JOBS_PER_LAUNCH, B - n0)
        _lib.call("dycon_assemble_batch_rot", cache.images.data_ptr(), cache.labels.data_ptr(),
                  jobs.ctypes.data + n0 * _ROT_JOB_DTYPE.itemsize, n, P0, P1, P2, image.data_ptr() + 4 * vox * n0,
                  label.data_ptr() + lb * vox * n0, lb, hot.data_ptr() + hb * C * vox * n0 if C else None, C, hb, stream)
    return out


_ROTATE_DTYPES = (torch.uint8, torch.bool, torch.float32, torch.float64, torch.int64)


def rotate_nearest(t, angle):
    """``scipy.ndimage.rotate(t, angle, order=0, reshape=False)`` of a 3-D CUDA tensor (uint8, bool, float32, float64 or int64) on
    the current stream, bit for bit: order 0 moves values and computes none, so the kernel moves bytes.  -> a new tensor."""
    if not (torch.is_tensor(t) and t.is_cuda and t.dim() == 3 and t.dtype in _ROTATE_DTYPES and t.numel() > 0):
        raise ValueError("rotate_nearest takes a non-empty 3-D CUDA tensor of dtype uint8, bool, float32, float64 or int64")
    t = t.contiguous()
    out = torch.empty_like(t)
    m, off = rotation_of(angle, t.shape)
    m, off = np.ascontiguousarray(m, dtype=np.float64), np.ascontiguousarray(off, dtype=np.float64)
    X, Y, Z = t.shape
    _lib.call("dycon_rotate_nearest", t.data_ptr(), out.data_ptr(), t.element_size(), X, Y, Z, m.ctypes.data, off.ctypes.data, ops._s())
    return out
