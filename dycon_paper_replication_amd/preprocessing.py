"""Preprocessing on the device: the reference's normalize_image and its scipy.ndimage.zoom calls (code/BraTS19_DataPreprocessing.py,
code/ISLES22_DataPreprocessing.py) as HIP kernels (csrc/resample.hip).

    volume_stats(x)                             VolumeStats: count, fp64 mean / std of the voxels > 0, extremes, per sample
    normalize_image(x)                          the reference function: z-score over the voxels > 0, then min-max to [0, 1]
    zoom(x, target_shape, order, norm=None)     scipy.ndimage.zoom(x, [t / s per axis], order) for order 0 and 1
    preprocess_brats_volume(image, seg)         (image fp32, label uint8) at 192 x 192 x 64   (BraTS19_DataPreprocessing.py:175-198)
    preprocess_isles_volume(image, mask)        the same at 112 x 112 x 64 with mask > 0.5    (ISLES22_DataPreprocessing.py:141-159)

CUDA tensors or host arrays come in (host arrays are cast as the reference casts them and uploaded); CUDA tensors go out, on the
input's device and the current stream, and nothing is read back.  Volumes are (X, Y, Z) or (B, X, Y, Z); every sample of a batch has
its own statistics.  A 2-D array goes through a trailing unit axis (the form RandomGenerator of dataloaders/la_heart.py uses, order
0).  There is no host fallback: without the library, or without a GPU, these raise.

What is equal to what (tests/test_preprocess_gpu.py): order 0 is scipy's result bit for bit; order 1 is the numpy restatement
(tests/resample_ref.py) bit for bit and scipy's up to its summation order; normalize_image differs from the reference's by the
rounding of its float32 pairwise mean and standard deviation (here: fp64 sums rounded once), which is about 1e-7 on [0, 1].
A preprocess_*_volume call is two launches of the library per image (statistics, zoom with the normalisation applied on load: the
full-resolution normalised volume is never written) and one per label (order-0 zoom that binarises on load).
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops

__all__ = ["VolumeStats", "volume_stats", "normalize_image", "zoom", "preprocess_brats_volume", "preprocess_isles_volume"]

STATS_BYTES, RECORD_BYTES = 48, 24            # dycon_volume_stats_t, dycon_norm_record_t


class VolumeStats:
    """Per-sample statistics of a batch, on the device: `raw` is (B, 48) uint8 holding dycon_volume_stats_t, `record` (B, 24) uint8
    holding dycon_norm_record_t (apply_z, mean32, std32, apply_mm, lo32, hi32), what `zoom(norm=...)` takes.  The named fields are
    views: n_pos int64, mean / std float64, min_pos / max_pos / min_all / max_all float32, any_nonpos int32, each of shape (B,)."""

    def __init__(self, raw, record):
        self.raw, self.record = raw, record

    n_pos = property(lambda self: self.raw.view(torch.int64)[:, 0])
    mean = property(lambda self: self.raw.view(torch.float64)[:, 1])
    std = property(lambda self: self.raw.view(torch.float64)[:, 2])
    min_pos = property(lambda self: self.raw.view(torch.float32)[:, 6])
    max_pos = property(lambda self: self.raw.view(torch.float32)[:, 7])
    min_all = property(lambda self: self.raw.view(torch.float32)[:, 8])
    max_all = property(lambda self: self.raw.view(torch.float32)[:, 9])
    any_nonpos = property(lambda self: self.raw.view(torch.int32)[:, 10])


def _device_volume(x, dtypes, what):
    """-> (contiguous CUDA tensor (B, X, Y, Z), the shape to give the result's leading axes back).  float arrays are cast to float32
    (the reference's astype(np.float32)), bool to uint8; anything not in `dtypes` after that raises"""
    if not torch.is_tensor(x):
        a = np.asarray(x)
        if a.dtype.kind == "f" and a.dtype != np.float32:
            a = a.astype(np.float32)
        elif a.dtype == np.bool_:
            a = a.astype(np.uint8)
        if not torch.cuda.is_available():
            raise _lib.DyconLibraryError(f"{what} runs on the GPU only")
        x = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    elif not x.is_cuda:
        raise ValueError(f"{what} takes CUDA tensors or host arrays, got a tensor on {x.device}")
    if x.is_floating_point() and x.dtype != torch.float32:
        x = x.float()
    elif x.dtype == torch.bool:
        x = x.to(torch.uint8)
    if x.dtype not in dtypes:
        raise ValueError(f"{what}: dtype {x.dtype} (takes {', '.join(str(d) for d in dtypes)})")
    if x.dim() not in (2, 3, 4) or min(x.shape) < 1:
        raise ValueError(f"{what}: a volume is (X, Y, Z), (B, X, Y, Z) or a 2-D (X, Y) array without empty axes, got {tuple(x.shape)}")
    lead = tuple(x.shape[:-3]) if x.dim() == 4 else ()
    v = x.reshape((1,) + tuple(x.shape) + (1,)) if x.dim() == 2 else x.reshape((-1,) + tuple(x.shape[-3:]))
    return v.contiguous(), lead


def _stats(vol, want_stats=True):
    B, dev = vol.shape[0], vol.device
    raw = torch.empty((B, STATS_BYTES), dtype=torch.uint8, device=dev) if want_stats else None
    record = torch.empty((B, RECORD_BYTES), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ops.volume_stats(vol, raw, record)
    return VolumeStats(raw, record)


def volume_stats(x):
    """VolumeStats of x, fp32 (X, Y, Z) or (B, X, Y, Z): what normalize_image reads from a volume, in fp64 and in a fixed order (the
    same bits on every run)."""
    vol, _ = _device_volume(x, (torch.float32,), "volume_stats")
    return _stats(vol)


def _record(norm, B, dev):
    rec = norm.record if isinstance(norm, VolumeStats) else norm
    if not (torch.is_tensor(rec) and rec.is_cuda and rec.device == dev and rec.dtype == torch.uint8 and rec.is_contiguous()
            and tuple(rec.shape) == (B, RECORD_BYTES)):
        raise ValueError(f"norm: a VolumeStats of the same batch (or its record, ({B}, {RECORD_BYTES}) uint8 on {dev})")
    return rec


def normalize_image(x):
    """normalize_image of BraTS19_DataPreprocessing.py:8-31 (= ISLES22_DataPreprocessing.py:10-33) for fp32 (X, Y, Z) or (B, X, Y, Z):
    z-score over the voxels > 0 (0 elsewhere), then min-max to [0, 1].  The reference's edge rules: an all-zero volume comes back
    unchanged; without a voxel > 0, or with std == 0, the z-score is skipped and the raw values are min-maxed; max == min skips the
    min-max.  NaN / infinite input: unspecified."""
    vol, lead = _device_volume(x, (torch.float32,), "normalize_image")
    rec = _stats(vol, want_stats=False).record
    with torch.cuda.device(vol.device):
        out = ops.normalize_apply(vol, rec)
    return out.reshape(lead + tuple(vol.shape[1:])) if np.ndim(x) != 2 else out.reshape(tuple(vol.shape[1:3]))


def _target(shape, target_shape, ndim):
    t = tuple(int(n) for n in target_shape)
    if ndim == 2:
        if len(t) != 2:
            raise ValueError(f"target_shape of a 2-D array has two sizes, got {target_shape}")
        t += (1,)
    if len(t) != 3 or min(t) < 1:
        raise ValueError(f"target_shape: three positive sizes, got {target_shape}")
    for s, n in zip(shape, t):                       # scipy's output shape for the factors t / s: the target itself
        if int(round(s * (n / s))) != n:
            raise ValueError(f"zoom factors {n} / {s} do not give the target size back (round({s} * ({n} / {s})) != {n})")
    return t


def _zoom(vol, target, order, rec, out_dtype, binarize):
    with torch.cuda.device(vol.device):
        return ops.zoom(vol, target, order, record=rec, binarize=binarize, out_dtype=out_dtype)


def zoom(x, target_shape, order, norm=None, out_dtype=None, binarize=None):
    """scipy.ndimage.zoom(x, [t / s for t, s in zip(target_shape, x.shape)], order=order) (mode="constant", cval=0,
    grid_mode=False) per sample of x: (X, Y, Z), (B, X, Y, Z) or 2-D (X, Y).

    order=0    nearest: fp32 -> fp32, uint8 / bool -> uint8; scipy's result bit for bit
    order=1    linear: fp32 -> fp32 (scipy's dtype), or out_dtype=torch.float64 to keep the fp64 accumulator
    norm       a VolumeStats (or its `record`) of the same batch: normalize_image is applied to every source value on load
    binarize   order 0 only, a threshold: the result is uint8 and holds `value > binarize` as 0 / 1 (taken on load)

    ValueError before anything is launched: an order other than 0 and 1, a target a factor t / s does not reproduce, a dtype or a
    combination the kernels do not take."""
    if order not in (0, 1):
        raise ValueError(f"order must be 0 or 1, got {order} (higher spline orders are not built)")
    vol, lead = _device_volume(x, (torch.float32,) if order == 1 else (torch.float32, torch.uint8), "zoom")
    two_d = np.ndim(x) == 2
    target = _target(vol.shape[1:], target_shape, 2 if two_d else 3)
    if binarize is not None and (order != 0 or norm is not None):
        raise ValueError("binarize takes order 0 and no norm")
    if norm is not None and vol.dtype != torch.float32:
        raise ValueError("norm needs a float32 volume")
    want = torch.uint8 if binarize is not None else vol.dtype
    if out_dtype is not None and out_dtype != want and not (order == 1 and out_dtype == torch.float64):
        raise ValueError(f"out_dtype {out_dtype}: order 0 keeps the dtype, order 1 writes float32 or float64")
    rec = None if norm is None else _record(norm, vol.shape[0], vol.device)
    out = _zoom(vol, target, order, rec, out_dtype or want, binarize)
    return out.reshape(target[:2]) if two_d else out.reshape(lead + target)


def _preprocess(image, label, target_shape, thr, what):
    img, lead = _device_volume(image, (torch.float32,), what)
    if torch.is_tensor(label) and label.dtype not in (torch.uint8, torch.bool) and not label.is_floating_point():
        label = label.float()                          # other integer labels: the comparison is taken in fp32
    elif not torch.is_tensor(label) and np.asarray(label).dtype.kind in "iu" and np.asarray(label).dtype != np.uint8:
        label = np.asarray(label).astype(np.float32)
    lab, _ = _device_volume(label, (torch.float32, torch.uint8), what)
    if img.dim() != 4 or np.ndim(image) == 2 or lab.shape != img.shape or lab.device != img.device:
        raise ValueError(f"{what}: a 3-D image (or a batch) and a label of its shape on its device, got {tuple(np.shape(image))} and "
                         f"{tuple(np.shape(label))}")
    target = _target(img.shape[1:], target_shape, 3)
    rec = _stats(img, want_stats=False).record
    out_i = _zoom(img, target, 1, rec, torch.float32, None)
    out_l = _zoom(lab, target, 0, None, torch.uint8, thr)
    return out_i.reshape(lead + target), out_l.reshape(lead + target)


def preprocess_brats_volume(image, seg, target_shape=(192, 192, 64)):
    """One modality and its segmentation as process_brats_case prepares them (BraTS19_DataPreprocessing.py:175-198): normalize_image,
    whole tumour = seg > 0, zoom(order=1) of the image and zoom(order=0) of the label to target_shape, `> 0.5`.
    -> (image float32, label uint8) CUDA tensors of target_shape (with the batch axis of the input, if it has one)."""
    return _preprocess(image, seg, target_shape, 0.0, "preprocess_brats_volume")


def preprocess_isles_volume(image, mask, target_shape=(112, 112, 64)):
    """One modality and its lesion mask as process_isles_bids_case prepares them (ISLES22_DataPreprocessing.py:141-159): normalize_image,
    mask > 0.5, zoom(order=1) / zoom(order=0) to target_shape.  -> (image float32, label uint8); the reference stores both as
    float64, which holds the same values."""
    return _preprocess(image, mask, target_shape, 0.5, "preprocess_isles_volume")
