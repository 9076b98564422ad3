"""``scipy.ndimage.gaussian_filter`` on the device, bit for bit (csrc/filters.hip).

    gaussian_weights(sigma, truncate)                      host: the fp64 weights scipy forms for one axis (None for sigma 0)
    gaussian_filter_host(a, sigma, mode, truncate)         host: numpy restatement of the kernel (the CPU-testable twin)
    gaussian_filter(t, sigma, mode, truncate, out, scale)  device: dycon_gaussian_filter on the last three axes of a CUDA fp32 tensor

scipy filters the axes in the order 0, 1, 2, stores every intermediate in the output's type (fp32) and sums a line in fp64 in the
symmetric form of its C code::

    r = int(truncate * sigma + 0.5);   w = exp(-0.5 / sigma**2 * x**2) / sum,  x = -r..r         (fp64, on the host)
    acc = x[c] * w[r];   for ii in -r..-1: acc += (x[c + ii] + x[c - ii]) * w[ii + r];   out = fp32(acc)

The twin and the kernel restate exactly that, one rounding per operation, so all three agree in every bit for fp32 input
(tests/test_filters_cpu.py compares the twin with the installed scipy, tests/test_filters_gpu.py the kernel with both).  An axis with
sigma 0 is skipped, as scipy skips it.  Modes: reflect (scipy's default), constant (cval 0) and nearest.  The radius of an axis is at
most MAX_RADIUS = 64 (sigma 13 at truncate 4 gives 52); a larger one is a ValueError.  There is no host fallback.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops

MAX_RADIUS = 64                # DYCON_GAUSS_RMAX
MODES = {"reflect": 0, "constant": 1, "nearest": 2}        # DYCON_FILTER_*


def _sigmas(sigma):
    s = np.atleast_1d(np.asarray(sigma, dtype=np.float64))
    if s.shape == (1,):
        s = np.repeat(s, 3)
    if s.shape != (3,) or not np.isfinite(s).all() or (s < 0).any():
        raise ValueError(f"sigma must be a non-negative number or three of them, got {sigma!r}")
    return [float(v) for v in s]


def gaussian_weights(sigma, truncate=4.0):
    """The 2 r + 1 fp64 weights of ``scipy.ndimage.gaussian_filter1d(sigma, truncate)`` (scipy's expressions), or None for an axis
    scipy skips (sigma <= 1e-15).  ValueError when r exceeds MAX_RADIUS."""
    sigma = float(sigma)
    if sigma <= 1e-15:
        return None
    r = int(float(truncate) * sigma + 0.5)
    if r > MAX_RADIUS:
        raise ValueError(f"gaussian_filter: sigma {sigma} at truncate {truncate} needs the radius {r}; the limit is {MAX_RADIUS}")
    sigma2 = sigma * sigma
    x = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / sigma2 * x ** 2)
    return np.ascontiguousarray(phi / phi.sum())


def _extended(n, r, mode):
    """source index of the positions -r .. n + r - 1 of a line of n extended by `mode` (-1: the constant 0)"""
    i = np.arange(-r, n + r)
    if mode == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def gaussian_filter_host(a, sigma, mode="reflect", truncate=4.0):
    """``scipy.ndimage.gaussian_filter(a, sigma, mode=mode, truncate=truncate)`` over the last three axes of a float32 host array,
    in numpy, operation for operation what the kernel does."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    a = np.asarray(a)
    if a.dtype != np.float32 or a.ndim < 3:
        raise ValueError("gaussian_filter_host takes a float32 array of at least three axes")
    weights = [gaussian_weights(s, truncate) for s in _sigmas(sigma)]
    cur = a
    for axis, w in zip(range(a.ndim - 3, a.ndim), weights):
        if w is None:
            continue
        r, n = len(w) // 2, cur.shape[axis]
        idx = _extended(n, r, mode)
        line = np.moveaxis(cur, axis, -1).astype(np.float64)
        ext = np.where(idx >= 0, line[..., np.maximum(idx, 0)], 0.0)          # positions -r .. n + r - 1
        acc = ext[..., r:r + n] * w[r]
        for ii in range(-r, 0):
            acc = acc + (ext[..., r + ii:r + ii + n] + ext[..., r - ii:r - ii + n]) * w[ii + r]
        cur = np.moveaxis(acc.astype(np.float32), -1, axis)
    return np.ascontiguousarray(cur) if cur is not a else a.copy()


def gaussian_filter(t, sigma, mode="reflect", truncate=4.0, out=None, scale=1.0, workspace=None):
    """``scipy.ndimage.gaussian_filter`` over the last three axes of a CUDA float32 tensor (leading axes are the batch), on the
    current stream, bit for bit.  sigma: a number or three.  out: a contiguous tensor of t's shape (t itself filters in place);
    scale: multiplies the fp32 result in fp32 (1: scipy's bits); workspace: a uint8 tensor of `workspace_bytes` to reuse.
    -> out.  A radius above MAX_RADIUS, another dtype or a tensor that is not on a GPU raise."""
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() >= 3 and t.numel() > 0):
        raise ValueError("gaussian_filter takes a non-empty CUDA float32 tensor of at least three axes")
    weights = [gaussian_weights(s, truncate) for s in _sigmas(sigma)]
    t = t.contiguous()
    if out is None:
        out = torch.empty_like(t)
    elif not (out.shape == t.shape and out.dtype == torch.float32 and out.device == t.device and out.is_contiguous()):
        raise ValueError("out: a contiguous float32 tensor of the input's shape on its device")
    X, Y, Z = (int(v) for v in t.shape[-3:])
    N = t.numel() // (X * Y * Z)
    inplace = out.data_ptr() == t.data_ptr()
    need = workspace_bytes(N, (X, Y, Z), sum(w is not None for w in weights), inplace)
    if workspace is None:
        workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=t.device)
    elif not (workspace.dtype == torch.uint8 and workspace.device == t.device and workspace.is_contiguous() and workspace.numel() >= need):
        raise ValueError(f"workspace: a contiguous uint8 tensor of at least {need} bytes on the input's device")
    args = []
    for w in weights:
        args += [None, 0] if w is None else [w.ctypes.data, len(w) // 2]
    _lib.call("dycon_gaussian_filter", t.data_ptr(), out.data_ptr(), N, X, Y, Z, *args, MODES[mode], float(scale),
              workspace.data_ptr(), workspace.numel(), ops._s())
    return out


def workspace_bytes(N, shape, naxes=3, inplace=False):
    """bytes of workspace `gaussian_filter` needs for N volumes of `shape` with `naxes` filtered axes"""
    X, Y, Z = (int(v) for v in shape)
    return int(_lib.query("dycon_gaussian_filter_workspace", int(N), X, Y, Z, int(naxes), int(bool(inplace))))
