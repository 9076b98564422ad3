"""fp64 numpy restatement of the blended sliding window (utils/sliding_window.py with ``blend=Blend(...)``): pad, entries, flip,
forward, softmax, un-flip, ``score[sl] += W * p``, ``cnt[sl] += W``, ``score / cnt``, crop.  It shares no code with the package: the
window loop is the reference's (code/utils/test_3d_patch.py:297-321), the tables are the formula of the option's specification.

`nets` is a callable or a list of callables, each mapping a (1, 1, p0, p1, p2) float32 tensor to (1, C, p0, p1, p2) logits; the logits
of a list are averaged before the softmax, as the ensemble evaluator does ((y1_l + y1_r) / 2, :460-463)."""
import itertools
import math

import numpy as np
import torch


def tables(patch_size, weighting="gaussian", sigma_scale=0.125):
    """the three fp32 importance tables: exp(-0.5 * ((i - (p - 1) / 2) / (sigma_scale * p)) ** 2) in fp64, rounded once"""
    out = []
    for p in patch_size:
        if weighting == "constant":
            out.append(np.ones(p, np.float32))
        else:
            out.append(np.array([math.exp(-0.5 * ((i - (p - 1) / 2) / (sigma_scale * p)) ** 2) for i in range(p)], np.float64).astype(np.float32))
    return out


def weight_volume(tabs):
    """W of a window: the fp32 tables' product, taken in fp64"""
    g0, g1, g2 = (t.astype(np.float64) for t in tabs)
    return g0[:, None, None] * g1[None, :, None] * g2[None, None, :]


def masks_of(mirror_axes):
    """every flip mask over the axes, ascending; bit a set = axis a flipped"""
    axes = sorted(mirror_axes)
    return sorted(sum(1 << a for a in combo) for r in range(len(axes) + 1) for combo in itertools.combinations(axes, r))


def windows(shape, patch_size, stride_xy, stride_z):
    """:319-332, on the padded shape"""
    ww, hh, dd = shape
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    return [(min(stride_xy * x, ww - patch_size[0]), min(stride_xy * y, hh - patch_size[1]), min(stride_z * z, dd - patch_size[2]))
            for x in range(sx) for y in range(sy) for z in range(sz)]


def entries(wins, mirror_axes):
    return [(x, y, z, m) for x, y, z in wins for m in masks_of(mirror_axes)]


def _axes(mask):
    return tuple(a for a in range(3) if mask >> a & 1)


def softmax64(logits):
    """(C, ...) float64 -> the max-shifted softmax over axis 0"""
    e = np.exp(logits - logits.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


def accumulate(logits, ents, patch_size, vol_shape, tabs, all_classes=False):
    """What dycon_sw_accumulate_weighted adds to zeroed maps, in fp64.  logits: (M, n, p0, p1, p2, C) of the windows as they went
    through the network, i.e. flipped by their entry's mask.  Returns (score, cnt); score is (C,) + vol_shape with all_classes."""
    logits = np.asarray(logits, np.float64)
    W = weight_volume(tabs)
    C = logits.shape[-1]
    score = np.zeros(((C,) if all_classes else ()) + tuple(vol_shape))
    cnt = np.zeros(vol_shape)
    for n, (x, y, z, mask) in enumerate(ents):
        p = softmax64(np.moveaxis(logits[:, n].mean(0), -1, 0))
        p = np.flip(p, tuple(1 + a for a in _axes(mask)))               # back to the volume's orientation
        sl = (slice(x, x + patch_size[0]), slice(y, y + patch_size[1]), slice(z, z + patch_size[2]))
        if all_classes:
            score[(slice(None),) + sl] += W * p
        else:
            score[sl] += W * p[1]
        cnt[sl] += W
    return score, cnt


def single_case(nets, image, stride_xy, stride_z, patch_size, weighting="constant", sigma_scale=0.125, mirror_axes=(), all_classes=False):
    """(label int64 (w, h, d), prob float64): prob is the class-1 probability (w, h, d) and label = prob > 0.5, or with all_classes
    every class (C, w, h, d) and label = argmax."""
    nets = list(nets) if isinstance(nets, (list, tuple)) else [nets]
    image = np.asarray(image, np.float32)
    shape = image.shape
    pads = [(max(p - s, 0) // 2, max(p - s, 0) - max(p - s, 0) // 2) for s, p in zip(shape, patch_size)]      # :297-316
    padded = np.pad(image, pads, mode="constant", constant_values=0)
    ents = entries(windows(padded.shape, patch_size, stride_xy, stride_z), mirror_axes)
    logits = []
    for x, y, z, mask in ents:
        win = padded[x:x + patch_size[0], y:y + patch_size[1], z:z + patch_size[2]]
        t = torch.from_numpy(np.ascontiguousarray(np.flip(win, _axes(mask)))[None, None])
        with torch.no_grad():
            logits.append([np.moveaxis(net(t)[0].double().numpy(), 0, -1) for net in nets])
    logits = np.moveaxis(np.asarray(logits), 1, 0)                      # (M, n, p0, p1, p2, C)
    score, cnt = accumulate(logits, ents, patch_size, padded.shape, tables(patch_size, weighting, sigma_scale), all_classes)
    prob = score / cnt
    label = prob.argmax(0) if all_classes else (prob > 0.5).astype(np.int64)
    sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, shape))
    return label[sl], prob[(Ellipsis,) + sl]
