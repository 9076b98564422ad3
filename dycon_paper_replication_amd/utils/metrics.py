"""Train-time metrics with the reference's names (code/utils/metrics.py; used at code/train_DyCON_BraTS19.py:385-395) -- SURVEY 8f-4.

The reference computes, EVERY iteration, a batch Dice on the GPU and a medpy HD95 per sample on the host (a device->host copy
of the binary volumes plus two distance transforms per sample: more host time than the whole HIP step).  Here

  * `batch_dice_from_logits` / `compute_dice` / `compute_jaccard` count on the device (csrc/eval.hip) and return device tensors
    without a host sync;
  * `compute_hd95` keeps the reference's semantics (max_dist for an empty mask) on scipy ("parity unpinned": medpy absent);
  * `AsyncTrainMetrics` takes it off the critical path: every `every`-th iteration the binary maps are copied to pinned memory
    asynchronously and a worker thread computes HD95 while the GPU trains on;
  * `compute_hd95_device` and `AsyncTrainMetrics(on_device=True)` are the opt-in device form (utils/surface.py, csrc/surface.hip):
    exact surface distances, a device tensor back, no host copy, no worker; `compute_hd95_device` also takes medpy's
    `voxelspacing` and `connectivity` (csrc/surface_spacing.hip).

Those names are 2-class and refuse another width.  For 2..8 classes, under names of their own: `class_dice_from_logits` (per sample
and foreground class, from one confusion count over the logits, csrc/evalc.hip), `AsyncClassTrainMetrics`, the device path of
`cal_dice`, and the reference's `dice` (utils/metrics.py:39-75), which its ISLES script validates with.
"""
from __future__ import annotations

import queue
import threading

import numpy as np
import torch

from .. import _lib
from . import surface
from .test_3d_patch import _surface_distances


def _counts(logits_ndhwc2, labels):
    B = logits_ndhwc2.shape[0]
    V = logits_ndhwc2.numel() // (2 * B)
    lab = labels.contiguous()
    if lab.dtype not in (torch.uint8, torch.int64):
        lab = lab.ne(0).to(torch.uint8)
    out = torch.zeros((B, 3), dtype=torch.int64, device=logits_ndhwc2.device)
    _lib.call("dycon_batch_overlap", logits_ndhwc2.data_ptr(), lab.data_ptr(), lab.element_size(), B, V, out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return out.double()


def _two_class_ndhwc(logits):
    """(B, 2, D, H, W) or (B, D, H, W, 2) -> the (B, D, H, W, 2) view; any other class width is refused here, before a kernel is sized
    with it (the train-time metrics are 2-class)."""
    if logits.dim() != 5:
        raise ValueError(f"expected 5-D logits (B, 2, D, H, W) or (B, D, H, W, 2), got {tuple(logits.shape)}")
    lg = logits if logits.shape[-1] == 2 and logits.shape[1] != 2 else logits.permute(0, 2, 3, 4, 1)
    if lg.shape[-1] != 2:
        raise ValueError(f"the train-time metrics take 2-class logits, got a class axis of width {lg.shape[-1]} "
                         f"(shape {tuple(logits.shape)})")
    return lg


def batch_dice_from_logits(logits, labels):
    """logits (B, 2, D, H, W) as the HIP nets return them (channels-last-3D view) or (B, D, H, W, 2); labels (B, D, H, W).
    Per-sample Dice of (softmax(logits)[:, 1] > 0.5) against labels, = metrics.compute_dice(outputs_bin, label) of the reference
    (train_DyCON_BraTS19.py:387-389), as a device tensor (no sync)."""
    lg = _two_class_ndhwc(logits)
    c = _counts(lg.contiguous().float(), labels)
    return 2.0 * c[:, 2] / (c[:, 0] + c[:, 1] + 1e-8)


def _binary_counts(output, label):
    out = torch.as_tensor(output)
    lab = torch.as_tensor(label)
    if not out.is_cuda:
        out, lab = out.cuda(), lab.cuda()
    B = out.shape[0]
    # binary maps -> two-channel "logits" whose argmax is the map: reuse the fused kernel
    lg = torch.stack([torch.zeros_like(out, dtype=torch.float32), out.float() - 0.5], dim=-1).reshape(B, -1, 2).contiguous()
    return _counts(lg, lab.reshape(B, -1))


def compute_dice(output, label):
    """Batch-wise Dice of binary volumes (B, ...): 2|A&B| / (|A| + |B| + 1e-8)  (utils/metrics.py:85-95)."""
    c = _binary_counts(output, label)
    return 2.0 * c[:, 2] / (c[:, 0] + c[:, 1] + 1e-8)


def compute_jaccard(output, label):
    """Batch-wise Jaccard / IoU (utils/metrics.py:98-109)."""
    c = _binary_counts(output, label)
    return c[:, 2] / (c[:, 0] + c[:, 1] - c[:, 2] + 1e-8)


def _check_classes(C):
    if not 2 <= int(C) <= 8:
        raise ValueError(f"the class-count metrics take 2..8 classes, got {C}")
    return int(C)


def _label_operand(t):
    """ground-truth labels as the confusion kernels read them: uint8 or int64, contiguous"""
    return (t if t.dtype in (torch.uint8, torch.int64) else t.to(torch.int64)).contiguous()


def _class_confusion(pred, gt, C):
    """CUDA label maps -> the (C*C + 1,) int64 counters of dycon_class_confusion: [p*C + g] and, last, the voxels whose prediction or
    label lies outside [0, C).  No host sync."""
    C = _check_classes(C)
    if pred.numel() != gt.numel():
        raise ValueError(f"prediction {tuple(pred.shape)} and label {tuple(gt.shape)} differ in size")
    if pred.dtype != torch.uint8:       # the kernel reads uint8 predictions: keep an out-of-range value out of range
        pred = torch.where((pred < 0) | (pred >= C), 255, pred).to(torch.uint8)
    p, g = pred.contiguous(), _label_operand(gt.to(pred.device))
    out = torch.zeros(C * C + 1, dtype=torch.int64, device=p.device)
    _lib.call("dycon_class_confusion", p.data_ptr(), g.data_ptr(), g.element_size(), p.numel(), C, out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return out


def _class_ndhwc(logits, labels):
    """(B, C, D, H, W) (what the HIP nets return: a channels-last-3D view) or (B, D, H, W, C) -> the (B, D, H, W, C) view.  The labels'
    (B, D, H, W) say which of the two it is."""
    if logits.dim() != 5 or labels.dim() != 4:
        raise ValueError(f"expected 5-D logits and (B, D, H, W) labels, got {tuple(logits.shape)} and {tuple(labels.shape)}")
    if logits.shape[:1] + logits.shape[2:] == labels.shape:
        lg = logits.permute(0, 2, 3, 4, 1)
    elif logits.shape[:-1] == labels.shape:
        lg = logits
    else:
        raise ValueError(f"logits {tuple(logits.shape)} do not match labels {tuple(labels.shape)}")
    _check_classes(lg.shape[-1])
    return lg


def class_dice_from_logits(logits, labels):
    """logits (B, C, D, H, W) or (B, D, H, W, C), C in 2..8; labels (B, D, H, W) with values in [0, C).  Per sample and foreground
    class 1..C-1 the Dice of argmax(logits) against labels, 2 I / (P + G + 1e-8) (cal_dice's arithmetic, utils/metrics.py:14-27), as a
    (B, C-1) float64 device tensor: the counts come from the logits in one pass (dycon_batch_class_confusion), no host sync.  A voxel
    whose label lies outside [0, C) is counted for no class."""
    return _class_dice_ndhwc(_class_ndhwc(logits, labels).contiguous().float(), labels)


def _class_dice_ndhwc(lg, labels):
    B, C = lg.shape[0], lg.shape[-1]
    lab = _label_operand(labels)
    out = torch.zeros((B, C * C + 1), dtype=torch.int64, device=lg.device)
    _lib.call("dycon_batch_class_confusion", lg.data_ptr(), lab.data_ptr(), lab.element_size(), B, lg.numel() // (B * C), C,
              out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    conf = out[:, :C * C].reshape(B, C, C).double()                         # [b, pred, gt]
    inter = torch.diagonal(conf, dim1=1, dim2=2)
    return (2.0 * inter / (conf.sum(2) + conf.sum(1) + 1e-8))[:, 1:]


def dice(input, target, ignore_index=None):
    """The reference's `dice` (utils/metrics.py:39-75): (2 sum(i * t) + 1) / (sum(i) + sum(t) + 1) over all elements, both sides zeroed
    where target == ignore_index.  numpy arrays (taken as float32, as the reference does) or tensors; computed on the device, returned
    as a 0-dim device tensor."""
    smooth = 1.0
    if isinstance(input, np.ndarray):
        input = torch.from_numpy(input.astype(np.float32))
    if isinstance(target, np.ndarray):
        target = torch.from_numpy(target.astype(np.float32))
    dev = input.device if input.is_cuda else target.device if target.is_cuda else torch.device("cuda")
    iflat, tflat = input.to(dev).reshape(-1), target.to(dev).reshape(-1)
    if ignore_index is not None:
        mask = tflat == ignore_index
        iflat, tflat = iflat.masked_fill(mask, 0), tflat.masked_fill(mask, 0)
    dt = torch.promote_types(iflat.dtype, tflat.dtype)
    dt = dt if dt.is_floating_point else torch.float32
    inter, total = (iflat.double() * tflat.double()).sum(), iflat.double().sum() + tflat.double().sum()
    return ((2.0 * inter + smooth) / (total + smooth)).to(dt)


def cal_dice(prediction, label, num=2):
    """Multi-class Dice on label maps, classes 1..num-1 (utils/metrics.py:14-27); numpy in, numpy out.  Two CUDA tensors are counted
    on the device (dycon_class_confusion) and give the num - 1 values as a float64 device tensor, without a host sync."""
    if torch.is_tensor(prediction) and torch.is_tensor(label) and prediction.is_cuda and label.is_cuda:
        # a value outside [0, num) equals no i of the loop below on its own side only: fold it into class 0, which is not reported,
        # so that the voxel still counts for the other side's class
        fold = lambda t: torch.where((t < 0) | (t >= num), 0, t)  # noqa: E731
        conf = _class_confusion(fold(prediction), fold(label), num)[:num * num].reshape(num, num).double()          # [pred, gt]
        return (2.0 * torch.diagonal(conf) / (conf.sum(1) + conf.sum(0) + 1e-8))[1:]
    total = np.zeros(num - 1)
    for i in range(1, num):
        p, g = (np.asarray(prediction) == i), (np.asarray(label) == i)
        total[i - 1] += 2 * np.sum(p & g) / (np.sum(p) + np.sum(g) + 1e-8)
    return total


def compute_hd95(pred, target, max_dist):
    """Per-sample HD95 with the reference's conventions (utils/metrics.py:112-131): max_dist when either mask is empty."""
    pred = pred.cpu().numpy() if torch.is_tensor(pred) else np.asarray(pred)
    target = target.cpu().numpy() if torch.is_tensor(target) else np.asarray(target)
    scores = []
    for p, t in zip(pred, target):
        if np.sum(p) == 0 or np.sum(t) == 0:
            scores.append(max_dist)
        else:
            hd1, hd2 = _surface_distances(p != 0, t != 0), _surface_distances(t != 0, p != 0)
            scores.append(float(np.percentile(np.hstack((hd1, hd2)), 95)))
    return scores


def compute_hd95_device(pred, target, max_dist, voxelspacing=None, connectivity=1):
    """`compute_hd95` on the device (utils/surface.py): pred / target are (B, X, Y, Z) binary volumes, numpy or CUDA; returns a (B,)
    float64 device tensor.  A sample where either mask is empty gets max_dist (utils/metrics.py:117-118), selected on the device: no
    host copy and no sync.  voxelspacing / connectivity are medpy's (`surface.surface_metrics`); the defaults are unit spacing and
    6-neighbour borders, as the reference calls hd95."""
    if len(pred.shape) != 4:
        raise ValueError(f"compute_hd95_device takes (B, X, Y, Z) volumes, got {tuple(pred.shape)}")
    hd = surface.surface_metrics(pred, target, voxelspacing=voxelspacing, connectivity=connectivity)[:, 0]
    return torch.where(torch.isnan(hd), torch.full_like(hd, float(max_dist)), hd)     # NaN = an empty border = an empty mask


class AsyncTrainMetrics:
    """Per-iteration Dice on the device, HD95 every `every` iterations on a worker thread.

        m = AsyncTrainMetrics(every=50)
        m.update(iter_num, out["s_logits"], label)     # never blocks on the GPU
        m.latest()  ->  {"iter": .., "dice": tensor (device), "hd95": (iter, mean) or None}

    With `on_device=True` there is no worker thread, no pinned buffer and no queue: every `every`-th `update` enqueues
    `compute_hd95_device` on the current stream and "hd95" is (iter, 0-dim device tensor of the batch mean).
    """

    def __init__(self, every=50, on_device=False):
        self.every = every
        self.on_device = bool(on_device)
        self._hd = None
        self._dice = None
        self._iter = -1
        self._q = self._t = None
        if not self.on_device:
            self._q = queue.Queue(maxsize=2)
            self._t = threading.Thread(target=self._work, daemon=True)
            self._t.start()

    def _work(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            it, ev, pred, lab, max_dist = item
            ev.synchronize()
            self._hd = (it, float(np.mean(compute_hd95(pred.numpy(), lab.numpy(), max_dist))))

    def update(self, iter_num, logits, labels):
        lg = _two_class_ndhwc(logits)
        self._iter = iter_num
        self._dice = batch_dice_from_logits(logits, labels)
        if self.on_device:
            if self.every and iter_num % self.every == 0:
                pred = (lg[..., 1] > lg[..., 0]).to(torch.uint8)
                self._hd = (iter_num, compute_hd95_device(pred, labels, float(np.linalg.norm(pred.shape[1:]))).mean())
            return
        if self.every and iter_num % self.every == 0 and not self._q.full():
            pred = (lg[..., 1] > lg[..., 0]).to(torch.uint8)
            ph = torch.empty(pred.shape, dtype=torch.uint8).pin_memory()
            lh = torch.empty(labels.shape, dtype=torch.uint8).pin_memory()
            ph.copy_(pred, non_blocking=True)
            lh.copy_(labels.ne(0).to(torch.uint8), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._q.put((iter_num, ev, ph, lh, float(np.linalg.norm(pred.shape[1:]))))

    def latest(self):
        return {"iter": self._iter, "dice": self._dice, "hd95": self._hd}

    def close(self):
        if self._q is not None:
            self._q.put(None)


class AsyncClassTrainMetrics(AsyncTrainMetrics):
    """AsyncTrainMetrics for 2..8 classes: `class_dice_from_logits` every iteration ("dice": a (B, C-1) device tensor), and every
    `every`-th iteration the HD95 of class 1 (argmax == 1 against label == 1) on the worker thread."""

    def update(self, iter_num, logits, labels):
        lg = _class_ndhwc(logits, labels).contiguous().float()
        self._iter = iter_num
        self._dice = _class_dice_ndhwc(lg, labels)
        if self.on_device:
            if self.every and iter_num % self.every == 0:
                arg = torch.empty(labels.shape, dtype=torch.uint8, device=lg.device)
                _lib.call("dycon_argmax_labels", lg.data_ptr(), lg.shape[-1], arg.numel(), arg.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
                hd = surface.surface_metrics(arg, labels, classes=(1, 1))[:, 0]         # class 1 straight from the label maps
                max_dist = float(np.linalg.norm(labels.shape[1:]))
                self._hd = (iter_num, torch.where(torch.isnan(hd), torch.full_like(hd, max_dist), hd).mean())
            return
        if self.every and iter_num % self.every == 0 and not self._q.full():
            arg = torch.empty(labels.shape, dtype=torch.uint8, device=lg.device)
            _lib.call("dycon_argmax_labels", lg.data_ptr(), lg.shape[-1], arg.numel(), arg.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
            ph = torch.empty(labels.shape, dtype=torch.uint8).pin_memory()
            lh = torch.empty(labels.shape, dtype=torch.uint8).pin_memory()
            ph.copy_(arg.eq(1).to(torch.uint8), non_blocking=True)
            lh.copy_(labels.eq(1).to(torch.uint8), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._q.put((iter_num, ev, ph, lh, float(np.linalg.norm(labels.shape[1:]))))
