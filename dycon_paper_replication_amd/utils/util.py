"""The reference's code/utils/util.py: the signed-distance target of the nets' first output (the `tanh` head), on the device, and the
module's host helpers.

    compute_sdf(img_gt, out_shape)                      -> float64 numpy array of out_shape            (code/utils/util.py:205-236)
    compute_sdf_device(labels, out_shape=None, dtype=torch.float32, normalize=True, classes=None)
                                                        -> CUDA tensor on the current stream, nothing read back
    AverageMeter, UnifLabelSampler, learning_rate_decay, Logger, save_checkpoint, load_checkpoint, restore_model

Both SDF forms run csrc/sdf.hip: an exact int32 squared Euclidean distance transform to the background and to the foreground of every
sample, the per-sample maxima by integer atomics, and one fp64 pass that writes -(sqrt(d2) / sqrt(max)) inside the mask,
+(sqrt(d2) / sqrt(max)) outside it and +0.0 on the inner boundary (a foreground voxel with a background 6-neighbour inside the volume:
skimage's find_boundaries(mode="inner"), which pads the volume so that its faces make no boundary).  That is the reference's
expression bit for bit whenever a sample has both a foreground and a background voxel.  A sample without
foreground is +0.0 everywhere, as in the reference; a sample without background is NaN everywhere, as in the reference (its 0 / 0).
Every axis of the volume is at most 512.  Unit voxel spacing and 3-D volumes only.

Foreground with `classes=None` is `label != 0` after the reference's `astype(np.uint8)`: a float label is truncated towards zero
first (0.5 is background).  One difference is kept on purpose: an integer label that is a non-zero multiple of 256 is foreground
here, where the reference's uint8 cast wraps it to background.

Not provided, with the reason:
    load_model          reads `models.__dict__`, a module the reference never imports or defines: it cannot run there either
    load_ddp_to_nddp    assigns into `model_dict` before binding it: it raises on the first key that contains "module"
    distributed_setup   the trainer's data-parallel path (trainer.py) owns the process-group setup
"""
from __future__ import annotations

import os
import pickle

import numpy as np
import torch
from torch.utils.data.sampler import Sampler

from .. import _lib

MAX_AXIS = 512
MAX_MAPS = 32767                  # maps (samples x classes) per launch sequence; more go in chunks
WORKSPACE_BUDGET = 1 << 30        # bytes of distance-transform workspace per launch sequence
# (device index, stream, bytes) -> uint8 tensor.  utils/surface.py allocates its workspace on every call; a training loop calls with
# one shape on one stream, so the buffer is kept.  Keyed by stream because the buffer must not be shared between streams.  At most
# _WORKSPACE_SLOTS entries, the oldest dropped first: a loop that alternates more shapes or streams than that allocates its
# workspace anew on each call (from torch's caching allocator), which is what surface.py pays on every call.
_WORKSPACES = {}
_WORKSPACE_SLOTS = 4


# ------------------------------------------------------------------------------------------------ signed distance maps
def _plan(label_shape, out_shape, classes):
    """Everything that can be refused, from shapes alone: -> (n_vol, (X, Y, Z), lo, n_cls, n_rep, result shape, expand).  `n_rep`
    is the number of consecutive copies of a map the kernel writes; `expand` is the shape a plain map is broadcast to afterwards
    when a size-1 axis of the volume has to grow (None otherwise).  out_shape[1:] must have the volume's three axes or more: numpy's
    assignment would also drop leading size-1 axes of the volume, a (1, 1, 5) volume into (B, 5); that is refused here."""
    label_shape = tuple(int(n) for n in label_shape)
    if len(label_shape) != 4:
        raise ValueError(f"labels must be (B, x, y, z): 3-D volumes per sample, got {label_shape}")
    B, vol = label_shape[0], label_shape[1:]
    if B < 1 or not all(1 <= n <= MAX_AXIS for n in vol):
        raise ValueError(f"every axis of the volume must be in 1..{MAX_AXIS} and the batch not empty, got {label_shape}")
    if classes is not None:
        lo, hi = (int(v) for v in classes)
        if lo < 1 or hi < lo or hi > 255:
            raise ValueError(f"classes = (lo, hi) takes 1 <= lo <= hi <= 255, got {classes}")
        if out_shape is not None and tuple(int(n) for n in out_shape) != (B, hi - lo + 1) + vol:
            raise ValueError(f"with classes = {classes} the result is {(B, hi - lo + 1) + vol}, got out_shape = {tuple(out_shape)}")
        return B, vol, lo, hi - lo + 1, 1, (B, hi - lo + 1) + vol, None
    if out_shape is None:
        return B, vol, 0, 1, 1, label_shape, None
    out_shape = tuple(int(n) for n in out_shape)
    if len(out_shape) < 1 or out_shape[0] != B:
        raise ValueError(f"out_shape {out_shape} must start with the batch size of the labels, {B}")
    n_vol, per = B, out_shape[1:]
    try:
        ok = np.broadcast_shapes(vol, per) == per
    except ValueError:
        ok = False
    if not ok:
        raise ValueError(f"a volume of {vol} does not broadcast into out_shape[1:] = {per}")
    if len(per) >= 3 and per[-3:] == vol:
        return n_vol, vol, 0, 1, int(np.prod(per[:-3], dtype=np.int64)), out_shape, None
    return n_vol, vol, 0, 1, 1, out_shape, out_shape            # a size-1 axis of the volume grows


def _kernel_labels(labels):
    """uint8 or int64, contiguous.  uint8, bool and int64 go as they are; other integers widen to int64; floats are truncated"""
    if labels.dtype == torch.bool:
        labels = labels.contiguous().view(torch.uint8)
    elif labels.dtype not in (torch.uint8, torch.int64):
        labels = labels.to(torch.int64)
    return labels.contiguous()


def _workspace(device, nbytes):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, nbytes)
    ws = _WORKSPACES.get(key)
    if ws is None:
        while len(_WORKSPACES) >= _WORKSPACE_SLOTS:
            _WORKSPACES.pop(next(iter(_WORKSPACES)))
        ws = _WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def compute_sdf_device(labels, out_shape=None, dtype=torch.float32, normalize=True, classes=None):
    """Signed distance maps of CUDA labels (B, x, y, z), uint8 or int64 with any strides (bool, other integers and floats holding
    integers are converted on the device), as a CUDA tensor of `dtype` (float32 or float64) on the current stream.  Nothing is read
    back and nothing synchronises.

    classes=None      the reference's foreground map, label != 0: the result is (B, x, y, z), or `out_shape` as compute_sdf takes
                      it, e.g. the shape of the nets' first output, (B, C, x, y, z): every channel gets the map
    classes=(lo, hi)  one map per label value lo..hi: (B, hi - lo + 1, x, y, z), the targets of a C-class head.  A class that a
                      sample does not contain reads +0.0, the reference's empty-mask branch
    normalize=False   the signed distance in voxels (no division by the per-sample maxima), same zeroed boundary, same NaN rule

    ValueError, before any launch: an axis above 512, labels that are not 3-D per sample, an out_shape the volume does not
    broadcast into or whose batch size is not the labels' (compute_sdf keeps the reference's reading of out_shape[0] samples)."""
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"dtype must be torch.float32 or torch.float64, got {dtype}")
    if not torch.is_tensor(labels):
        raise TypeError("compute_sdf_device takes a CUDA tensor; compute_sdf takes numpy arrays")
    n_vol, (X, Y, Z), lo, n_cls, n_rep, shape, expand = _plan(labels.shape, out_shape, classes)
    if not labels.is_cuda:
        raise ValueError("compute_sdf_device takes CUDA labels; compute_sdf moves host labels to the device")
    dev = labels.device
    lab = _kernel_labels(labels)
    out = torch.empty((n_vol * n_cls, n_rep, X, Y, Z), dtype=dtype, device=dev)
    per_vol = int(_lib.query("dycon_sdf_workspace", n_cls, X, Y, Z))
    step = max(1, min(n_vol, WORKSPACE_BUDGET // per_vol, MAX_MAPS // n_cls))
    with torch.cuda.device(dev):
        ws = _workspace(dev, step * per_vol)
        stream = torch.cuda.current_stream(dev).cuda_stream
        for v0 in range(0, n_vol, step):
            nv = min(step, n_vol - v0)
            _lib.call("dycon_sdf", lab[v0:].data_ptr(), lab.element_size(), nv, lo, n_cls, X, Y, Z, int(bool(normalize)), n_rep,
                      out.element_size(), out[v0 * n_cls:].data_ptr(), ws.data_ptr(), ws.numel(), stream)
    if expand is not None:
        return out.view((n_vol, X, Y, Z)).reshape((n_vol,) + (1,) * (len(expand) - 4) + (X, Y, Z)).expand(expand).contiguous()
    return out.view(shape)


def compute_sdf(img_gt, out_shape):
    """compute_sdf of code/utils/util.py:205-236: img_gt (B, x, y, z), numpy or a tensor on any device, integer, bool or float ->
    the normalised signed distance map as a float64 numpy array of out_shape: negative inside, positive outside, 0 on the inner
    boundary, range [-1, 1].  out_shape is (B, x, y, z) or anything a volume broadcasts into per sample, (B, 1, x, y, z) for one.
    As the reference loops over range(out_shape[0]), an out_shape with a smaller batch size than img_gt's takes the first samples.
    Computed on the device; labels that already live there stay there on the way in."""
    if not torch.is_tensor(img_gt):
        img_gt = np.asarray(img_gt)
    out_shape = tuple(int(n) for n in out_shape)
    if len(img_gt.shape) == 4 and out_shape and 1 <= out_shape[0] < img_gt.shape[0]:
        img_gt = img_gt[:out_shape[0]]
    _plan(img_gt.shape, out_shape, None)
    lab = img_gt if torch.is_tensor(img_gt) else torch.from_numpy(np.ascontiguousarray(img_gt))
    if not lab.is_cuda:
        lab = lab.to("cuda")
    return compute_sdf_device(lab, out_shape, dtype=torch.float64).cpu().numpy()


# ------------------------------------------------------------------------------------------------ host helpers
# Written for this package from the behaviour of code/utils/util.py:55-202; the attribute and key names are the interface the
# reference's training scripts and checkpoint files use.  tests/golden/sdf.npz holds traces recorded from the reference's own classes.
def save_checkpoint(epoch, model, optimizer, loss, path):
    """One file with the keys the reference writes: epoch, state_dict, optimizer_state_dict, loss."""
    payload = dict(epoch=epoch, state_dict=model.state_dict(), optimizer_state_dict=optimizer.state_dict(), loss=loss)
    torch.save(payload, path)


def load_checkpoint(path, model, optimizer, from_ddp=False):
    """Load a file of save_checkpoint into `model` and `optimizer` -> (model, optimizer, epoch, loss as a Python float).  The loss
    must have been saved as a tensor (the reference calls `.item()` on it); `from_ddp` is accepted and ignored, as there."""
    del from_ddp
    saved = torch.load(path)
    model.load_state_dict(saved["state_dict"])
    optimizer.load_state_dict(saved["optimizer_state_dict"])
    return model, optimizer, saved["epoch"], saved["loss"].item()


def _newest_checkpoint(folder, tag):
    """(file name, iteration) by the reference's matching rules, which restore_model documents; raises when nothing matches"""
    names = [n for n in os.listdir(folder) if tag in n]
    newest = max(int(os.path.splitext(n)[0].split("_")[2]) for n in names)
    return [n for n in names if str(newest) in n][-1], newest


def restore_model(logger, snapshot_path, model_num=None, *, model=None, optimizer=None):
    """Find the newest checkpoint in `snapshot_path` and load it -> (model, optimizer, start_epoch, performance), or None, with a
    warning on `logger`, when nothing could be restored.

    The reference reads `model` and `optimizer` without ever binding them, so its own call always ends in the warning branch and
    returns None; here they are keyword arguments, and leaving them out gives exactly that.  Its other habits are kept:
      * a file takes part when the tag ("model_iter", or `model_num` when that is given) occurs anywhere in its name, and its
        iteration is the third "_"-separated field of the name without extension: "model_iter_6000.pth" -> 6000; a matching file
        without such a number ends the search with the warning;
      * the chosen file is the LAST one in os.listdir order whose name contains both the tag and the digits of the largest
        iteration as a substring, so "model_iter_16000.pth" can stand in for iteration 6000 when 6000 is not the maximum's name."""
    logger.info(f"Snapshot path: {snapshot_path}")
    try:
        filename, iteration = _newest_checkpoint(snapshot_path, model_num or "model_iter")
    except Exception as e:
        logger.warning(f"Error finding previous checkpoints: {e}")
        logger.warning("Unable to restore model checkpoint: none found, using new model")
        return None
    logger.info(f"Restoring model checkpoint: {filename}")
    if model is None or optimizer is None:
        logger.warning("Unable to restore model checkpoint: model and optimizer must be given as keyword arguments, using new model")
        return None
    try:
        restored = load_checkpoint(os.path.join(snapshot_path, filename), model, optimizer)
    except Exception as e:
        logger.warning(f"Unable to restore model checkpoint: {e}, using new model")
        return None
    logger.info(f"Models restored from iteration {iteration}")
    return restored


class UnifLabelSampler(Sampler):
    """N indices spread evenly over pseudolabels; images_lists[k] lists the items of pseudolabel k.  Every pseudolabel contributes
    N // K + 1 draws (with replacement only when it has no more items than that), the pool is shuffled once and cut to N.  The calls
    into np.random -- one `choice` per pseudolabel in order, then one `shuffle` of the pool -- are those of the reference, so a
    seeded run yields its indices."""

    def __init__(self, N, images_lists):
        self.N = N
        self.images_lists = images_lists
        self.indexes = self.generate_indexes_epoch()

    def generate_indexes_epoch(self):
        share = self.N // len(self.images_lists) + 1
        draws = [np.random.choice(members, share, replace=len(members) <= share)
                 for members in (self.images_lists[k] for k in range(len(self.images_lists)))]
        pool = np.concatenate(draws).astype(np.float64)
        np.random.shuffle(pool)
        return pool[:self.N].astype(np.int64)

    def __iter__(self):
        return iter(self.indexes)

    def __len__(self):
        return self.N


class AverageMeter:
    """`val` is the last value, `avg` the mean of all values weighted by their `n`; `sum` and `count` are its two parts."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.count += n
        self.sum += n * val
        self.avg = self.sum / self.count


def learning_rate_decay(optimizer, t, lr_0):
    """Every parameter group gets lr_0 / sqrt(1 + lr_0 * weight_decay * t), with its own weight decay (DeepCluster's schedule)."""
    for group in optimizer.param_groups:
        group["lr"] = lr_0 / np.sqrt(1 + lr_0 * group["weight_decay"] * t)


class Logger:
    """`log(point)` appends to `data` and rewrites the whole list as a pickle at `path`."""

    def __init__(self, path):
        self.path = path
        self.data = []

    def log(self, train_point):
        self.data.append(train_point)
        with open(self.path, "wb") as fh:
            pickle.dump(self.data, fh, pickle.HIGHEST_PROTOCOL)
