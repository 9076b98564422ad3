"""Multi-class evaluation: the all-class sliding window and per-class metrics (csrc/evalc.hip).

``utils.test_3d_patch.test_single_case`` scores class 1 only, as the reference does (code/utils/test_3d_patch.py:337-347): it is
the reference-compatible evaluator.  The functions here are the standard multi-class form it was derived from, under names of their
own, through the same driver (``sliding_window._sliding_window(..., all_classes=True)``) and the same case loop
(``case_loop.mean_over_cases``): every window adds its whole C-way softmax to a class-major (C, w, h, d) score map, the label
map is the argmax of the averaged scores (lowest index on ties, as ``np.argmax``), and Dice / Jaccard are taken per foreground class
from one C x C confusion matrix counted on the device.  HD95 / ASD stay on the host (``case_loop.hd95_asd``), one binary pair per class, unless
``device_surface=True`` asks for the device form (``utils/surface.py``: all classes of a case in one set of launches).

    test_single_case_classes(model, image, stride_xy, stride_z, patch_size)     -> (label_map, score_map) as numpy
    single_case_classes_device(...)                                             -> the same as device tensors, no host copies
    confusion_counts(pred, gt, num_classes)                                     -> (C, C) int64 device tensor, [pred, gt]
    metrics_from_confusion(conf)                                                -> (C-1, 2) Dice / Jaccard
    calculate_metric_perclass(pred, gt, num_classes)                            -> (C-1, 4) dice, jaccard, hd95, asd
    test_all_case_classes(model, cases, num_classes, patch_size, ...)           -> mean (C-1, 4) over the cases
    isles_val_dice(model, volume, label, patch_size)                            -> code/train_DyCON_ISLES22.py:351-370 for one case
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import components, metrics, morphology, surface
from .case_loop import dc_jc as _dc_jc, hd95_asd as _hd95_asd, mean_over_cases as _mean_over_cases
from .sliding_window import _sliding_window, _stream, chunk_box  # noqa: F401  (chunk_box: public here, tools/eval_bench.py and the tests)


def single_case_classes_device(model, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None):
    """The device-resident form of `test_single_case_classes`: (label uint8 (w, h, d), score float32 (C, w, h, d)) as CUDA tensors,
    without host copies.  blend: None or a `sliding_window.Blend`."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("test_single_case_classes runs on the MI355X only: move the model to 'cuda'")
    C = getattr(model, "n_classes", None)
    if C is not None and C < 2:
        raise ValueError("test_single_case_classes takes the argmax over the classes: the model needs at least 2 classes")
    declared = [C]                                              # a model that declares no class count: its first logits do

    def forward(patches):
        logits = model(patches)[1]
        if declared[0] is None:
            declared[0] = int(logits.shape[1])
        if not 2 <= declared[0] <= 8:
            raise ValueError(f"test_single_case_classes takes models of 2..8 classes, got {declared[0]}")
        if logits.shape[1] != declared[0]:
            raise ValueError(f"the model declares {declared[0]} classes and returns logits of {logits.shape[1]}")
        return logits

    return _sliding_window([model], [forward], image, stride_xy, stride_z, patch_size, batch_size, dev, all_classes=True, blend=blend)


def test_single_case_classes(model, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None):
    """image: (w, h, d) numpy array or tensor.  Returns (label_map int64 (w, h, d) with values in [0, C), score_map float32
    (C, w, h, d)) as numpy: score_map[c] is the class-c probability averaged over the windows that cover a voxel, label_map its argmax
    over c.  Padding, window list, crop and the handling of the model's mode are `sliding_window.test_single_case`'s; C is the
    model's `n_classes`, or the channel count of its logits when it declares none.  `batch_size` windows go through the network per
    launch sequence.  blend: None, the plain mean over the windows, or a `sliding_window.Blend`."""
    label, score = single_case_classes_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device,
                                              blend=blend)
    return label.cpu().numpy().astype(np.int64), score.cpu().numpy()


def _as_device_labels(a, dev=None):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    if dev is None:
        dev = t.device if t.is_cuda else torch.device("cuda:0")
    t = t.to(dev)
    return t if t.dtype in (torch.uint8, torch.int64) else t.to(torch.int64)


def confusion_counts(pred, gt, num_classes):
    """The C x C confusion matrix of two label maps (CUDA tensors or numpy arrays of equal size) as an int64 device tensor indexed
    [pred, gt], counted in one pass (dycon_class_confusion).  ValueError when a prediction or a label lies outside [0, C)."""
    C = int(num_classes)
    p = _as_device_labels(pred)
    out = metrics._class_confusion(p, _as_device_labels(gt, p.device), C)
    bad = int(out[C * C])
    if bad:
        raise ValueError(f"{bad} voxels have a prediction or a label outside [0, {C})")
    return out[:C * C].reshape(C, C)


def metrics_from_confusion(conf):
    """(C, C) confusion counts indexed [pred, gt] -> (C-1, 2) Dice / Jaccard of the classes 1..C-1, each with medpy's dc / jc arithmetic
    on the class's binary pair (a class absent from both maps has no Jaccard: ZeroDivisionError, as medpy).  Host arithmetic only."""
    conf = np.asarray(conf.cpu() if torch.is_tensor(conf) else conf)
    if conf.ndim != 2 or conf.shape[0] != conf.shape[1] or conf.shape[0] < 2:
        raise ValueError(f"expected a (C, C) confusion matrix with C >= 2, got {conf.shape}")
    return np.array([_dc_jc(int(conf[c].sum()), int(conf[:, c].sum()), int(conf[c, c])) for c in range(1, conf.shape[0])])


def calculate_metric_perclass(pred, gt, num_classes, device_surface=False, voxelspacing=None, connectivity=1):
    """(C-1, 4) array of (dice, jaccard, hd95, asd), one row per foreground class, each `calculate_metric_percase(pred == c, gt == c)`
    (code/utils/test_3d_patch.py:496-508) with the reference's conventions for empty masks: a class the prediction does not contain
    gives (0, 0, 0, 0) (:268-271), a class absent from the ground truth hd95 = asd = 0 (:500-503).  Dice and Jaccard come from the
    device counts; the surface distances run on the host, or, with device_surface=True, for all foreground classes in one
    `surface.surface_metrics` call on the label maps.  voxelspacing / connectivity are medpy's arguments of hd95 / asd, passed to
    whichever of the two computes the distances; the defaults are unit spacing and 6-neighbour borders."""
    spacing, connectivity = surface.normalise_spacing(voxelspacing, connectivity)
    conf = confusion_counts(pred, gt, num_classes).cpu().numpy()
    out = np.zeros((conf.shape[0] - 1, 4))
    p_host = g_host = dev = None
    for c in range(1, conf.shape[0]):
        n_p, n_g = int(conf[c].sum()), int(conf[:, c].sum())
        if n_p == 0:
            continue
        out[c - 1, :2] = _dc_jc(n_p, n_g, int(conf[c, c]))
        if n_g == 0:
            continue
        if device_surface:
            if dev is None:
                dev = surface.surface_metrics(pred, gt, classes=(1, conf.shape[0] - 1), voxelspacing=spacing,
                                              connectivity=connectivity).cpu().numpy()
            out[c - 1, 2:] = dev[c - 1, 0], dev[c - 1, 1]
            continue
        if p_host is None:
            p_host = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred)
            g_host = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt)
        out[c - 1, 2:] = _hd95_asd(p_host == c, g_host == c, spacing, connectivity)
    return out


def test_all_case_classes(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                          preproc_fn=None, test_save_path=None, label_key="label", device_surface=False, nms=0, voxelspacing=None,
                          connectivity=1, *, postprocess=None, blend=None):
    """`test_all_case` (code/utils/test_3d_patch.py:251-291) with the all-class evaluator: cases as there; returns the mean (C-1, 4)
    (dice, jaccard, hd95, asd) per foreground class over the cases and writes `../performance.txt` the same way.  device_surface is
    passed to `calculate_metric_perclass`.  The reference defines `nms` for the class-1 map only (:19-26, :266-267); `nms` here is
    its per-class extension: each foreground class of the prediction keeps its largest component
    (`components.largest_component_per_class`, on the device) before the metrics.  The default, 0, leaves the prediction as it is.
    voxelspacing / connectivity go to `calculate_metric_perclass`; a case given as (image, label, spacing) carries its own spacing.
    postprocess (`morphology.PostProcess`): the label map of every case goes through `postprocess.per_class` before `nms`.
    blend goes to `single_case_classes_device`."""
    surface.normalise_spacing(voxelspacing, connectivity)
    morphology.check_postprocess(postprocess)
    def per_case(image, label, spacing):
        pred, score = single_case_classes_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, blend=blend)
        if score.shape[0] != num_classes:
            raise ValueError(f"num_classes = {num_classes}, the model has {score.shape[0]} classes")
        if postprocess is not None:
            pred = postprocess.per_class(pred, num_classes)
        if nms:
            pred = components.largest_component_per_class(pred, num_classes)
        return calculate_metric_perclass(pred, np.asarray(label), num_classes, device_surface=device_surface, voxelspacing=spacing,
                                         connectivity=connectivity)

    def detail(n, m):
        for c, row in enumerate(m, 1):
            print("%02d, class %d,\t%.5f, %.5f, %.5f, %.5f" % ((n, c) + tuple(row)))

    return _mean_over_cases(cases, per_case, np.zeros((num_classes - 1, 4)), label_key, preproc_fn, triples=True,
                            voxelspacing=voxelspacing, detail=detail if metric_detail else None, test_save_path=test_save_path)


def isles_pad(shape, patch_size):
    """The pad of code/train_DyCON_ISLES22.py:355-362 per axis: nothing unless some axis is shorter than the patch; then every axis gets
    max((patch - size) // 2 + 1, 0) on both sides -- the `+ 1` included, so an axis exactly one patch long grows by 2."""
    if all(s >= p for s, p in zip(shape, patch_size)):
        return (0, 0, 0)
    return tuple(max((p - s) // 2 + 1, 0) for s, p in zip(shape, patch_size))


def isles_val_dice(model, volume, label, patch_size):
    """The validation of the ISLES script for one case (code/train_DyCON_ISLES22.py:351-370): pad volume and label by `isles_pad`, one
    forward of the whole volume, argmax over the classes of the model's first output (dycon_argmax_labels; the softmax of :365 does
    not move the argmax) and `metrics.dice(pred == 1, y == 1)`.  volume, label: (w, h, d).  Returns a 0-dim device tensor.  The nets'
    own "divisible by 16" ValueError passes through."""
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("isles_val_dice runs on the MI355X only: move the model to 'cuda'")
    vol = torch.as_tensor(np.asarray(volume) if not torch.is_tensor(volume) else volume).to(dev, torch.float32)[None, None]
    lab = torch.as_tensor(np.asarray(label) if not torch.is_tensor(label) else label).to(dev)[None, None]
    pw, ph, pd = isles_pad(vol.shape[2:], patch_size)
    if pw or ph or pd:
        vol = torch.nn.functional.pad(vol, [pd, pd, ph, ph, pw, pw], mode="constant", value=0)
        lab = torch.nn.functional.pad(lab, [pd, pd, ph, ph, pw, pw], mode="constant", value=0)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            outputs = model(vol)[0]                                               # (1, C, w, h, d)
    finally:
        model.train(was_training)
    C = outputs.shape[1]
    if not 2 <= C <= 8:
        raise ValueError(f"isles_val_dice takes models of 2..8 classes, got {C}")
    lg = outputs.permute(0, 2, 3, 4, 1).contiguous().float()
    pred = torch.empty(lg.shape[1:4], dtype=torch.uint8, device=dev)
    _lib.call("dycon_argmax_labels", lg.data_ptr(), C, pred.numel(), pred.data_ptr(), _stream())
    return metrics.dice(pred == 1, lab[0, 0] == 1)


for _f in (test_single_case_classes, test_all_case_classes):
    _f.__test__ = False        # evaluator names in the reference's style, not pytest cases
