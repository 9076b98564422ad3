"""Model-ensemble sliding-window evaluation (code/utils/test_3d_patch.py: the `_plus` family and its small neighbours).

    single_case_ensemble_device(models, image, ...)      2..4 models -> (label uint8, prob float32) CUDA tensors
    single_case_plus_device(model_l, model_r, image, ...)     the two-model form
    test_single_case_plus(model_l, model_r, image, ...)       :415-476   numpy (label_map int64, score_map (num_classes, w, h, d))
    test_all_case_plus(model_l, model_r, image_list, ...)     :375-413   mean (dice, jaccard, hd95, asd)
    var_all_case_LA(model, root_dir, ...)                     :28-49     mean Dice over `<root_dir>/test.list`
    var_all_case_LA_plus(model_l, model_r, num_classes, ...)  :354-373   the same for a pair of models
    calculate_metric_percase1(pred, gt)                       :488-494   the four metrics without the empty-ground-truth rule
    normalize_image(data)                                     :14-17

Every window goes through each model in turn; the models' logits are averaged BEFORE the softmax ((y1_l + y1_r) / 2, :460-463), which
is not the mean of the models' probability maps.  Per chunk of `batch_size` windows: one `dycon_sw_gather` launch (the windows
straight from the unpadded volume, the origins of the whole case uploaded once), the forwards, one `dycon_sw_accumulate_ens` launch
(csrc/ensemble.hip); `dycon_sw_finalize` at the end.  Score and count maps never leave the device.  The models run one after the
other on the current stream.  ``utils.sliding_window.single_case_device`` and ``utils.test_3d_patch.test_single_case`` are not
touched; an ensemble of a model with itself gives `single_case_device`'s bits at the same `batch_size`.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from .. import _lib
from . import components, surface_eval
from . import test_3d_patch as _host
from .test_3d_patch import _windows

MAX_MODELS = 4


def _center_pads(shape, patch_size):
    """:418-437: (front, back) zero pad of every axis shorter than the window"""
    pads = []
    for size, p in zip(shape, patch_size):
        pad = max(p - size, 0)
        pads.append((pad // 2, pad - pad // 2))
    return pads


def gather_windows_host(volume, origins, patch_size):
    """What `dycon_sw_gather` writes, in numpy: (n, 1, p0, p1, p2) float32 windows of the UNPADDED (w, h, d) `volume` at `origins`
    (n x 3, coordinates of the centre-padded volume); a source index outside the stored volume reads as 0."""
    vol = np.asarray(volume, dtype=np.float32)
    org = np.asarray(origins, dtype=np.int64).reshape(-1, 3)
    p = tuple(int(v) for v in patch_size)
    lo = [a for a, _ in _center_pads(vol.shape, p)]
    out = np.zeros((len(org), 1) + p, dtype=np.float32)
    idx = [np.arange(n) for n in p]
    for n, o in enumerate(org):
        s = [o[a] - lo[a] + idx[a] for a in range(3)]
        ok = [(s[a] >= 0) & (s[a] < vol.shape[a]) for a in range(3)]
        c = [np.clip(s[a], 0, vol.shape[a] - 1) for a in range(3)]
        inside = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
        out[n, 0] = np.where(inside, vol[c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]], 0)
    return out


def _logits_of(out):
    """a 3-tuple (this package's nets: tanh map, logits, features) gives element 1; a 2-tuple gives element 0, as the reference
    unpacks ``y1_l, _ = model_l(x)`` (:460)"""
    if isinstance(out, (tuple, list)):
        if len(out) == 3:
            return out[1]
        if len(out) == 2:
            return out[0]
        raise ValueError(f"a model returns (tanh, logits, features) or (logits, features), got {len(out)} outputs")
    return out


def _check_models(models):
    models = list(models)
    if not 2 <= len(models) <= MAX_MODELS:
        raise ValueError(f"an ensemble takes 2..{MAX_MODELS} models, got {len(models)}")
    declared = [getattr(m, "n_classes", None) for m in models]
    known = [c for c in declared if c is not None]
    if any(c != known[0] for c in known):
        raise ValueError(f"the models of an ensemble share one class count, got {declared}")
    if known and not 2 <= known[0] <= 8:
        raise ValueError(f"the ensemble scores class 1 of the softmax of 2..8 classes (:463-466), the models have {known[0]}")
    return models


def single_case_ensemble_device(models, image, stride_xy, stride_z, patch_size, batch_size=4, device=None):
    """(label uint8 (w, h, d), prob float32 (w, h, d)) as CUDA tensors: the sliding window of `test_single_case_plus` over 2..4
    models with one class count (2..8; otherwise ValueError).  prob: class 1 of the softmax of the models' mean logits, averaged over
    the windows covering a voxel; label = prob > 0.5.  image: (w, h, d) numpy array or tensor.  batch_size: 1..64 windows per chunk."""
    models = _check_models(models)
    if not 1 <= int(batch_size) <= 64:
        raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
    dev = torch.device(device) if device is not None else next(models[0].parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the models to 'cuda'")
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))).to(dtype=torch.float32)
    w, h, d = img.shape
    p0, p1, p2 = (int(v) for v in patch_size)
    pads = _center_pads((w, h, d), (p0, p1, p2))
    add_pad = any(lo or hi for lo, hi in pads)
    vol = img.to(dev).contiguous()                              # the UNPADDED volume: the pad lives in the gather's index arithmetic
    ww, hh, dd = (n + lo + hi for n, (lo, hi) in zip((w, h, d), pads))
    wins = _windows((ww, hh, dd), (p0, p1, p2), stride_xy, stride_z)
    origins = torch.tensor(wins, dtype=torch.int32).to(dev)     # every window of the case, uploaded once
    score = torch.zeros((ww, hh, dd), dtype=torch.float32, device=dev)
    cnt = torch.zeros_like(score)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    saved = [(m, m.training, getattr(m, "weights_static", None)) for m in models]
    C = None
    try:
        for m, _, was_static in saved:
            m.eval()
            if was_static is not None:
                m.weights_static = True      # no parameter changes between the windows: pack the weights once (networks/_base.py)
        with torch.no_grad():
            for i in range(0, len(wins), batch_size):
                nb = min(batch_size, len(wins) - i)
                patches = torch.empty((nb, 1, p0, p1, p2), dtype=torch.float32, device=dev)
                _lib.call("dycon_sw_gather", vol.data_ptr(), w, h, d, origins.data_ptr(), len(wins), i, nb, p0, p1, p2,
                          patches.data_ptr(), stream())
                lgs = []
                for m in models:
                    logits = _logits_of(m(patches))                               # (nb, C, p0, p1, p2), channels-last-3D view
                    if tuple(logits.shape[2:]) != (p0, p1, p2) or logits.shape[0] != nb:
                        raise ValueError(f"a model's logits have shape {tuple(logits.shape)} for windows {tuple(patches.shape)}")
                    if C is None:
                        C = int(logits.shape[1])
                        if not 2 <= C <= 8:
                            raise ValueError(f"the ensemble scores class 1 of the softmax of 2..8 classes (:463-466), the logits have {C}")
                    elif int(logits.shape[1]) != C:
                        raise ValueError(f"the models of an ensemble share one class count, got logits with {C} and {logits.shape[1]}")
                    lgs.append(logits.permute(0, 2, 3, 4, 1).contiguous().float())   # NDHWC (free for the HIP nets' outputs)
                ptrs = [t.data_ptr() for t in lgs] + [None] * (MAX_MODELS - len(lgs))
                _lib.call("dycon_sw_accumulate_ens", *ptrs, len(lgs), C, nb, p0, p1, p2, origins.data_ptr() + 12 * i,
                          score.data_ptr(), cnt.data_ptr(), ww, hh, dd, stream())
    finally:
        for m, was_training, was_static in saved:
            m.train(was_training)
            if was_static is not None:
                m.weights_static = was_static
    label = torch.empty((ww, hh, dd), dtype=torch.uint8, device=dev)
    prob = torch.empty_like(score)
    _lib.call("dycon_sw_finalize", score.data_ptr(), cnt.data_ptr(), score.numel(), 0.5, label.data_ptr(), prob.data_ptr(), stream())
    if add_pad:
        sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, (w, h, d)))
        label, prob = label[sl], prob[sl]
    return label, prob


def single_case_plus_device(model_l, model_r, image, stride_xy, stride_z, patch_size, batch_size=4, device=None):
    """`single_case_ensemble_device` of the reference's pair (model_l, model_r)"""
    return single_case_ensemble_device((model_l, model_r), image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device)


def test_single_case_plus(model_l, model_r, image, stride_xy, stride_z, patch_size, device=None, num_classes=1, batch_size=4):
    """:415-476.  Returns (label_map int64 (w, h, d), score_map float32 (num_classes, w, h, d)) as numpy; the class-1 probability
    fills every channel of score_map (the reference's broadcast, :467-468), label_map = score > 0.5 (:472).  `device` keeps the
    reference's position; its own callers leave it out (:365, :387), so it defaults to the models' device."""
    label, prob = single_case_plus_device(model_l, model_r, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device)
    label_map = label.cpu().numpy().astype(np.int64)
    score_map = np.broadcast_to(prob.cpu().numpy()[None], (num_classes,) + label_map.shape).copy()
    return label_map, score_map


def test_all_case_plus(model_l, model_r, image_list, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4, save_result=True,
                       test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_resident=False, batch_size=4):
    """:375-413: the mean (dice, jaccard, hd95, asd) over the cases.  image_list: (image, label) arrays or h5 paths with 'image' /
    'label' (needs h5py); with device_resident=True also (image, label, spacing).  An empty prediction scores (0, 0, 0, 0);
    test_save_path receives `/performance.txt` (:411).  save_result is accepted and ignored (no NIfTI writer here).
    device_resident=True keeps the label map on the device: `components.largest_component` for nms and the device surface
    distances, as `utils.device_eval.test_all_case` does for one model."""
    total = np.zeros(4)
    n = 0
    for case in image_list:
        if device_resident:
            image, label, spacing = surface_eval.read_case(case, "label")
        else:
            image, label = _host._read_case(case, "label")
        if preproc_fn is not None:
            image = preproc_fn(image)
        if device_resident:
            pred, _ = single_case_plus_device(model_l, model_r, image, stride_xy, stride_z, patch_size, batch_size=batch_size)
            if nms:
                pred = components.largest_component(pred)
            if not bool(pred.any()):                           # one flag read back; the empty-prediction convention of :391-392
                m = (0.0, 0.0, 0.0, 0.0)
            else:
                m = surface_eval.calculate_metric_percase(pred, np.asarray(label), device_surface=True, voxelspacing=spacing)
        else:
            pred, _ = test_single_case_plus(model_l, model_r, image, stride_xy, stride_z, patch_size, num_classes=num_classes,
                                            batch_size=batch_size)
            if nms:
                pred = _host.getLargestCC(pred)
            m = (0.0, 0.0, 0.0, 0.0) if pred.sum() == 0 else _host.calculate_metric_percase(pred, np.asarray(label))
        if metric_detail:
            print("%02d,\t%.5f, %.5f, %.5f, %.5f" % ((n,) + tuple(m)))
        total += np.asarray(m)
        n += 1
    avg = total / max(n, 1)
    if test_save_path is not None:
        with open(test_save_path + "/performance.txt", "w") as f:
            f.writelines("average metric is {} \n".format(avg))
    return avg


def _la_cases(root_dir, folder):
    with open(os.path.join(root_dir, "test.list"), "r") as f:
        return [root_dir + "/" + folder + "/" + item.replace("\n", "") + "/mri_norm2.h5" for item in f.readlines()]


def _mean_dice(cases, single_case):
    """:34-49: Dice of every case (0 for an empty prediction) over the number of cases"""
    total = 0.0
    for path in cases:
        image, label = _host._read_case(path, "label")       # h5py is imported there, when a path is read
        pred, _ = single_case(image)
        if pred.sum() != 0:
            n_p, n_g, n_i = _host.overlap_counts(pred, np.asarray(label))
            total += 2.0 * n_i / float(n_p + n_g)
    return total / len(cases)


def var_all_case_LA(model, root_dir, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4):
    """:28-49: mean Dice over `<root_dir>/test.list`, cases at `<root_dir>/LA_data/<case>/mri_norm2.h5`"""
    return _mean_dice(_la_cases(root_dir, "LA_data"),
                      lambda image: _host.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes))


def var_all_case_LA_plus(model_l, model_r, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4, root_dir="../data/LA"):
    """:354-373: the same for the pair; the reference's fixed `../data/LA/test.list` and `2018LA_Seg_Training Set/<case>/mri_norm2.h5`
    under `root_dir`"""
    return _mean_dice(_la_cases(root_dir, "2018LA_Seg_Training Set"),
                      lambda image: test_single_case_plus(model_l, model_r, image, stride_xy, stride_z, patch_size, num_classes=num_classes))


def calculate_metric_percase1(pred, gt):
    """:488-494: (dice, jaccard, hd95, asd), medpy.metric.binary semantics, WITHOUT the empty-ground-truth rule of
    calculate_metric_percase: an empty mask on either side raises, as medpy's surface distances do.  A per-case diagnostic on the
    host (numpy arrays or tensors of any device)."""
    p = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred) != 0
    g = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt) != 0
    n_p, n_g, n_i = int(np.count_nonzero(p)), int(np.count_nonzero(g)), int(np.count_nonzero(p & g))
    dice = 2.0 * n_i / float(n_p + n_g) if n_p + n_g else 0.0
    jc = float(n_i) / float(n_p + n_g - n_i)               # ZeroDivisionError for two empty masks, as medpy
    hd1, hd2 = _host._surface_distances(p, g), _host._surface_distances(g, p)
    return dice, jc, float(np.percentile(np.hstack((hd1, hd2)), 95)), float(hd1.mean())


def normalize_image(data: np.ndarray):
    """:14-17: (data - min) / (max - min)"""
    data_min = np.min(data)
    return (data - data_min) / (np.max(data) - data_min)


REFERENCE_NAMES = ("test_single_case_plus", "test_all_case_plus", "var_all_case_LA", "var_all_case_LA_plus",
                   "calculate_metric_percase1", "normalize_image")

for _f in (test_single_case_plus, test_all_case_plus):
    _f.__test__ = False        # reference names, not pytest cases
