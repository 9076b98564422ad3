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
is not the mean of the models' probability maps.  The windows go through the driver of ``utils/sliding_window.py``: per chunk of
`batch_size` windows one `dycon_sw_gather` launch, the forwards, one `dycon_sw_accumulate_ens` launch; `dycon_sw_finalize` at the
end.  Score and count maps never leave the device.  The models run one after the other on the current stream.  An ensemble of a
model with itself gives `single_case_device`'s bits at the same `batch_size`: one kernel body serves both (csrc/sw_accumulate.h).
The case loops are `case_loop.mean_over_cases` and `case_loop.mean_dice`.

`single_case_ensemble_device` and `single_case_plus_device` take ``blend=`` (`sliding_window.Blend`: Gaussian importance weighting,
mirror test-time augmentation).  The functions under the reference's names keep the reference's parameter lists and blend as the
reference does.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import case_loop, device_eval, sliding_window
from . import test_3d_patch as _host
from .case_loop import mean_dice as _mean_dice
from .sliding_window import MAX_MODELS, _center_pads, _logits_of  # noqa: F401  (_center_pads: gather_windows_host and the tests)


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


def single_case_ensemble_device(models, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None):
    """(label uint8 (w, h, d), prob float32 (w, h, d)) as CUDA tensors: the sliding window of `test_single_case_plus` over 2..4
    models with one class count (2..8; otherwise ValueError).  prob: class 1 of the softmax of the models' mean logits, averaged over
    the windows covering a voxel; label = prob > 0.5.  image: (w, h, d) numpy array or tensor.  batch_size: 1..64 windows per chunk.
    blend: None or a `sliding_window.Blend`."""
    models = _check_models(models)
    if not 1 <= int(batch_size) <= 64:
        raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
    dev = torch.device(device) if device is not None else next(models[0].parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the models to 'cuda'")
    seen = []                                                   # the class count of the first logits

    def forward_of(model):
        def forward(patches):
            logits = _logits_of(model(patches))
            if tuple(logits.shape[2:]) != tuple(patches.shape[2:]) or logits.shape[0] != patches.shape[0]:
                raise ValueError(f"a model's logits have shape {tuple(logits.shape)} for windows {tuple(patches.shape)}")
            C = int(logits.shape[1])
            if not seen:
                if not 2 <= C <= 8:
                    raise ValueError(f"the ensemble scores class 1 of the softmax of 2..8 classes (:463-466), the logits have {C}")
                seen.append(C)
            elif C != seen[0]:
                raise ValueError(f"the models of an ensemble share one class count, got logits with {seen[0]} and {C}")
            return logits
        return forward

    return sliding_window._sliding_window(models, [forward_of(m) for m in models], image, stride_xy, stride_z, patch_size, batch_size,
                                          dev, blend=blend)


def single_case_plus_device(model_l, model_r, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None):
    """`single_case_ensemble_device` of the reference's pair (model_l, model_r)"""
    return single_case_ensemble_device((model_l, model_r), image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device,
                                       blend=blend)


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
    def device_case(image):
        return single_case_plus_device(model_l, model_r, image, stride_xy, stride_z, patch_size, batch_size=batch_size)

    def host_case(image, label, spacing):
        pred, _ = test_single_case_plus(model_l, model_r, image, stride_xy, stride_z, patch_size, num_classes=num_classes,
                                        batch_size=batch_size)
        return case_loop.binary_case(pred, label, nms, _host.getLargestCC, _host.calculate_metric_percase)

    per_case = device_eval._device_case(device_case, nms) if device_resident else host_case

    return case_loop.mean_over_cases(image_list, per_case, np.zeros(4), preproc_fn=preproc_fn, triples=device_resident,
                                     detail=case_loop.print_metrics if metric_detail else None, test_save_path=test_save_path,
                                     performance="/performance.txt")


def _la_cases(root_dir, folder):
    with open(os.path.join(root_dir, "test.list"), "r") as f:
        return [root_dir + "/" + folder + "/" + item.replace("\n", "") + "/mri_norm2.h5" for item in f.readlines()]


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
    p, g = case_loop.host_mask(pred), case_loop.host_mask(gt)
    # ZeroDivisionError for two empty masks, as medpy
    return case_loop.dc_jc(int(np.count_nonzero(p)), int(np.count_nonzero(g)), int(np.count_nonzero(p & g))) + case_loop.hd95_asd(p, g)


def normalize_image(data: np.ndarray):
    """:14-17: (data - min) / (max - min)"""
    data_min = np.min(data)
    return (data - data_min) / (np.max(data) - data_min)


REFERENCE_NAMES = ("test_single_case_plus", "test_all_case_plus", "var_all_case_LA", "var_all_case_LA_plus",
                   "calculate_metric_percase1", "normalize_image")

for _f in (test_single_case_plus, test_all_case_plus):
    _f.__test__ = False        # reference names, not pytest cases
