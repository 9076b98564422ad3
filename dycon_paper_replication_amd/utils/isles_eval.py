"""The test protocol of the reference's ISLES22 script (code/test_ISLES22.py:78-180) with the prediction kept on the device, and the
lesion-wise scores of utils/lesions.py next to it.

The script does not go through ``test_all_case_ISLES22``: it runs the whole volume through the model once, thresholds the class-1
softmax at 0.5 (:87-91), and scores each case by rules of its own for empty masks (:98-121), which differ from the (0, 0, 0, 0) of
``test_3d_patch.test_all_case``.  Next to Dice, HD95 and ASD it reports sensitivity and specificity (:154-164), each metric as mean
and standard deviation over the cases (:177-179).

    isles_case_metrics(pred, gt, device_surface=True, voxelspacing=None)   -> dict dice, hd95, asd, sensitivity, specificity
    evaluate_isles22(model, cases, patch_size=None, ..., lesion=True)      -> {"per_case": {...}, "summary": {name: (mean, std)}}

Per case the host sends the image and the ground truth and reads back the voxel counts, one row of surface metrics and, with
`lesion=True`, the eight lesion counts; the masks stay where they are.
"""
from __future__ import annotations

import numpy as np

from . import lesions, morphology, sliding_window, surface_eval
from . import test_3d_patch as _host

CASE_FIELDS = ("dice", "hd95", "asd", "sensitivity", "specificity")
LESION_FIELDS = ("lesion_f1", "lesion_count_diff", "abs_volume_diff")


def isles_case_metrics(pred, gt, device_surface=True, voxelspacing=None):
    """One case of code/test_ISLES22.py:98-164.  pred, gt: (H, W, D) numpy arrays or CUDA tensors, foreground = non-zero.

    both masks empty        dice 1, hd95 0, asd 0, sensitivity 1, specificity 1
    exactly one empty       dice 0, hd95 = asd = ||(H, W, D)||_2 (in voxels, whatever the spacing), sensitivity 0, specificity 0 when
                            the ground truth is the empty one (:117 can only give 0 there) and 1 when the prediction is
    otherwise               dice, hd95, asd of `surface_eval.calculate_metric_percase` (HD95 and ASD on the device with
                            device_surface=True, in the units of `voxelspacing`), sensitivity = tp / (tp + fn + 1e-10), specificity =
                            tn / (tn + fp + 1e-10) from the voxel confusion counts
    """
    shape = tuple(gt.shape)
    if len(shape) != 3 or tuple(pred.shape) != shape:
        raise ValueError(f"expected one (H, W, D) prediction and ground truth, got {tuple(pred.shape)} and {shape}")
    n_p, n_g, n_i = _host.overlap_counts(pred, gt)                   # the one set of counts read back; the masks stay
    if n_p == 0 and n_g == 0:
        return dict(dice=1.0, hd95=0.0, asd=0.0, sensitivity=1.0, specificity=1.0)
    if n_p == 0 or n_g == 0:
        far = float(np.linalg.norm(shape))
        return dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=0.0 if n_g == 0 else 1.0)
    dice, _, hd95, asd = surface_eval.calculate_metric_percase(pred, gt, device_surface=device_surface, voxelspacing=voxelspacing)
    tp, fn, fp = n_i, n_g - n_i, n_p - n_i
    tn = int(np.prod(shape)) - n_p - n_g + n_i
    return dict(dice=float(dice), hd95=float(hd95), asd=float(asd), sensitivity=tp / (tp + fn + 1e-10),
                specificity=tn / (tn + fp + 1e-10))


def evaluate_isles22(model, cases, patch_size=None, stride_xy=16, stride_z=4, batch_size=4, lesion=True, connectivity=3,
                     min_voxels=1, label_key="mask", *, postprocess=None, blend=None):
    """The loop of code/test_ISLES22.py:78-180 over `cases` (h5 paths, (image, label) or (image, label, spacing), read by
    `surface_eval.read_case`; a case's spacing goes into its HD95, ASD and abs_volume_diff).

    patch_size=None is the script's forward: the whole volume as one window (the nets need every axis divisible by 16 and say so);
    a patch size runs the sliding window with the given strides.  Either way the prediction is the class-1 probability > 0.5
    (:88-91) as a device tensor.  With lesion=True every case also gets lesion_f1, lesion_count_diff and abs_volume_diff
    (utils/lesions.py; `connectivity`, `min_voxels`).  blend (`sliding_window.Blend`) blends overlapping windows, so it is valid on the
    sliding-window route only: with patch_size=None a blend raises ValueError.  postprocess (`morphology.PostProcess`) is applied to
    the prediction on the device before the voxel metrics and the lesion scores alike.

    Returns {"per_case": {name: float64 array over the cases}, "summary": {name: (np.mean, np.std)}} (:177-179)."""
    if patch_size is None and blend is not None:
        raise ValueError("blend needs the sliding window: the whole-volume forward (patch_size=None) has one window and nothing to blend")
    morphology.check_postprocess(postprocess)
    names = CASE_FIELDS + (LESION_FIELDS if lesion else ())
    rows = {name: [] for name in names}
    for case in cases:
        image, label, spacing = surface_eval.read_case(case, label_key)
        window = tuple(image.shape) if patch_size is None else tuple(patch_size)
        pred, _ = sliding_window.single_case_device(model, image, stride_xy, stride_z, window, batch_size=batch_size, blend=blend)
        if postprocess is not None:
            pred = postprocess(pred)
        label = np.asarray(label)
        m = isles_case_metrics(pred, label, device_surface=True, voxelspacing=spacing)
        if lesion:
            scores = lesions.lesion_metrics(pred, label, voxelspacing=spacing, connectivity=connectivity, min_voxels=min_voxels)
            m.update((name, float(scores[name])) for name in LESION_FIELDS)
        for name in names:
            rows[name].append(m[name])
    per_case = {name: np.asarray(v, dtype=np.float64) for name, v in rows.items()}
    return {"per_case": per_case, "summary": {name: (np.mean(v), np.std(v)) for name, v in per_case.items()}}
