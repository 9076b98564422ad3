"""The one loop over cases and medpy's arithmetic for every evaluator of the package.

The ``test_all_case`` and ``var_all_case_*`` families of ``test_3d_patch``, ``surface_eval``, ``device_eval``, ``ensemble_eval`` and
``eval_classes`` are each a per-case closure and one call to `mean_over_cases` (`mean_dice` for the validation wrappers), with
`dc_jc` and `hd95_asd` for the metrics.  ``test_3d_patch``'s ``_read_case``, ``overlap_counts`` and ``_surface_distances`` are
looked up on that module at call time, so a stand-in placed there reaches every loop.  This module sits below ``test_3d_patch``
(which imports it) so that the modules beside that one need nothing from it but the reference's names.
"""
from __future__ import annotations

import numpy as np
import torch

from . import test_3d_patch as _host


def dc_jc(n_p, n_g, n_i):
    """medpy.metric.binary.dc / jc from |pred|, |gt|, |pred & gt|: dc is 0 for two empty masks, jc raises ZeroDivisionError"""
    dc = 2.0 * n_i / float(n_p + n_g) if n_p + n_g else 0.0
    return dc, float(n_i) / float(n_p + n_g - n_i)


def host_mask(a):
    return np.asarray(a.cpu() if torch.is_tensor(a) else a) != 0


def hd95_asd(pred, gt, voxelspacing=None, connectivity=1):
    """medpy.metric.binary.hd95 / asd of two boolean host arrays"""
    hd1 = _host._surface_distances(pred, gt, voxelspacing, connectivity)
    hd2 = _host._surface_distances(gt, pred, voxelspacing, connectivity)
    return float(np.percentile(np.hstack((hd1, hd2)), 95)), float(hd1.mean())


def read_case(case, label_key, voxelspacing=None):
    """(image, label, spacing) of one case: an h5 path or (image, label) takes the call's `voxelspacing`, (image, label, spacing) its
    own"""
    if not isinstance(case, (str, bytes)) and len(case) == 3:
        return tuple(case)
    image, label = _host._read_case(case, label_key)
    return image, label, voxelspacing


def mean_over_cases(cases, per_case, zero, label_key="label", preproc_fn=None, triples=False, voxelspacing=None, detail=None,
                    test_save_path=None, performance="../performance.txt"):
    """The loop of the test_all_case and var_all_case families (code/utils/test_3d_patch.py:251-291, :28-49): read every case, apply
    `preproc_fn` to its image, add up `per_case(image, label, spacing)` starting from `zero` and divide by the number of cases.  With
    `triples` a case may be (image, label, spacing) and carries its own spacing; every other case takes `voxelspacing`.
    `detail(n, m)` prints the metrics of case n; `test_save_path + performance` receives the mean."""
    total, n = zero, 0
    for case in cases:
        if triples:
            image, label, spacing = read_case(case, label_key, voxelspacing)
        else:
            (image, label), spacing = _host._read_case(case, label_key), voxelspacing
        if preproc_fn is not None:
            image = preproc_fn(image)
        m = per_case(image, label, spacing)
        if detail is not None:
            detail(n, m)
        total = total + m
        n += 1
    avg = total / max(n, 1)
    if test_save_path is not None:
        with open(test_save_path + performance, "w") as f:
            f.writelines("average metric is {} \n".format(avg))
    return avg


def print_metrics(n, m):
    print("%02d,\t%.5f, %.5f, %.5f, %.5f" % ((n,) + tuple(m)))


def binary_case(pred, label, nms, largest, metric):
    """`nms`, the empty-prediction rule (:268-271) and the four metrics of one predicted label map, a numpy array or a CUDA tensor
    (then one flag is read back)"""
    if nms:
        pred = largest(pred)
    if not bool(pred.any()):
        return np.zeros(4)
    return np.asarray(metric(pred, np.asarray(label)))


def mean_dice(cases, single_case, label_key="label", transpose=None):
    """validation during training (the var_all_case_* family, :28-49, :52-74, :120-141, :188-209): Dice of the prediction
    `single_case(image)[0]` of every case, 0 for an empty one, over the number of cases.  transpose: axis permutation applied to image
    AND label before the sliding window (BraTS19: (2, 1, 0), :64-65 -- the orientation the training patches have after
    dataloaders.brats19.SagittalToAxial)."""
    def dice(image, label, spacing):
        if transpose is not None:
            image, label = np.transpose(np.asarray(image), transpose), np.transpose(np.asarray(label), transpose)
        pred, _ = single_case(image)
        return dc_jc(*_host.overlap_counts(pred, np.asarray(label)))[0] if pred.sum() != 0 else 0.0

    return mean_over_cases(cases, dice, 0.0, label_key)
