"""The per-case evaluator of ``utils/test_3d_patch.py`` with the opt-in device surface distances (utils/surface.py).

``utils/test_3d_patch.py`` is left as it is and nothing in it is rebound: its ``calculate_metric_percase`` and ``test_all_case`` family
stay the host-scipy functions they were.  The functions here carry the same names and arguments plus ``device_surface=False``.  With
the flag off each calls the function of ``test_3d_patch.py`` with the arguments it was given; with the flag on, HD95 and ASD of a case
come from one ``surface.surface_metrics`` call (unit voxel spacing, csrc/surface.hip), while Dice, Jaccard and the conventions for
empty masks are decided from the same device counts either way.

    calculate_metric_percase(pred, gt, device_surface=False)                    code/utils/test_3d_patch.py:496-508
    test_all_case(model, cases, num_classes, ..., device_surface=False)         :251-291
    test_all_case_BraTS19 / _Pancreas / _ISLES22(..., device_surface=False)
"""
from __future__ import annotations

import numpy as np

from . import surface
from . import test_3d_patch as _host


def calculate_metric_percase(pred, gt, device_surface=False):
    """(dice, jaccard, hd95, asd) of one case, medpy.metric.binary semantics (code/utils/test_3d_patch.py:496-508)."""
    if not device_surface:
        return _host.calculate_metric_percase(pred, gt)
    n_p, n_g, n_i = _host.overlap_counts(pred, gt)
    dice = 2.0 * n_i / float(n_p + n_g) if n_p + n_g else 0.0
    jc = float(n_i) / float(n_p + n_g - n_i)               # ZeroDivisionError for two empty masks, as medpy
    if n_g == 0:
        return dice, jc, 0.0, 0.0
    if n_p == 0:                                           # what the host path's surface distances raise
        raise RuntimeError("The first supplied array does not contain any binary object.")
    m = surface.surface_metrics(pred, gt)[0].tolist()
    return dice, jc, m[0], m[1]


def test_all_case(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                  nms=0, preproc_fn=None, test_save_path=None, label_key="label", device_surface=False):
    """`test_3d_patch.test_all_case`; with device_surface=True the same loop (:251-291) with the device surface distances per case."""
    if not device_surface:
        return _host.test_all_case(model, cases, num_classes, patch_size, stride_xy, stride_z, batch_size=batch_size,
                                   metric_detail=metric_detail, nms=nms, preproc_fn=preproc_fn, test_save_path=test_save_path,
                                   label_key=label_key)
    total = np.zeros(4)
    n = 0
    for case in cases:
        image, label = _host._read_case(case, label_key)
        if preproc_fn is not None:
            image = preproc_fn(image)
        pred, _ = _host.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, batch_size=batch_size)
        if nms:
            pred = _host.getLargestCC(pred)
        m = (0.0, 0.0, 0.0, 0.0) if pred.sum() == 0 else calculate_metric_percase(pred, np.asarray(label), device_surface=True)
        if metric_detail:
            print("%02d,\t%.5f, %.5f, %.5f, %.5f" % ((n,) + tuple(m)))
        total += np.asarray(m)
        n += 1
    avg = total / max(n, 1)
    if test_save_path is not None:
        with open(test_save_path + "../performance.txt", "w") as f:
            f.writelines("average metric is {} \n".format(avg))
    return avg


def test_all_case_BraTS19(model, image_list, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, save_result=True,
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False):
    if not device_surface:
        return _host.test_all_case_BraTS19(model, image_list, num_classes, patch_size, stride_xy, stride_z, save_result,
                                           test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, device_surface=True)


def test_all_case_Pancreas(model, image_list, num_classes, device=None, patch_size=(96, 96, 64), stride_xy=16, stride_z=4,
                           save_result=True, test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False):
    if not device_surface:
        return _host.test_all_case_Pancreas(model, image_list, num_classes, device, patch_size, stride_xy, stride_z, save_result,
                                            test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, device_surface=True)


def test_all_case_ISLES22(model, image_list, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, save_result=True,
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False):
    if not device_surface:
        return _host.test_all_case_ISLES22(model, image_list, num_classes, patch_size, stride_xy, stride_z, save_result,
                                           test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, label_key="mask", device_surface=True)


for _f in (test_all_case, test_all_case_BraTS19, test_all_case_Pancreas, test_all_case_ISLES22):
    _f.__test__ = False        # reference names, not pytest cases
