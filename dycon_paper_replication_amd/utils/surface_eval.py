"""The per-case evaluator of ``utils/test_3d_patch.py`` with the opt-in device surface distances (utils/surface.py).

``utils/test_3d_patch.py`` is left as it is and nothing in it is rebound: its ``calculate_metric_percase`` and ``test_all_case`` family
stay the host-scipy functions they were.  The functions here carry the same names and arguments plus ``device_surface=False``,
``voxelspacing=None`` and ``connectivity=1`` (medpy's arguments of hd95 / asd).  With all three at their defaults each calls the
function of ``test_3d_patch.py`` with the arguments it was given.  With the flag on, HD95 and ASD of a case come from one
``surface.surface_metrics`` call (csrc/surface.hip for unit spacing and 6-neighbour borders, csrc/surface_spacing.hip otherwise), while
Dice, Jaccard and the conventions for empty masks are decided from the same device counts either way.  With the flag off and a
spacing or connectivity given, the host branch passes them to ``test_3d_patch._surface_distances``: millimetres on the host.

    calculate_metric_percase(pred, gt, device_surface=False, voxelspacing=None, connectivity=1)      code/utils/test_3d_patch.py:496-508
    test_all_case(model, cases, num_classes, ..., device_surface=False, voxelspacing=None, connectivity=1)               :251-291
    test_all_case_BraTS19 / _Pancreas / _ISLES22(..., device_surface=False, voxelspacing=None, connectivity=1)

In the ``test_all_case`` family a case may be ``(image, label, spacing)``: its spacing replaces the call's ``voxelspacing`` for that
case.  Two-element cases and h5 paths are read as before.
"""
from __future__ import annotations

import numpy as np
import torch

from . import surface
from . import test_3d_patch as _host


def read_case(case, label_key, voxelspacing=None):
    """(image, label, spacing) of one case: an h5 path or (image, label) takes the call's `voxelspacing`, (image, label, spacing) its
    own"""
    if not isinstance(case, (str, bytes)) and len(case) == 3:
        return tuple(case)
    image, label = _host._read_case(case, label_key)
    return image, label, voxelspacing


def calculate_metric_percase(pred, gt, device_surface=False, voxelspacing=None, connectivity=1):
    """(dice, jaccard, hd95, asd) of one case, medpy.metric.binary semantics (code/utils/test_3d_patch.py:496-508)."""
    spacing, connectivity = surface.normalise_spacing(voxelspacing, connectivity)
    if not device_surface and spacing is None and connectivity == 1:
        return _host.calculate_metric_percase(pred, gt)
    n_p, n_g, n_i = _host.overlap_counts(pred, gt)
    dice = 2.0 * n_i / float(n_p + n_g) if n_p + n_g else 0.0
    jc = float(n_i) / float(n_p + n_g - n_i)               # ZeroDivisionError for two empty masks, as medpy
    if n_g == 0:
        return dice, jc, 0.0, 0.0
    if n_p == 0:                                           # what the host path's surface distances raise
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if device_surface:
        m = surface.surface_metrics(pred, gt, voxelspacing=spacing, connectivity=connectivity)[0].tolist()
        return dice, jc, m[0], m[1]
    p = np.asarray(pred.cpu() if torch.is_tensor(pred) else pred) != 0
    g = np.asarray(gt.cpu() if torch.is_tensor(gt) else gt) != 0
    hd1, hd2 = _host._surface_distances(p, g, spacing, connectivity), _host._surface_distances(g, p, spacing, connectivity)
    return dice, jc, float(np.percentile(np.hstack((hd1, hd2)), 95)), float(hd1.mean())


def _cases_carry_spacing(cases):
    return isinstance(cases, (list, tuple)) and any(not isinstance(c, (str, bytes)) and len(c) == 3 for c in cases)


def _own_loop(device_surface, voxelspacing, connectivity, cases):
    return device_surface or voxelspacing is not None or connectivity != 1 or _cases_carry_spacing(cases)


def test_all_case(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                  nms=0, preproc_fn=None, test_save_path=None, label_key="label", device_surface=False, voxelspacing=None,
                  connectivity=1):
    """`test_3d_patch.test_all_case`; with device_surface=True, a spacing, a connectivity or a list holding (image, label, spacing)
    cases the same loop (:251-291) with `calculate_metric_percase` of this module per case."""
    surface.normalise_spacing(voxelspacing, connectivity)
    if not _own_loop(device_surface, voxelspacing, connectivity, cases):
        return _host.test_all_case(model, cases, num_classes, patch_size, stride_xy, stride_z, batch_size=batch_size,
                                   metric_detail=metric_detail, nms=nms, preproc_fn=preproc_fn, test_save_path=test_save_path,
                                   label_key=label_key)
    total = np.zeros(4)
    n = 0
    for case in cases:
        image, label, spacing = read_case(case, label_key, voxelspacing)
        if preproc_fn is not None:
            image = preproc_fn(image)
        pred, _ = _host.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, batch_size=batch_size)
        if nms:
            pred = _host.getLargestCC(pred)
        if pred.sum() == 0:
            m = (0.0, 0.0, 0.0, 0.0)
        else:
            m = calculate_metric_percase(pred, np.asarray(label), device_surface=device_surface, voxelspacing=spacing,
                                         connectivity=connectivity)
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
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False, voxelspacing=None,
                          connectivity=1):
    if not _own_loop(device_surface, voxelspacing, connectivity, image_list):
        return _host.test_all_case_BraTS19(model, image_list, num_classes, patch_size, stride_xy, stride_z, save_result,
                                           test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, device_surface=device_surface,
                         voxelspacing=voxelspacing, connectivity=connectivity)


def test_all_case_Pancreas(model, image_list, num_classes, device=None, patch_size=(96, 96, 64), stride_xy=16, stride_z=4,
                           save_result=True, test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False,
                           voxelspacing=None, connectivity=1):
    if not _own_loop(device_surface, voxelspacing, connectivity, image_list):
        return _host.test_all_case_Pancreas(model, image_list, num_classes, device, patch_size, stride_xy, stride_z, save_result,
                                            test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, device_surface=device_surface,
                         voxelspacing=voxelspacing, connectivity=connectivity)


def test_all_case_ISLES22(model, image_list, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, save_result=True,
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0, device_surface=False, voxelspacing=None,
                          connectivity=1):
    if not _own_loop(device_surface, voxelspacing, connectivity, image_list):
        return _host.test_all_case_ISLES22(model, image_list, num_classes, patch_size, stride_xy, stride_z, save_result,
                                           test_save_path, preproc_fn, metric_detail, nms)
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, label_key="mask", device_surface=device_surface,
                         voxelspacing=voxelspacing, connectivity=connectivity)


for _f in (test_all_case, test_all_case_BraTS19, test_all_case_Pancreas, test_all_case_ISLES22):
    _f.__test__ = False        # reference names, not pytest cases
