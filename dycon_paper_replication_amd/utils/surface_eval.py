"""The per-case evaluator of ``utils/test_3d_patch.py`` with the opt-in device surface distances (utils/surface.py).

``calculate_metric_percase`` and the ``test_all_case`` family of ``utils/test_3d_patch.py`` are the host-scipy functions; the case
loop and medpy's arithmetic beside them are ``utils/case_loop.py``.  The functions here carry the same names and arguments plus
``device_surface=False``, ``voxelspacing=None`` and ``connectivity=1`` (medpy's arguments of hd95 / asd).  With all three at their
defaults each calls the function of ``test_3d_patch.py`` with the arguments it was given.  With the flag on, HD95 and ASD of a case come from one
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

from . import case_loop, components, morphology, sliding_window, surface
from . import test_3d_patch as _host
from .case_loop import read_case  # noqa: F401  (other modules read cases through this name)


def calculate_metric_percase(pred, gt, device_surface=False, voxelspacing=None, connectivity=1):
    """(dice, jaccard, hd95, asd) of one case, medpy.metric.binary semantics (code/utils/test_3d_patch.py:496-508)."""
    spacing, connectivity = surface.normalise_spacing(voxelspacing, connectivity)
    if not device_surface and spacing is None and connectivity == 1:
        return _host.calculate_metric_percase(pred, gt)
    n_p, n_g, n_i = _host.overlap_counts(pred, gt)
    dice, jc = case_loop.dc_jc(n_p, n_g, n_i)
    if n_g == 0:
        return dice, jc, 0.0, 0.0
    if n_p == 0:                                           # what the host path's surface distances raise
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if device_surface:
        m = surface.surface_metrics(pred, gt, voxelspacing=spacing, connectivity=connectivity)[0].tolist()
        return dice, jc, m[0], m[1]
    return (dice, jc) + case_loop.hd95_asd(case_loop.host_mask(pred), case_loop.host_mask(gt), spacing, connectivity)


def _cases_carry_spacing(cases):
    return isinstance(cases, (list, tuple)) and any(not isinstance(c, (str, bytes)) and len(c) == 3 for c in cases)


def _own_loop(device_surface, voxelspacing, connectivity, cases):
    return device_surface or voxelspacing is not None or connectivity != 1 or _cases_carry_spacing(cases)


def test_all_case(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                  nms=0, preproc_fn=None, test_save_path=None, label_key="label", device_surface=False, voxelspacing=None,
                  connectivity=1, *, postprocess=None, blend=None):
    """`test_3d_patch.test_all_case`; with device_surface=True, a spacing, a connectivity or a list holding (image, label, spacing)
    cases the same loop (:251-291) with `calculate_metric_percase` of this module per case.

    blend (`sliding_window.Blend`, not in the reference) runs the loop here as well.  With device_surface=True the blended loop is
    the device-resident one of `device_eval.test_all_case`: `single_case_device`, `components.largest_component` for `nms` and the
    device metrics, with no host copy of the label map; otherwise the maps go through `test_single_case` to the host as before.

    postprocess (`morphology.PostProcess`, not in the reference) runs the loop here too: the label map of every case goes through it
    on the device after the sliding window and before `nms`; on the route that holds the map on the host the result is copied back."""
    surface.normalise_spacing(voxelspacing, connectivity)
    morphology.check_postprocess(postprocess)
    if blend is None and postprocess is None and not _own_loop(device_surface, voxelspacing, connectivity, cases):
        return _host.test_all_case(model, cases, num_classes, patch_size, stride_xy, stride_z, batch_size=batch_size,
                                   metric_detail=metric_detail, nms=nms, preproc_fn=preproc_fn, test_save_path=test_save_path,
                                   label_key=label_key)

    def device_case(image, label, spacing):
        pred, _ = sliding_window.single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, blend=blend)
        if postprocess is not None:
            pred = postprocess(pred)
        return case_loop.binary_case(pred, label, nms, components.largest_component, lambda p, g: calculate_metric_percase(
            p, g, device_surface=True, voxelspacing=spacing, connectivity=connectivity))

    def per_case(image, label, spacing):
        pred, _ = _host.test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, batch_size=batch_size,
                                         blend=blend)
        if postprocess is not None:
            pred = postprocess(pred).cpu().numpy().astype(pred.dtype)
        return case_loop.binary_case(pred, label, nms, _host.getLargestCC, lambda p, g: calculate_metric_percase(
            p, g, device_surface=device_surface, voxelspacing=spacing, connectivity=connectivity))

    resident = device_surface and blend is not None
    return case_loop.mean_over_cases(cases, device_case if resident else per_case, np.zeros(4), label_key, preproc_fn, triples=True,
                                     voxelspacing=voxelspacing, detail=case_loop.print_metrics if metric_detail else None,
                                     test_save_path=test_save_path)


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
