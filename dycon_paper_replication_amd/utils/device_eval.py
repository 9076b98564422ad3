"""The `test_all_case` family of ``utils/test_3d_patch.py`` with every per-case stage on the device, the `nms` step included.

The functions take the reference's names, arguments and defaults as ``utils/surface_eval.py`` lays them out.  Per case:
``sliding_window.single_case_device`` (the label map as a CUDA tensor), ``components.largest_component`` when `nms` is set
(code/utils/test_3d_patch.py:19-26 on the device, csrc/components.hip), then
``surface_eval.calculate_metric_percase(pred, gt, device_surface=True)`` on the device tensors.  The label map never leaves the
device: per case the host sends the image and the ground truth and reads back one "prediction is empty" flag, three overlap
counts and, unless the ground truth is empty, one row of surface metrics.  The convention for an empty prediction, (0, 0, 0, 0),
and ``performance.txt`` are those of ``test_3d_patch.test_all_case`` (:251-291).  Unit voxel spacing, as everywhere in the
reference's evaluators, unless a case is given as ``(image, label, spacing)``: then HD95 / ASD of that case are in the units of its
spacing (utils/surface.py, csrc/surface_spacing.hip).  The parameter lists stay those of ``utils/test_3d_patch.py``
(tests/test_components_cpu.py pins them), so there is no ``voxelspacing=`` / ``connectivity=`` keyword here;
``surface_eval.test_all_case(..., device_surface=True)`` has both.

    test_all_case(model, cases, num_classes, ..., nms=0)
    test_all_case_BraTS19 / _Pancreas / _ISLES22(..., nms=0)
"""
from __future__ import annotations

import numpy as np

from . import case_loop, components, sliding_window, surface_eval


def _device_case(single_case, nms):
    """the per-case stage of the device-resident loops: `single_case(image)[0]` is the label map as a CUDA tensor"""
    def per_case(image, label, spacing):
        pred, _ = single_case(image)
        return case_loop.binary_case(pred, label, nms, components.largest_component, lambda p, g: surface_eval.calculate_metric_percase(
            p, g, device_surface=True, voxelspacing=spacing))
    return per_case


def test_all_case(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                  nms=0, preproc_fn=None, test_save_path=None, label_key="label"):
    """`test_3d_patch.test_all_case` (:251-291): the mean (dice, jaccard, hd95, asd) over the cases."""
    def single_case(image):
        return sliding_window.single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size)

    return case_loop.mean_over_cases(cases, _device_case(single_case, nms), np.zeros(4), label_key, preproc_fn, triples=True,
                                     detail=case_loop.print_metrics if metric_detail else None, test_save_path=test_save_path)


def test_all_case_BraTS19(model, image_list, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, save_result=True,
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0):
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path)


def test_all_case_Pancreas(model, image_list, num_classes, device=None, patch_size=(96, 96, 64), stride_xy=16, stride_z=4,
                           save_result=True, test_save_path=None, preproc_fn=None, metric_detail=0, nms=0):
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path)


def test_all_case_ISLES22(model, image_list, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, save_result=True,
                          test_save_path=None, preproc_fn=None, metric_detail=0, nms=0):
    return test_all_case(model, image_list, num_classes, patch_size, stride_xy, stride_z, metric_detail=metric_detail, nms=nms,
                         preproc_fn=preproc_fn, test_save_path=test_save_path, label_key="mask")


for _f in (test_all_case, test_all_case_BraTS19, test_all_case_Pancreas, test_all_case_ISLES22):
    _f.__test__ = False        # reference names, not pytest cases
