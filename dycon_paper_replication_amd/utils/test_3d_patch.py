"""Sliding-window evaluation with the reference's names and argument meaning (code/utils/test_3d_patch.py).

    test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=1)   :293-351
    calculate_metric_percase(pred, gt) -> (dice, jaccard, hd95, asd)                 :496-508
    test_all_case(model, cases, ...)                                                 :251-291

`test_single_case` is the class-1 evaluator of utils/sliding_window.py, imported here under the reference's name: the windows run
through the HIP network in batches; score / count maps, the final threshold and the overlap counts behind Dice and Jaccard stay on
the MI355X (csrc/sw_accumulate.h, csrc/eval.hip).  The loop over cases and medpy's arithmetic are utils/case_loop.py's, for the
functions here as for surface_eval.py, device_eval.py, ensemble_eval.py and eval_classes.py; it reads `_read_case`,
`overlap_counts` and `_surface_distances` from this module at call time.  HD95 / ASD are surface-distance metrics of medpy (absent
here, not vendored by the reference): they are restated on scipy.ndimage on the host ("parity unpinned", see oracle/evaluate.py) -- they are
per-case diagnostics off the hot path.  The reference reads h5 files (h5py is not available in this image): `test_all_case`
takes (image, label) arrays, or h5 paths when h5py can be imported.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .case_loop import binary_case, dc_jc, hd95_asd, host_mask, mean_dice, mean_over_cases, print_metrics
from .sliding_window import _windows, single_case_device, test_single_case  # noqa: F401  (the driver and its class-1 evaluator)


def overlap_counts(pred, gt):
    """(|pred|, |gt|, |pred & gt|) on the device.  pred / gt: CUDA tensors (uint8 / int64) or numpy arrays."""
    dev = pred.device if torch.is_tensor(pred) and pred.is_cuda else torch.device("cuda:0")
    p = torch.as_tensor(np.asarray(pred) if not torch.is_tensor(pred) else pred).to(dev).ne(0).to(torch.uint8).contiguous()
    g = torch.as_tensor(np.asarray(gt) if not torch.is_tensor(gt) else gt).to(dev)
    g = (g if g.dtype in (torch.uint8, torch.int64) else g.ne(0).to(torch.uint8)).contiguous()
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    _lib.call("dycon_binary_overlap", p.data_ptr(), g.data_ptr(), g.element_size(), p.numel(), out.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    return tuple(int(v) for v in out.tolist())


def _surface_distances(result, reference, voxelspacing=None, connectivity=1):
    from scipy import ndimage
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    footprint = ndimage.generate_binary_structure(result.ndim, connectivity)
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ ndimage.binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ ndimage.binary_erosion(reference, structure=footprint, iterations=1)
    return ndimage.distance_transform_edt(~reference_border, sampling=voxelspacing)[result_border]


def calculate_metric_percase(pred, gt):
    """(dice, jaccard, hd95, asd) of one case, medpy.metric.binary semantics (code/utils/test_3d_patch.py:496-508)."""
    n_p, n_g, n_i = overlap_counts(pred, gt)
    dice, jc = dc_jc(n_p, n_g, n_i)
    if n_g == 0:
        return dice, jc, 0.0, 0.0
    return (dice, jc) + hd95_asd(host_mask(pred), host_mask(gt))


def getLargestCC(segmentation):
    """Largest connected component of a label map (code/utils/test_3d_patch.py:19-26; skimage.measure.label's default full
    connectivity -- 26 neighbours in 3-D -- on scipy.ndimage, skimage is not vendored by the reference).  An empty map is returned
    unchanged.  The `nms` option of the test_all_case family."""
    from scipy import ndimage
    seg = np.asarray(segmentation)
    labels, n = ndimage.label(seg, structure=np.ones((3,) * seg.ndim, dtype=bool))
    if n == 0:
        return segmentation
    return labels == np.argmax(np.bincount(labels.flat)[1:]) + 1


def _read_case(case, label_key):
    if isinstance(case, (str, bytes)):
        import h5py   # not available in this image; present where the datasets are
        with h5py.File(case, "r") as f:
            return f["image"][:], f[label_key][:]
    return case


def test_all_case(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=4, metric_detail=0,
                  nms=0, preproc_fn=None, test_save_path=None, label_key="label"):
    """cases: iterable of (image, label) arrays, or of h5 paths with 'image' / `label_key` datasets (needs h5py).
    Returns the mean (dice, jaccard, hd95, asd) over the cases; nms keeps the largest connected component of each prediction,
    preproc_fn is applied to the image first, test_save_path receives `../performance.txt` (code/utils/test_3d_patch.py:251-291)."""
    def per_case(image, label, spacing):
        pred, _ = test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, batch_size=batch_size)
        return binary_case(pred, label, nms, getLargestCC, calculate_metric_percase)

    return mean_over_cases(cases, per_case, np.zeros(4), label_key, preproc_fn, detail=print_metrics if metric_detail else None,
                           test_save_path=test_save_path)


def _case_list(root_path, list_name, pattern):
    import os
    with open(os.path.join(root_path, list_name), "r") as f:
        return [pattern.format(root=root_path, case=line.strip()) for line in f if line.strip()]


def _var_all_case(model, cases, num_classes, patch_size, stride_xy, stride_z, label_key, transpose=None):
    return mean_dice(cases, lambda image: test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes),
                     label_key, transpose)


# per-dataset wrappers with the reference's names, defaults and on-disk layouts
def var_all_case_BraTS19(model, root_path, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4):
    return _var_all_case(model, _case_list(root_path, "val.txt", "{root}/data/{case}.h5"), num_classes, patch_size, stride_xy, stride_z,
                         "label", transpose=(2, 1, 0))


def var_all_case_Pancreas(model, root_path, num_classes, patch_size=(112, 112, 80), stride_xy=18, stride_z=4):
    return _var_all_case(model, _case_list(root_path, "test1.list", "{root}/Pancreas_data/{case}"), num_classes, patch_size, stride_xy, stride_z, "label")


def var_all_case_ISLES22(root_path, model, num_classes, device=None, patch_size=(96, 96, 64), stride_xy=16, stride_z=4):
    return _var_all_case(model, _case_list(root_path, "val.list", "{root}/{case}.h5"), num_classes, patch_size, stride_xy, stride_z, "mask")


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
