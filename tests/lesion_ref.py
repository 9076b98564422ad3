"""scipy restatements of the lesion statistics (csrc/lesions.hip, utils/lesions.py) and of the ISLES22 test protocol
(utils/isles_eval.py; code/test_ISLES22.py:98-164), and the hand-made inputs their tests share.

    filtered(mask, connectivity, min_voxels)        the mask without its components of fewer than min_voxels voxels
    counts(pred, gt, connectivity, min_voxels)      int64 (8,): n_gt, n_pred, tp, fn, fp, vox_gt, vox_pred, vox_and
    table(pred, gt, of, connectivity, min_voxels)   int64 (n, 3): label, size, overlap of the surviving lesions of one side
    metrics(counts, voxel_volume, empty_value)      the scores of one row of counts, scalar by scalar
    isles_case(pred, gt, percase)                   dice, hd95, asd, sensitivity, specificity of one case as the script computes them
    HAND                                            name -> (pred, gt) of the hand-made cases
"""
import numpy as np
from scipy import ndimage

FIELDS = ("n_gt", "n_pred", "tp", "fn", "fp", "vox_gt", "vox_pred", "vox_and")


def _label(mask, connectivity):
    return ndimage.label(mask, ndimage.generate_binary_structure(3, connectivity))


def filtered(mask, connectivity=3, min_voxels=1):
    mask = np.asarray(mask) != 0
    labels, n = _label(mask, connectivity)
    keep = np.bincount(labels.ravel(), minlength=n + 1) >= min_voxels
    keep[0] = False
    return keep[labels]


def counts(pred, gt, connectivity=3, min_voxels=1):
    p, g = filtered(pred, connectivity, min_voxels), filtered(gt, connectivity, min_voxels)
    (lp, n_pred), (lg, n_gt) = _label(p, connectivity), _label(g, connectivity)
    both = p & g
    tp = len(np.unique(lg[both]))
    fp = n_pred - len(np.unique(lp[both]))
    return np.array([n_gt, n_pred, tp, n_gt - tp, fp, g.sum(), p.sum(), both.sum()], np.int64)


def table(pred, gt, of="gt", connectivity=3, min_voxels=1):
    p, g = filtered(pred, connectivity, min_voxels), filtered(gt, connectivity, min_voxels)
    mine, other = (g, p) if of == "gt" else (p, g)
    labels, n = _label(mine, connectivity)
    size = np.bincount(labels.ravel(), minlength=n + 1)[1:]
    overlap = np.bincount(labels[mine & other], minlength=n + 1)[1:]
    return np.stack([np.arange(1, n + 1), size, overlap], 1).astype(np.int64).reshape(n, 3)


def metrics(row, voxel_volume=1.0, empty_value=1.0):
    c = {k: float(v) for k, v in zip(FIELDS, row)}
    misses = c["tp"] + c["fp"] + c["fn"]
    return {
        "lesion_f1": c["tp"] / (c["tp"] + (c["fp"] + c["fn"]) / 2) if misses else empty_value,
        "lesion_recall": c["tp"] / c["n_gt"] if c["n_gt"] else empty_value,
        "lesion_precision": (c["n_pred"] - c["fp"]) / c["n_pred"] if c["n_pred"] else empty_value,
        "lesion_count_diff": abs(c["n_pred"] - c["n_gt"]),
        "abs_volume_diff": abs(c["vox_pred"] - c["vox_gt"]) * voxel_volume,
        "dice": 2 * c["vox_and"] / (c["vox_pred"] + c["vox_gt"]) if c["vox_pred"] + c["vox_gt"] else empty_value,
    }


def isles_case(pred, gt, percase=None):
    """code/test_ISLES22.py:98-164 on two binary numpy volumes.  percase(pred, gt) -> (dice, jaccard, hd95, asd) is the evaluator the
    script imports at :127-129; the package's host one (utils/test_3d_patch.py) unless another is given."""
    pred, gt = np.asarray(pred).astype(np.float32), np.asarray(gt).astype(np.float32)
    if pred.sum() == 0 and gt.sum() == 0:                                     # :98-104
        return dict(dice=1.0, hd95=0.0, asd=0.0, sensitivity=1.0, specificity=1.0)
    if pred.sum() == 0 or gt.sum() == 0:                                      # :105-121
        far = float(np.sqrt(float(sum(n * n for n in gt.shape))))
        if gt.sum() == 0:
            return dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=1.0 if pred.sum() == 0 else 0.0)
        return dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=1.0)
    if percase is None:
        from dycon_paper_replication_amd.utils import test_3d_patch
        percase = test_3d_patch.calculate_metric_percase
    dice, _, hd95, asd = percase(pred, gt)                                    # :129-132
    tp = np.sum((pred == 1) & (gt == 1))                                      # :155-161
    tn = np.sum((pred == 0) & (gt == 0))
    fp = np.sum((pred == 1) & (gt == 0))
    fn = np.sum((pred == 0) & (gt == 1))
    return dict(dice=dice, hd95=hd95, asd=asd, sensitivity=tp / (tp + fn + 1e-10), specificity=tn / (tn + fp + 1e-10))


# ------------------------------------------------------------------ the hand-made cases
def checkerboard(shape=(6, 5, 7), parity=0):
    x, y, z = np.indices(shape)
    return ((x + y + z) % 2 == parity).astype(np.uint8)


def cubes():
    """gt = the cube [1:4]^3 and the voxel (6, 6, 6); pred = the voxel (3, 3, 3) and the cube [5:8]^3: each big lesion is hit by a
    single voxel of the other mask, so a size filter of 2 turns both hits into misses"""
    gt, pred = np.zeros((8, 8, 8), np.uint8), np.zeros((8, 8, 8), np.uint8)
    gt[1:4, 1:4, 1:4] = 1
    gt[6, 6, 6] = 1
    pred[3, 3, 3] = 1
    pred[5:8, 5:8, 5:8] = 1
    return pred, gt


def touching():
    """two voxels that meet at a corner: neighbours under 26-connectivity, no shared voxel"""
    gt, pred = np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8)
    gt[1, 1, 1] = 1
    pred[2, 2, 2] = 1
    return pred, gt


HAND = {
    "checker_opposite": (checkerboard(parity=0), checkerboard(parity=1)),
    "checker_same": (checkerboard(parity=0), checkerboard(parity=0)),
    "cubes": cubes(),
    "touching": touching(),
}


def random_pair(shape, density, seed):
    """pred and gt drawn independently"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) < density).astype(np.uint8), (rng.random(shape) < density).astype(np.uint8)
