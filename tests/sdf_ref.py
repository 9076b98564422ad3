"""numpy / scipy restatement of the signed distance maps (csrc/sdf.hip, utils/util.py) and the inputs their tests share.

    inner_boundary(pos)                  skimage.segmentation.find_boundaries(pos, mode="inner"), connectivity 1, restated with scipy
    signed_distance(pos, normalize)      one sample: the map of code/utils/util.py:205-236 in this project's words, or with
                                         normalize=False the signed distance in voxels
    compute_sdf(img_gt, out_shape)       the batch form with the reference's signature
    class_maps(labels, lo, hi, normalize)  (B, hi - lo + 1, x, y, z): signed_distance(labels[b] == c) for c = lo..hi
    blobs(shape, seed), golden_batches(), the helper traces' inputs

compute_sdf is held to the reference's own outputs, arithmetic and order of operations included, by tests/golden/sdf.npz (tests/test_util_cpu.py); the device path is held to these
functions bit for bit (tests/test_sdf_gpu.py).
"""
import numpy as np
from scipy import ndimage
from scipy.ndimage import distance_transform_edt as edt


def inner_boundary(pos):
    """foreground voxels with a background 6-neighbour inside the volume.  skimage dilates and erodes with a padding that repeats the
    volume's own values, so a face of the volume makes no boundary: border_value=1 is that rule for the erosion"""
    pos = np.asarray(pos).astype(bool)
    return pos & ~ndimage.binary_erosion(pos, border_value=1)


def _rescaled(d):
    """d moved and scaled onto [0, 1] by its own minimum and maximum; 0 / 0 (a constant d) is NaN, silently"""
    lo, hi = d.min(), d.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return (d - lo) / (hi - lo)


def signed_distance(pos, normalize=True):
    """float64 map of one sample, positive outside the mask and negative inside, 0 on the inner boundary; all zeros when the mask is
    empty.  normalize=True: the outside and the inside scipy transforms are each rescaled by their own extremes before the inside
    is subtracted, which is what the reference computes (a mask without background comes out NaN through 0 / 0).  normalize=False
    is this package's extension: the distances in voxels, NaN without background by the same rule"""
    pos = np.asarray(pos).astype(bool)
    if not pos.any():
        return np.zeros(pos.shape)
    if normalize:
        out = _rescaled(edt(~pos)) - _rescaled(edt(pos))
    elif pos.all():
        out = np.full(pos.shape, np.nan)
    else:
        out = edt(~pos) - edt(pos)
    out[inner_boundary(pos)] = 0
    return out


def compute_sdf(img_gt, out_shape):
    """float64 array of out_shape; sample b is signed_distance of img_gt[b] (cast to uint8 first, as the reference does), broadcast
    into out_shape[1:] by numpy's assignment; out_shape[0] samples are read"""
    img_gt = np.asarray(img_gt).astype(np.uint8)
    out = np.zeros(out_shape)
    for b, sample in enumerate(img_gt[:out_shape[0]]):
        out[b] = signed_distance(sample != 0)
    return out


def class_maps(labels, lo, hi, normalize=True):
    labels = np.asarray(labels)
    return np.stack([np.stack([signed_distance(vol == c, normalize) for c in range(lo, hi + 1)]) for vol in labels])


def blobs(shape, seed, keep=0.15):
    """seeded smoothed noise, the top `keep` of the voxels"""
    x = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 1.5, mode="nearest")
    return x >= np.quantile(x, 1.0 - keep)


def golden_batches():
    """name -> (img_gt uint8 (2, x, y, z), out_shape): the inputs of tests/golden/sdf.npz.  Blobs; an empty sample (the reference's
    `if posmask.any()` branch); a sample without background (its 0 / 0); a box on three faces of the volume; a single voxel; an
    output with a channel axis"""
    a = np.stack([blobs((12, 10, 9), 1, 0.3), np.zeros((12, 10, 9), bool)])
    b = np.stack([blobs((7, 13, 70), 2, 0.2), np.ones((7, 13, 70), bool)])
    box, one = np.zeros((5, 6, 9), bool), np.zeros((5, 6, 9), bool)
    box[:3, :4, 4:] = True
    one[2, 3, 4] = True
    c = np.stack([box, one])
    return {"a": (a.astype(np.uint8), (2, 12, 10, 9)), "b": (b.astype(np.uint8) * 3, (2, 7, 13, 70)),
            "c": (c.astype(np.uint8), (2, 1, 5, 6, 9))}


# the host helpers' recorded traces (tests/golden/sdf.npz): np.random.seed(HELPER_SEED) right before the sampler is built
HELPER_SEED = 1234
SAMPLER_N = 20
SAMPLER_LISTS = [list(range(0, 7)), list(range(7, 10)), list(range(10, 40))]      # with and without replacement
LR_0 = 0.05
LR_WEIGHT_DECAYS = (1e-4, 5e-3)                                                  # one parameter group each
LR_STEPS = tuple(range(0, 5000, 700))
METER_UPDATES = ((0.5, 1), (0.25, 4), (3.0, 2), (-1.5, 1), (0.125, 8))           # (val, n)
