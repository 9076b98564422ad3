"""Multi-class evaluation on the MI355X (csrc/evalc.hip, utils/eval_classes.py, the class-count names of utils/metrics.py):
the kernels against fp64 numpy / exact integer counts through the C ABI, the evaluator against a one-window-at-a-time restatement
on the same model, the metrics against the per-class binary calls, the fixture recorded from the reference and numpy."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import _lib
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.utils import eval_classes as EC
    from dycon_paper_replication_amd.utils import metrics as M
    from dycon_paper_replication_amd.utils import test_3d_patch as T3
from oracle import nets as ON
from test_eval_classes_cpu import DICE_CASES, binary_batch, dice_case
from test_eval_gpu import _blob

DEV = "cuda"
int3 = ctypes.c_int * 3


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------- sliding-window kernels, C ABI
VOL, PATCH = (13, 9, 7), (8, 6, 5)
FAR = tuple(v - p for v, p in zip(VOL, PATCH))                          # (5, 3, 2): the window clamped at the far faces
CHUNKS = {
    "overlapping": [(0, 0, 0), (1, 1, 0), (2, 0, 1), (1, 2, 1)],
    # opposite corners.  No two windows of 8 x 6 x 5 in 13 x 9 x 7 are disjoint (the patch is longer than half of every axis): these
    # two share only their 3 x 3 x 3 corner, and their bounding box, the whole volume, holds 13*9*7 - (2*240 - 27) = 366 voxels that
    # neither covers
    "far_corners": [(0, 0, 0), FAR],
    "clamped": [FAR, (4, 2, 1), (5, 0, 0)],
}


def _softmax64(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _accumulate(lg, org, score, cnt, C):
    lo, hi = EC.chunk_box(org, PATCH)
    _lib.call("dycon_sw_accumulate_all", lg.data_ptr(), C, len(org), *PATCH, dev(np.asarray(org, np.int32)).data_ptr(), score.data_ptr(),
              cnt.data_ptr(), *VOL, int3(*lo), int3(*hi), stream())


@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_accumulate_all_and_finalize_against_fp64(C):
    """three chunks onto maps that already hold values: an uncovered voxel must keep its bits, inside the chunk's box and outside"""
    rng = np.random.default_rng(100 + C)
    score0 = rng.random((C,) + VOL).astype(np.float32)
    cnt0 = rng.integers(1, 4, VOL).astype(np.float32)
    score, cnt = dev(score0), dev(cnt0)
    ref_score, ref_cnt = score0.astype(np.float64), cnt0.astype(np.float64)
    for name, org in CHUNKS.items():
        logits = (3.0 * rng.standard_normal((len(org),) + PATCH + (C,))).astype(np.float32)
        before_s, before_c = score.cpu().numpy(), cnt.cpu().numpy()
        _accumulate(dev(logits), org, score, cnt, C)
        covered = np.zeros(VOL, bool)
        prob = _softmax64(logits.astype(np.float64))
        for p, (x, y, z) in enumerate(org):
            win = (slice(x, x + PATCH[0]), slice(y, y + PATCH[1]), slice(z, z + PATCH[2]))
            ref_score[(slice(None),) + win] += np.moveaxis(prob[p], -1, 0)
            ref_cnt[win] += 1
            covered[win] = True
        got_s, got_c = score.cpu().numpy(), cnt.cpu().numpy()
        lo, hi = EC.chunk_box(org, PATCH)
        in_box = np.zeros(VOL, bool)
        in_box[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
        assert covered.sum() > 0 and not (covered & ~in_box).any()
        if name == "far_corners":
            assert (in_box & ~covered).sum() == 366
        assert np.array_equal(got_s[:, ~covered].view(np.uint32), before_s[:, ~covered].view(np.uint32)), name
        assert np.array_equal(got_c[~covered].view(np.uint32), before_c[~covered].view(np.uint32)), name
        np.testing.assert_array_equal(got_c, ref_cnt, err_msg=name)
        np.testing.assert_allclose(got_s, ref_score, rtol=1e-4, atol=1e-5, err_msg=name)       # the project's fp32 bound
    assert ref_cnt.max() >= 5
    n = cnt.numel()
    label, prob = torch.empty(VOL, dtype=torch.uint8, device=DEV), torch.empty_like(score)
    _lib.call("dycon_sw_finalize_argmax", score.data_ptr(), cnt.data_ptr(), C, n, label.data_ptr(), prob.data_ptr(), stream())
    ref_prob = ref_score / ref_cnt
    np.testing.assert_allclose(prob.cpu().numpy(), ref_prob, rtol=1e-4, atol=1e-5)
    top = np.sort(ref_prob, 0)
    decided = top[-1] - top[-2] > 4e-5
    assert decided.mean() > 0.9
    assert np.array_equal(label.cpu().numpy()[decided], ref_prob.argmax(0)[decided])
    # prob may be NULL, and may be the score map itself: same labels, same probabilities
    label2 = torch.empty_like(label)
    _lib.call("dycon_sw_finalize_argmax", score.data_ptr(), cnt.data_ptr(), C, n, label2.data_ptr(), None, stream())
    assert torch.equal(label2, label)
    alias, label3 = score.clone(), torch.empty_like(label)
    _lib.call("dycon_sw_finalize_argmax", alias.data_ptr(), cnt.data_ptr(), C, n, label3.data_ptr(), alias.data_ptr(), stream())
    assert torch.equal(label3, label) and torch.equal(alias, prob)


@pytest.mark.parametrize("C", [2, 3, 8])
def test_accumulate_entry_points_share_their_bits(C):
    """One kernel body serves the four accumulate entry points, so on the same logits, bit for bit: class 1 of dycon_sw_accumulate_c
    is plane 1 of dycon_sw_accumulate_all over the chunk's box, and a model ensembled with itself (dycon_sw_accumulate_ens, M = 2)
    is dycon_sw_accumulate for 2 classes and dycon_sw_accumulate_c for more.  The maps hold random values beforehand: whatever a
    launch does not cover, inside its box or outside, keeps its bits."""
    rng = np.random.default_rng(300 + C)
    all0 = rng.random((C,) + VOL).astype(np.float32)
    cnt0 = rng.integers(1, 4, VOL).astype(np.float32)
    s_all, c_all = dev(all0), dev(cnt0)
    s_c, c_c = dev(all0[1]), dev(cnt0)
    s_one, c_one = dev(all0[1]), dev(cnt0)
    s_ens, c_ens = dev(all0[1]), dev(cnt0)
    for name, org in CHUNKS.items():
        lg = dev((3.0 * rng.standard_normal((len(org),) + PATCH + (C,))).astype(np.float32))
        origins = dev(np.asarray(org, np.int32))
        before_all, before_cnt = s_all.clone(), c_all.clone()
        _accumulate(lg, org, s_all, c_all, C)
        _lib.call("dycon_sw_accumulate_c", lg.data_ptr(), C, len(org), *PATCH, origins.data_ptr(), s_c.data_ptr(), c_c.data_ptr(), *VOL,
                  stream())
        assert torch.equal(s_all[1], s_c) and torch.equal(c_all, c_c), name
        lo, hi = EC.chunk_box(org, PATCH)
        outside = torch.ones(VOL, dtype=torch.bool, device=DEV)
        outside[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = False
        assert torch.equal(s_all[:, outside], before_all[:, outside]) and torch.equal(c_all[outside], before_cnt[outside]), name
        assert not torch.equal(c_all, before_cnt), name
        if C == 2:
            _lib.call("dycon_sw_accumulate", lg.data_ptr(), len(org), *PATCH, origins.data_ptr(), s_one.data_ptr(), c_one.data_ptr(), *VOL,
                      stream())
        else:
            s_one, c_one = s_c, c_c
        _lib.call("dycon_sw_accumulate_ens", lg.data_ptr(), lg.data_ptr(), None, None, 2, C, len(org), *PATCH, origins.data_ptr(),
                  s_ens.data_ptr(), c_ens.data_ptr(), *VOL, stream())
        assert torch.equal(s_ens, s_one) and torch.equal(c_ens, c_one), name


@pytest.mark.parametrize("C", [2, 3, 5, 8])
def test_exact_tie_yields_the_lower_index(C):
    """two classes with identical logits in every covering window, both the maximum: identical sums, and np.argmax's answer"""
    lower, upper = (0, 1) if C == 2 else (1, C - 1)
    rng = np.random.default_rng(200 + C)
    org = [(x, y, z) for x in (0, FAR[0]) for y in (0, FAR[1]) for z in (0, FAR[2])]         # the eight corner windows cover the volume
    logits = rng.standard_normal((len(org),) + PATCH + (C,)).astype(np.float32)
    logits[..., lower] = logits[..., upper] = logits.max(-1) + rng.random(logits.shape[:-1]).astype(np.float32)
    score = torch.zeros((C,) + VOL, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(VOL, dtype=torch.float32, device=DEV)
    _accumulate(dev(logits), org, score, cnt, C)
    assert float(cnt.min()) >= 1 and float(cnt.max()) == 8
    assert torch.equal(score[lower], score[upper])
    for k in set(range(C)) - {lower, upper}:
        assert bool((score[k] < score[lower]).all())
    label = torch.empty(VOL, dtype=torch.uint8, device=DEV)
    _lib.call("dycon_sw_finalize_argmax", score.data_ptr(), cnt.data_ptr(), C, cnt.numel(), label.data_ptr(), score.data_ptr(), stream())
    assert bool((label == lower).all())
    assert np.array_equal(score.cpu().numpy().argmax(0), np.full(VOL, lower))


# ------------------------------------------------------------------------------------------------- confusion counts and argmax
def _confusion(pred, gt, C):
    out = torch.zeros(C * C + 1, dtype=torch.int64, device=DEV)
    p, g = dev(pred), dev(gt)
    _lib.call("dycon_class_confusion", p.data_ptr(), g.data_ptr(), g.element_size(), p.numel(), C, out.data_ptr(), stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("n", [7, 256, 1000, 256 * 4096 + 3])
def test_class_confusion_is_exact(n, gt_dtype, C):
    rng = np.random.default_rng(n % 1000 + C)
    pred, gt = rng.integers(0, C, n).astype(np.uint8), rng.integers(0, C, n).astype(gt_dtype)
    got = _confusion(pred, gt, C)
    assert np.array_equal(got[:C * C], np.bincount(pred.astype(np.int64) * C + gt.astype(np.int64), minlength=C * C))
    assert got[C * C] == 0 and got.sum() == n


@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int64])
def test_class_confusion_counts_out_of_range_labels_only_in_the_last_slot(gt_dtype):
    C, n = 3, 5000
    rng = np.random.default_rng(9)
    pred, gt = rng.integers(0, C + 2, n).astype(np.uint8), rng.integers(0, C + 2, n).astype(gt_dtype)
    pred[:3] = 255
    if gt_dtype is np.int64:
        gt[3:9] = (-1, -2 ** 40, 2 ** 40, 256, 2 ** 32, 2 ** 32 + 1)          # values whose low byte or word would be in range
    ok = (pred < C) & (gt >= 0) & (gt < C)
    got = _confusion(pred, gt, C)
    assert 0 < ok.sum() < n
    assert np.array_equal(got[:C * C], np.bincount(pred[ok].astype(np.int64) * C + gt[ok].astype(np.int64), minlength=C * C))
    assert got[C * C] == n - ok.sum()


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.int64])
def test_batch_class_confusion_and_argmax_labels(C, gt_dtype):
    B, V = 3, 1000
    rng = np.random.default_rng(40 + C)
    logits = torch.from_numpy(rng.standard_normal((B, V, C)).astype(np.float32))
    logits[0, 5, 1] = logits[0, 5, 2] = logits[0, 5].max() + 1.0                  # a tie between classes 1 and 2: class 1
    logits[1, 7] = 0.25                                                           # every class ties: class 0
    logits[2, 9, C - 1] = logits[2, 9, 0] = logits[2, 9].max() + 0.5             # first against last: class 0
    labels = torch.from_numpy(rng.integers(0, C, (B, V))).to(gt_dtype)
    labels[1, :4] = C                                                             # out of range: counted in the last slot only
    ref = torch.argmax(logits, dim=-1)
    assert ref[0, 5] == 1 and ref[1, 7] == 0 and ref[2, 9] == 0
    lg, lab = logits.to(DEV), labels.to(DEV)
    arg = torch.empty((B, V), dtype=torch.uint8, device=DEV)
    _lib.call("dycon_argmax_labels", lg.data_ptr(), C, B * V, arg.data_ptr(), stream())
    assert torch.equal(arg.cpu().long(), ref)
    out = torch.zeros((B, C * C + 1), dtype=torch.int64, device=DEV)
    _lib.call("dycon_batch_class_confusion", lg.data_ptr(), lab.data_ptr(), lab.element_size(), B, V, C, out.data_ptr(), stream())
    out = out.cpu().numpy()
    for b in range(B):
        ok = labels[b].numpy() < C
        exp = np.bincount(ref[b].numpy()[ok] * C + labels[b].numpy()[ok].astype(np.int64), minlength=C * C)
        assert np.array_equal(out[b, :C * C], exp), b
        assert out[b, C * C] == (4 if b == 1 else 0)


# ------------------------------------------------------------------------------------------------- evaluator against a restatement
PATCH_NET, STRIDE_XY, STRIDE_Z = (32, 32, 16), 8, 4


def _single_case_classes_restated(model, image, stride_xy, stride_z, patch_size, C):
    """the multi-class form code/utils/test_3d_patch.py:293-351 was derived from: one window at a time, torch.softmax of all
    channels, numpy accumulation, np.argmax"""
    w, h, d = image.shape
    pads = [max(p - s, 0) for p, s in zip(patch_size, (w, h, d))]
    lo = [p // 2 for p in pads]
    hi = [p - p // 2 for p in pads]
    if any(pads):
        image = np.pad(image, [(lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2])], mode="constant", constant_values=0)
    ww, hh, dd = image.shape
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    score_map = np.zeros((C,) + image.shape).astype(np.float32)
    cnt = np.zeros(image.shape).astype(np.float32)
    for x in range(sx):
        xs = min(stride_xy * x, ww - patch_size[0])
        for y in range(sy):
            ys = min(stride_xy * y, hh - patch_size[1])
            for z in range(sz):
                zs = min(stride_z * z, dd - patch_size[2])
                patch = image[xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]]
                patch = torch.from_numpy(np.expand_dims(np.expand_dims(patch, 0), 0).astype(np.float32)).to(DEV)
                with torch.no_grad():
                    y_ = torch.softmax(model(patch)[1], dim=1)
                score_map[:, xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]] += y_.cpu().numpy()[0]
                cnt[xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]] += 1
    score_map = score_map / np.expand_dims(cnt, 0)
    label_map = np.argmax(score_map, axis=0)
    if any(pads):
        label_map = label_map[lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d]
        score_map = score_map[:, lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d]
    return label_map, score_map, sx * sy * sz


@functools.lru_cache(maxsize=None)
def _model(net_type, C):
    params = (ON.make_vnet_params if net_type == "vnet" else ON.make_unet_params)(3, n_classes=C)
    model = net_factory_3d(net_type, 1, C, 2, dtype=torch.float32).to(DEV).eval()
    model.load_state_dict(params)
    return model


@functools.lru_cache(maxsize=None)
def _restated(net_type, C, shape):
    """(image, label, score, windows): computed once per model and volume, shared by the batch sizes, never written to"""
    image = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    out = (image,) + _single_case_classes_restated(_model(net_type, C), image, STRIDE_XY, STRIDE_Z, PATCH_NET, C)
    for a in out[1:3]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("batch_size", [4, 5])
@pytest.mark.parametrize("shape", [(40, 36, 24), (24, 20, 10)], ids=["overlapping", "padded"])
@pytest.mark.parametrize("C", [3, 5])
@pytest.mark.parametrize("net_type", ["vnet", "unet_3D"])
def test_single_case_classes_matches_restatement(net_type, C, shape, batch_size):
    """40 x 36 x 24: 12 overlapping windows, clamped at the far faces; batch_size 5 does not divide them, so chunks straddle rows.
    24 x 20 x 10: smaller than the window, the padding path."""
    image, ref_label, ref_score, nwin = _restated(net_type, C, shape)
    assert nwin == (12 if shape == (40, 36, 24) else 1)
    label, score = EC.test_single_case_classes(_model(net_type, C), image, STRIDE_XY, STRIDE_Z, PATCH_NET, batch_size=batch_size)
    assert label.shape == shape and label.dtype == np.int64 and score.shape == (C,) + shape and score.dtype == np.float32
    err = np.abs(score - ref_score).max()
    top = np.sort(ref_score.astype(np.float64), 0)
    decided = top[-1] - top[-2] > 4e-5                       # twice the two-sided score bound
    classes = np.unique(label)
    print(f"{net_type} C={C} {shape} batch {batch_size}: |score - restated| {err:.3e}; {int((~decided).sum())} of {decided.size} voxels "
          f"undecided; labels {classes.tolist()}; |sum - 1| {np.abs(score.sum(0) - 1).max():.3e}")
    assert err <= 1e-5
    assert (~decided).sum() < 1e-3 * decided.size
    assert np.array_equal(label[decided], ref_label[decided])
    assert label.min() >= 0 and label.max() < C and len(classes) >= 3
    assert np.abs(score.sum(0, dtype=np.float64) - 1).max() <= 1e-5
    # the device-resident form returns the same maps without host copies
    if batch_size == 4:
        lab_d, score_d = EC.single_case_classes_device(_model(net_type, C), image, STRIDE_XY, STRIDE_Z, PATCH_NET, batch_size=4)
        assert lab_d.is_cuda and lab_d.dtype == torch.uint8 and score_d.is_cuda
        assert np.array_equal(lab_d.cpu().numpy(), label) and np.array_equal(score_d.cpu().numpy(), score)


def test_single_case_classes_takes_the_class_count_from_the_logits():
    """a module that declares no n_classes: C is the channel count of its logits; one class is refused"""
    class Net(torch.nn.Module):
        def __init__(self, C):
            super().__init__()
            self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, C).reshape(1, C, 1, 1, 1))

        def forward(self, x):
            return None, x * self.w

    image = np.random.default_rng(1).standard_normal((20, 16, 8)).astype(np.float32)
    label, score = EC.test_single_case_classes(Net(4).to(DEV), image, 8, 4, (16, 16, 8), batch_size=3)
    prob = torch.softmax(torch.from_numpy(image)[None] * torch.linspace(-1.0, 1.0, 4).reshape(4, 1, 1, 1), 0).numpy()
    np.testing.assert_allclose(score, prob, rtol=1e-4, atol=1e-5)                 # every window sees the same voxel-wise logits
    clear = np.abs(image) > 1e-3                                                  # away from the four-way tie at 0
    assert np.array_equal(label[clear], np.where(image > 0, 3, 0)[clear]) and clear.mean() > 0.99
    with pytest.raises(ValueError, match="2..8 classes"):
        EC.test_single_case_classes(Net(1).to(DEV), image, 8, 4, (16, 16, 8))


# ------------------------------------------------------------------------------------------------- metrics
SHAPE = (40, 36, 28)


def _three_blobs(shift):
    lab = np.zeros(SHAPE, np.int64)
    for c, (centre, radius) in enumerate((((12, 12, 10), 7), ((28, 22, 16), 6), ((14, 28, 20), 4)), 1):
        lab[_blob(SHAPE, tuple(v + shift for v in centre), radius)] = c
    return lab


def test_metric_perclass_matches_the_per_class_binary_calls():
    gt, pred = _three_blobs(0), _three_blobs(2)
    got = EC.calculate_metric_perclass(pred, gt, 4)
    assert got.shape == (3, 4)
    for c in (1, 2, 3):
        ref = T3.calculate_metric_percase((pred == c).astype(np.uint8), (gt == c).astype(np.int64))
        np.testing.assert_allclose(got[c - 1], ref, rtol=1e-12, atol=0)
        assert 0 < got[c - 1, 0] < 1 and got[c - 1, 2] > 0
    on_dev = EC.calculate_metric_perclass(torch.from_numpy(pred).to(DEV).to(torch.uint8), torch.from_numpy(gt).to(DEV), 4)
    np.testing.assert_array_equal(on_dev, got)
    conf = EC.confusion_counts(pred, gt, 4)
    assert conf.is_cuda and conf.dtype == torch.int64 and conf.shape == (4, 4)
    assert np.array_equal(conf.cpu().numpy(), np.bincount((pred * 4 + gt).ravel(), minlength=16).reshape(4, 4))
    np.testing.assert_allclose(EC.metrics_from_confusion(conf), got[:, :2], rtol=1e-12)
    with pytest.raises(ValueError, match="outside"):
        EC.confusion_counts(pred, gt, 3)                      # class 3 occurs
    bad = pred.copy()
    bad[0, 0, 0] = -1
    with pytest.raises(ValueError, match="1 voxels"):
        EC.confusion_counts(bad, gt, 4)


def test_metric_perclass_empty_class_conventions():
    gt, pred = _three_blobs(0), _three_blobs(1)
    pred[pred == 2] = 0                 # class 2: absent from the prediction
    gt[gt == 3] = 0                     # class 3: absent from the ground truth
    got = EC.calculate_metric_perclass(pred, gt, 5)           # class 4: absent from both
    assert 0 < got[0, 0] < 1 and got[0, 2] > 0
    assert got[1].tolist() == [0.0, 0.0, 0.0, 0.0]            # :268-271
    assert got[2].tolist() == [0.0, 0.0, 0.0, 0.0]            # dice = jaccard = 0 without overlap, hd95 = asd = 0 (:500-503)
    assert got[3].tolist() == [0.0, 0.0, 0.0, 0.0]
    same = EC.calculate_metric_perclass(gt, gt, 3)
    assert same.tolist() == [[1.0, 1.0, 0.0, 0.0], [1.0, 1.0, 0.0, 0.0]]


def test_all_case_classes(tmp_path):
    """a 'network' whose logits put class c on blob c: Dice 1 per class, performance.txt written as test_all_case writes it"""
    gt = _three_blobs(0)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):                                  # the image holds the label: one-hot logits
            return None, torch.cat([4.0 * (x == c).float() for c in range(4)], 1)

    (tmp_path / "pred").mkdir()
    net = Net().to(DEV)
    m = EC.test_all_case_classes(net, [(gt.astype(np.float32), gt), (gt.astype(np.float32), gt)], 4, patch_size=(32, 32, 16),
                                 stride_xy=8, stride_z=8, batch_size=5, test_save_path=str(tmp_path) + "/pred/")
    assert m.shape == (3, 4) and np.array_equal(m, [[1.0, 1.0, 0.0, 0.0]] * 3)
    assert (tmp_path / "performance.txt").read_text().startswith("average metric is")
    shifted = EC.test_all_case_classes(net, [(gt.astype(np.float32), _three_blobs(2))], 4, patch_size=(32, 32, 16), stride_xy=8,
                                       stride_z=8, preproc_fn=lambda a: a)
    np.testing.assert_allclose(shifted, EC.calculate_metric_perclass(gt, _three_blobs(2), 4), rtol=1e-12)
    with pytest.raises(ValueError, match="the model has 4 classes"):
        EC.test_all_case_classes(net, [(gt.astype(np.float32), gt)], 3, patch_size=(32, 32, 16), stride_xy=8, stride_z=8)


def test_dice_matches_the_reference_fixture():
    g = load_golden("eval_classes")
    for i, name in enumerate(DICE_CASES):
        inp, tgt, k = dice_case(name)
        for args in ((inp, tgt), (torch.as_tensor(inp).to(DEV), torch.as_tensor(tgt).to(DEV))):
            plain, ignored = M.dice(*args), M.dice(*args, ignore_index=k)
            assert plain.is_cuda and plain.dim() == 0 and ignored.dim() == 0
            np.testing.assert_allclose(plain.item(), g["dice.plain"][i], rtol=1e-6, err_msg=name)
            np.testing.assert_allclose(ignored.item(), g["dice.ignored"][i], rtol=1e-6, err_msg=name)


def test_class_dice_from_logits():
    g = load_golden("eval_classes")
    out, lab = binary_batch()
    # two classes: binary maps as logits whose argmax is the map, against the reference's compute_dice / compute_jaccard
    logits = dev(np.stack([np.zeros_like(out), out - 0.5], -1))
    labels = dev(lab.astype(np.int64))
    d = M.class_dice_from_logits(logits, labels)
    assert d.is_cuda and d.shape == (out.shape[0], 1)
    np.testing.assert_allclose(d[:, 0].cpu().numpy(), g["batch.dice"], rtol=1e-6)
    np.testing.assert_allclose((d / (2 - d))[:, 0].cpu().numpy(), g["batch.jaccard"], rtol=1e-6)       # J = D / (2 - D)
    np.testing.assert_array_equal(M.class_dice_from_logits(logits.permute(0, 4, 1, 2, 3), labels.to(torch.uint8)).cpu().numpy(),
                                  d.cpu().numpy())
    # three classes: numpy cal_dice of the argmax, per sample
    rng = np.random.default_rng(23)
    B, shape, C = 3, (12, 10, 9), 3
    lg = rng.standard_normal((B, C) + shape).astype(np.float32)
    lb = rng.integers(0, C, (B,) + shape)
    got = M.class_dice_from_logits(dev(lg), dev(lb))
    assert got.shape == (B, C - 1)
    ref = np.stack([M.cal_dice(lg[b].argmax(0), lb[b], C) for b in range(B)])
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-12)
    # the CUDA cal_dice against the numpy cal_dice; labels outside [0, num) belong to no class in either
    pred, lab4 = rng.integers(0, 6, shape), rng.integers(0, 6, shape)
    got = M.cal_dice(dev(pred), dev(lab4), 4)
    assert got.is_cuda and got.shape == (3,)
    np.testing.assert_allclose(got.cpu().numpy(), M.cal_dice(pred, lab4, 4), rtol=1e-12)
    np.testing.assert_allclose(M.cal_dice(dev(pred.astype(np.uint8)), dev(lab4.astype(np.uint8)), 4).cpu().numpy(),
                               M.cal_dice(pred, lab4, 4), rtol=1e-12)


def _isles_val_restated(model, volume, label, patch_size):
    """code/train_DyCON_ISLES22.py:351-370 for one case, line by line; metrics.dice restated in numpy (utils/metrics.py:39-75)"""
    import torch.nn.functional as F
    volume_batch = torch.from_numpy(volume).unsqueeze(0).unsqueeze(0).to(DEV)
    label_batch = torch.from_numpy(label).unsqueeze(0).unsqueeze(0).to(DEV)
    if volume_batch.shape[2] < patch_size[0] or volume_batch.shape[3] < patch_size[1] or volume_batch.shape[4] < patch_size[2]:
        pw = max((patch_size[0] - volume_batch.shape[2]) // 2 + 1, 0)
        ph = max((patch_size[1] - volume_batch.shape[3]) // 2 + 1, 0)
        pd = max((patch_size[2] - volume_batch.shape[4]) // 2 + 1, 0)
        volume_batch = F.pad(volume_batch, [pd, pd, ph, ph, pw, pw], mode="constant", value=0)
        label_batch = F.pad(label_batch, [pd, pd, ph, ph, pw, pw], mode="constant", value=0)
    with torch.no_grad():
        outputs, _, _ = model(volume_batch)
    outputs_soft = torch.softmax(outputs, dim=1)
    outputs = torch.argmax(outputs_soft, dim=1).squeeze(0).cpu().numpy()
    y = label_batch.squeeze(0).squeeze(0).cpu().numpy()
    i, t = (outputs == 1).astype(np.float64), (y == 1).astype(np.float64)
    return (2.0 * (i * t).sum() + 1.0) / (i.sum() + t.sum() + 1.0), outputs.shape, int(i.sum())


@pytest.mark.parametrize("shape,patch", [((32, 32, 16), (32, 32, 16)), ((28, 32, 12), (30, 30, 14))], ids=["whole", "padded_to_16"])
def test_isles_val_dice_matches_restatement(shape, patch):
    """28 x 32 x 12 under a 30 x 30 x 14 patch: padded by (2, 0, 2) per side to 32 x 32 x 16"""
    model = _model("vnet", 3)
    rng = np.random.default_rng(31)
    volume = rng.standard_normal(shape).astype(np.float32)
    label = rng.integers(0, 3, shape)
    ref, padded, n_pred = _isles_val_restated(model, volume, label, patch)
    assert padded == (32, 32, 16)
    got = EC.isles_val_dice(model, volume, label, patch)
    assert got.is_cuda and got.dim() == 0
    print(f"isles {shape}: dice {got.item():.6f} restated {ref:.6f}, {n_pred} voxels of class 1")
    np.testing.assert_allclose(got.item(), ref, rtol=1e-6)
    assert not model.training


def test_isles_val_dice_passes_the_nets_shape_error_through():
    """24 x 20 x 10 under 32 x 32 x 16 pads to 34 x 46 x 18 (the `// 2 + 1` of :358-360): the net refuses it"""
    with pytest.raises(ValueError, match="divisible by 16"):
        EC.isles_val_dice(_model("vnet", 3), np.zeros((24, 20, 10), np.float32), np.zeros((24, 20, 10), np.int64), (32, 32, 16))


def test_async_class_train_metrics():
    rng = np.random.default_rng(3)
    B, C, shape = 2, 3, (12, 10, 8)
    logits = dev(rng.standard_normal((B, C) + shape).astype(np.float32))
    label = dev(rng.integers(0, C, (B,) + shape))
    m = M.AsyncClassTrainMetrics(every=1)
    m.update(0, logits, label)
    m.close()
    m._t.join(timeout=60)                                     # the worker drains its queue and ends
    got = m.latest()
    assert got["iter"] == 0 and got["dice"].is_cuda and got["dice"].shape == (B, C - 1)
    np.testing.assert_array_equal(got["dice"].cpu().numpy(), M.class_dice_from_logits(logits, label).cpu().numpy())
    hd = M.compute_hd95(logits.argmax(1) == 1, label == 1, float(np.linalg.norm(shape)))
    assert got["hd95"] is not None and got["hd95"][0] == 0 and got["hd95"][1] == pytest.approx(float(np.mean(hd)))
    m = M.AsyncClassTrainMetrics(every=0)                     # Dice only
    m.update(7, logits.permute(0, 2, 3, 4, 1), label)
    m.close()
    assert m.latest()["iter"] == 7 and m.latest()["hd95"] is None and m.latest()["dice"].shape == (B, C - 1)
