"""Surface distances on the MI355X (csrc/surface.hip, utils/surface.py): the integer histograms against their numpy restatement bit for
bit, HD95 / ASD against the oracle's scipy path at the tolerance tests/test_eval_gpu.py holds the metric path to (rtol 1e-12: the
fp64 summation order is the only difference), and the opt-in entry points of utils.metrics, utils.test_3d_patch and
utils.eval_classes against their host forms."""
import functools

import numpy as np
import pytest
import torch

import surface_ref as SR
from oracle import evaluate as OE

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import metrics as M
from dycon_paper_replication_amd.utils import surface
from dycon_paper_replication_amd.utils import surface_eval as SE
from dycon_paper_replication_amd.utils import test_3d_patch as T3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("blobs", "face", "corners", "full_vs_voxel", "identical", "plates")
RTOL = 1e-12


@functools.lru_cache(maxsize=None)
def _cases(shape):
    return SR.cases(shape)


@functools.lru_cache(maxsize=None)
def _ref_hists(shape, name):
    return SR.hists(*_cases(shape)[name])


@functools.lru_cache(maxsize=None)
def _oracle(shape, name):
    a, b = _cases(shape)[name]
    return float(OE.hd95(a, b)), float(OE.asd(a, b)), float(OE.asd(b, a))


def _stack(shape, names, side, dtype):
    return torch.from_numpy(np.stack([_cases(shape)[n][side] for n in names]).astype(dtype)).to(DEV)


@pytest.mark.parametrize("gt_dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("names", [NAMES[:3], NAMES[3:]], ids=["first3", "last3"])
@pytest.mark.parametrize("shape", SR.SHAPES)
def test_hists_equal_the_restatement(shape, names, gt_dtype):
    """3 pairs per call; the counts and the border sizes are integers and must be equal"""
    hist, nborder = surface.surface_hists(_stack(shape, names, 0, np.uint8), _stack(shape, names, 1, gt_dtype))
    assert hist.is_cuda and hist.dtype == torch.int32 and hist.shape == (3, 2, SR.nbins_of(shape)) and nborder.shape == (3, 2)
    ref = [_ref_hists(shape, n) for n in names]
    assert torch.equal(nborder.cpu(), torch.from_numpy(np.stack([r[1] for r in ref])).to(torch.int32))
    assert torch.equal(hist.cpu(), torch.from_numpy(np.stack([r[0] for r in ref])).to(torch.int32))


def test_class_form_on_a_label_map():
    """cls_lo = 1, n_cls = 3 in one call over two 4-class volumes: pair v * 3 + k is class 1 + k of volume v"""
    shape = (24, 40, 72)
    maps = []
    for seed in range(4):                                     # label = number of overlapping blobs, clipped to 3
        maps.append(np.minimum(sum(SR._blobs(shape, 100 * seed + j).astype(np.int64) for j in range(4)), 3))
    pred, gt = np.stack(maps[:2]), np.stack(maps[2:])
    pred[1][pred[1] == 3] = 0                                 # class 3 absent from the prediction of volume 1
    for gt_t in (torch.from_numpy(gt).to(DEV), torch.from_numpy(gt.astype(np.uint8)).to(DEV)):
        hist, nborder = surface.surface_hists(torch.from_numpy(pred.astype(np.uint8)).to(DEV), gt_t, classes=(1, 3))
        assert hist.shape == (6, 2, SR.nbins_of(shape))
        for v in range(2):
            for k in range(3):
                rh, rn = SR.hists(pred[v] == 1 + k, gt[v] == 1 + k)
                assert torch.equal(hist[v * 3 + k].cpu(), torch.from_numpy(rh).to(torch.int32)), (v, k)
                assert nborder[v * 3 + k].tolist() == rn.tolist()
    assert nborder[5, 0].item() == 0 and hist[5].sum().item() == 0


@pytest.mark.parametrize("shape", SR.SHAPES)
def test_metrics_match_the_oracle(shape):
    a, b = _stack(shape, NAMES, 0, np.uint8), _stack(shape, NAMES, 1, np.uint8)
    got = surface.surface_metrics(a, b)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (6, 5)
    got = got.cpu().numpy()
    from_numpy = surface.surface_metrics(a.cpu().numpy(), b.cpu().numpy()).cpu().numpy()       # numpy in: the same bits
    assert np.array_equal(got, from_numpy)
    for i, name in enumerate(NAMES):
        hd, ab, ba = _oracle(shape, name)
        print(f"{shape} {name}: hd95 {got[i, 0]!r} - oracle = {got[i, 0] - hd:.3e}; asd {got[i, 1] - ab:.3e}, {got[i, 2] - ba:.3e}")
        np.testing.assert_allclose(got[i, :3], [hd, ab, ba], rtol=RTOL, atol=0)
        assert got[i, 3:].tolist() == _ref_hists(shape, name)[1].tolist()
    np.testing.assert_allclose(got, surface.metrics_from_hists(*surface.surface_hists(a, b)), rtol=RTOL, atol=0)


def test_pairs_go_in_chunks_over_the_workspace_budget(monkeypatch):
    """6 volumes x 2 classes with room for 2 volumes per launch sequence: the same integers as in one piece"""
    shape = (17, 33, 70)
    a = torch.from_numpy(np.stack([_cases(shape)[n][0] for n in NAMES]).astype(np.uint8) * 2).to(DEV)
    b = torch.from_numpy(np.stack([_cases(shape)[n][1] for n in NAMES]).astype(np.int64) * 2).to(DEV)
    a[:, ::2], b[:, 1::3] = a[:, ::2] // 2, b[:, 1::3] // 2                       # label maps with the classes 1 and 2
    whole = surface.surface_hists(a, b, classes=(1, 2))
    monkeypatch.setattr(surface, "WORKSPACE_BUDGET", 2 * int(_lib.load().dycon_surface_workspace(2, *shape)) + 5)
    parts = surface.surface_hists(a, b, classes=(1, 2))
    assert whole[0].shape[0] == 12 and whole[1].sum().item() > 0
    assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])


@pytest.mark.parametrize("q", [0.0, 50.0, 77.5, 100.0])
def test_other_percentiles(q):
    a, b = _cases((17, 33, 70))["blobs"]
    both = np.hstack((OE.surface_distances(a, b), OE.surface_distances(b, a)))
    got = surface.surface_metrics(a, b, q=q)[0, 0].item()
    np.testing.assert_allclose(got, np.percentile(both, q), rtol=RTOL, atol=0)


def test_empty_masks():
    shape = (17, 33, 70)
    m = _cases(shape)["blobs"][0]
    e = np.zeros(shape, bool)
    a, b = np.stack([e, m, e, m]), np.stack([m, e, e, m])
    got = surface.surface_metrics(a, b).cpu().numpy()
    nb = int(SR.border6(m).sum())
    assert np.isnan(got[:3, :3]).all()
    assert got[:3, 3:].tolist() == [[0, nb], [nb, 0], [0, 0]]
    assert got[3].tolist() == [0.0, 0.0, 0.0, nb, nb]
    hist, _ = surface.surface_hists(a, b)
    assert hist[:3].sum().item() == 0
    max_dist = float(np.linalg.norm(shape))
    a[3] = _cases(shape)["blobs"][1]
    dev = M.compute_hd95_device(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), max_dist)
    assert dev.is_cuda and dev.dtype == torch.float64 and dev.shape == (4,)
    host = M.compute_hd95(a, b, max_dist)
    assert dev[:3].tolist() == [max_dist] * 3 == host[:3]
    np.testing.assert_allclose(dev.cpu().numpy(), host, rtol=RTOL, atol=0)
    assert host[3] not in (0.0, max_dist)


# ------------------------------------------------------------------------------------------------- evaluators
SHAPE = (40, 36, 28)


def _blob(shape, centre, radius):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1)
    return (((g - np.asarray(centre)) ** 2).sum(-1) <= radius ** 2)


def _three_blobs(shift):
    """the 4-class maps of tests/test_eval_classes_gpu.py"""
    lab = np.zeros(SHAPE, np.int64)
    for c, (centre, radius) in enumerate((((12, 12, 10), 7), ((28, 22, 16), 6), ((14, 28, 20), 4)), 1):
        lab[_blob(SHAPE, tuple(v + shift for v in centre), radius)] = c
    return lab


def test_percase_device_surface():
    gt, pred = _three_blobs(0), _three_blobs(2)
    for c in (1, 2, 3):
        p, g = (pred == c).astype(np.uint8), (gt == c).astype(np.int64)
        host = T3.calculate_metric_percase(p, g)
        np.testing.assert_allclose(SE.calculate_metric_percase(p, g, device_surface=True), host, rtol=RTOL, atol=0)
        on_dev = SE.calculate_metric_percase(torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV), device_surface=True)
        np.testing.assert_allclose(on_dev, host, rtol=RTOL, atol=0)
        assert host[2] > 0 and host[3] > 0
    p = (pred == 1).astype(np.uint8)
    empty = np.zeros(SHAPE, np.uint8)
    assert SE.calculate_metric_percase(p, empty, device_surface=True) == SE.calculate_metric_percase(p, empty) == (0.0, 0.0, 0.0, 0.0)
    for flag in (False, True):
        with pytest.raises(RuntimeError, match="does not contain any binary object"):
            SE.calculate_metric_percase(empty, p, device_surface=flag)


def test_all_case_family_device_surface(tmp_path):
    """the `test_all_case` family of utils.surface_eval: flag off = the functions of utils/test_3d_patch.py, flag on = their values at
    rtol 1e-12; a 'network' of two blobs as in tests/test_eval_gpu.py"""
    shape = (40, 40, 32)
    big, small = _blob(shape, (14, 14, 14), 7), _blob(shape, (32, 32, 24), 3)
    image = (big | small).astype(np.float32) * 4.0 - 2.0          # logit +2 inside the blobs, -2 outside

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))     # test_single_case takes the device from the parameters

        def forward(self, x):
            return None, torch.cat([-x, x], 1)

    net = Net().to(DEV)
    kw = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    cases = [(image, big.astype(np.uint8)), (image, _blob(shape, (16, 14, 14), 7).astype(np.uint8))]
    host = T3.test_all_case(net, cases, 2, **kw)
    assert host[2] > 10.0 and host[3] > 0                        # the far blob dominates HD95
    np.testing.assert_array_equal(SE.test_all_case(net, cases, 2, **kw), host)
    (tmp_path / "pred").mkdir()
    got = SE.test_all_case(net, cases, 2, device_surface=True, test_save_path=str(tmp_path) + "/pred/", **kw)
    np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
    assert (tmp_path / "performance.txt").read_text().startswith("average metric is")
    for name, args in (("test_all_case_BraTS19", (net, cases, 2)), ("test_all_case_Pancreas", (net, cases, 2)),
                       ("test_all_case_ISLES22", (net, [(i, l.astype(np.float64)) for i, l in cases], 2))):
        ref = getattr(T3, name)(*args, nms=1, **kw)
        np.testing.assert_array_equal(getattr(SE, name)(*args, nms=1, **kw), ref)
        np.testing.assert_allclose(getattr(SE, name)(*args, nms=1, device_surface=True, **kw), ref, rtol=RTOL, atol=0)
        assert ref[2] > 0


def test_perclass_device_surface():
    gt, pred = _three_blobs(0), _three_blobs(2)
    host = EC.calculate_metric_perclass(pred, gt, 4)
    got = EC.calculate_metric_perclass(pred, gt, 4, device_surface=True)
    np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
    assert (host[:, 2:] > 0).all()
    on_dev = EC.calculate_metric_perclass(torch.from_numpy(pred).to(DEV).to(torch.uint8), torch.from_numpy(gt).to(DEV), 4,
                                          device_surface=True)
    np.testing.assert_array_equal(on_dev, got)
    gt, pred = _three_blobs(0), _three_blobs(1)
    pred[pred == 2] = 0                 # class 2: absent from the prediction
    gt[gt == 3] = 0                     # class 3: absent from the ground truth
    host = EC.calculate_metric_perclass(pred, gt, 5)          # class 4: absent from both
    got = EC.calculate_metric_perclass(pred, gt, 5, device_surface=True)
    np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
    assert got[0, 2] > 0 and got[1:].tolist() == [[0.0] * 4] * 3


def test_real_size_twice():
    """(2, 96, 96, 96): the same bits on both runs, and the host path's values"""
    shape = (96, 96, 96)
    a = np.stack([SR._blobs(shape, 5), SR._blobs(shape, 6)])
    b = np.stack([SR._blobs(shape, 7), SR._blobs(shape, 8)])
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    runs = []
    for _ in range(2):
        hist, nborder = surface.surface_hists(ta, tb)
        runs.append((hist, nborder, surface.surface_metrics(ta, tb)))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    hist, nborder, got = (t.cpu().numpy() for t in runs[0])
    assert hist.shape == (2, 2, 27076)
    for s in range(2):
        assert hist[s].sum(1).tolist() == nborder[s].tolist() == got[s, 3:].tolist()
        ref = [OE.hd95(a[s], b[s]), OE.asd(a[s], b[s]), OE.asd(b[s], a[s])]
        print(f"pair {s}: device {got[s, :3]!r} host {ref!r}")
        np.testing.assert_allclose(got[s, :3], ref, rtol=RTOL, atol=0)


def test_async_train_metrics_on_device():
    rng = np.random.default_rng(3)
    B, shape = 2, (12, 10, 8)
    max_dist = float(np.linalg.norm(shape))
    logits = torch.from_numpy(rng.standard_normal((B, 2) + shape).astype(np.float32)).to(DEV)
    label = torch.from_numpy(rng.integers(0, 2, (B,) + shape)).to(DEV)
    m = M.AsyncTrainMetrics(every=1, on_device=True)
    assert m._t is None and m._q is None                      # no worker thread, no queue
    m.update(0, logits, label)
    got = m.latest()
    assert got["iter"] == 0 and got["dice"].is_cuda
    it, hd = got["hd95"]
    assert it == 0 and hd.is_cuda and hd.dim() == 0 and hd.dtype == torch.float64
    ref = np.mean(M.compute_hd95(logits.argmax(1), label, max_dist))
    np.testing.assert_allclose(hd.item(), ref, rtol=RTOL, atol=0)
    m.update(1, logits, torch.zeros_like(label))              # empty labels: max_dist for every sample
    assert m.latest()["hd95"][0] == 1 and m.latest()["hd95"][1].item() == max_dist
    m.close()

    C = 3
    logits = torch.from_numpy(rng.standard_normal((B, C) + shape).astype(np.float32)).to(DEV)
    label = torch.from_numpy(rng.integers(0, C, (B,) + shape)).to(DEV)
    m = M.AsyncClassTrainMetrics(every=1, on_device=True)
    assert m._t is None and m._q is None
    m.update(4, logits, label)
    it, hd = m.latest()["hd95"]
    assert it == 4 and hd.is_cuda and hd.dim() == 0
    ref = np.mean(M.compute_hd95(logits.argmax(1) == 1, label == 1, max_dist))
    np.testing.assert_allclose(hd.item(), ref, rtol=RTOL, atol=0)
    assert m.latest()["dice"].shape == (B, C - 1)
    m.close()
    m = M.AsyncTrainMetrics(every=0, on_device=True)          # Dice only
    m.update(7, logits[:, :2], label)
    assert m.latest()["hd95"] is None


def test_refusals():
    z = torch.zeros((1, 4, 4, 513), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="1..512"):
        surface.surface_hists(z, z)
    a = torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device=DEV)
    nbins = SR.nbins_of((4, 5, 6))
    hist = torch.zeros((4, 2, nbins), dtype=torch.int32, device=DEV)
    nborder = torch.zeros((4, 2), dtype=torch.int32, device=DEV)
    ws = torch.empty(int(_lib.load().dycon_surface_workspace(4, 4, 5, 6)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(a_bytes=1, b_bytes=1, n_vol=2, cls_lo=0, n_cls=1, shape=(4, 5, 6), ws_bytes=ws.numel()):
        _lib.call("dycon_surface_hist", a.data_ptr(), a_bytes, a.data_ptr(), b_bytes, n_vol, cls_lo, n_cls, *shape, hist.data_ptr(),
                  nborder.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    call()
    call(cls_lo=1, n_cls=2)
    for bad, match in ((dict(b_bytes=4), "uint8 or int64"), (dict(a_bytes=8), "uint8"), (dict(cls_lo=0, n_cls=2), "class range"),
                       (dict(cls_lo=255, n_cls=2), "class range"), (dict(shape=(4, 5, 513)), "every axis"),
                       (dict(shape=(0, 5, 6)), "every axis"), (dict(cls_lo=1, n_cls=2, ws_bytes=ws.numel() - 1), "workspace")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            call(**bad)
    out = torch.empty((4, 5), dtype=torch.float64, device=DEV)
    with pytest.raises(_lib.DyconLibraryError, match="percentile"):
        _lib.call("dycon_surface_metrics", hist.data_ptr(), nborder.data_ptr(), 4, nbins, 101.0, out.data_ptr(), stream)
    torch.cuda.synchronize()
