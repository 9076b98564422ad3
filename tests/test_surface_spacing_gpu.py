"""Weighted surface distances on the MI355X (csrc/surface_spacing.hip, utils/surface.py): HD95 / ASD with a voxel spacing and a border
connectivity against the oracle's scipy path (`sampling=`, `generate_binary_structure`) at the tolerance tests/test_surface_gpu.py
holds the unit path to (rtol 1e-12, atol 0), border counts as integers, the same bits on every run, and the evaluators' spacing
arguments against their host forms."""
import functools

import numpy as np
import pytest
import torch

import surface_ref as SR
import surface_spacing_ref as SSR
from oracle import evaluate as OE

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import device_eval as DE
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import metrics as M
from dycon_paper_replication_amd.utils import surface
from dycon_paper_replication_amd.utils import surface_eval as SE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("blobs", "face", "corners", "full_vs_voxel", "identical", "plates")
RTOL = 1e-12
ANISO = (0.7, 0.7, 5.0)


@functools.lru_cache(maxsize=None)
def _cases(shape):
    return SR.cases(shape)


@functools.lru_cache(maxsize=None)
def _oracle(shape, name, spacing, conn):
    a, b = _cases(shape)[name]
    return (float(OE.hd95(a, b, spacing, conn)), float(OE.asd(a, b, spacing, conn)), float(OE.asd(b, a, spacing, conn)),
            int(SSR.border(a, conn).sum()), int(SSR.border(b, conn).sum()))


def _stack(shape, side, dtype=np.uint8):
    return torch.from_numpy(np.stack([_cases(shape)[n][side] for n in NAMES]).astype(dtype)).to(DEV)


def _check_against_oracle(shape, spacing, conn):
    got = surface.surface_metrics(_stack(shape, 0), _stack(shape, 1), voxelspacing=spacing, connectivity=conn)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (6, 5)
    got = got.cpu().numpy()
    for i, name in enumerate(NAMES):
        ref = _oracle(shape, name, spacing, conn)
        print(f"{shape} {name} spacing {spacing} conn {conn}: device {got[i].tolist()!r} - oracle = "
              f"{got[i, 0] - ref[0]:.3e}, {got[i, 1] - ref[1]:.3e}, {got[i, 2] - ref[2]:.3e}")
        np.testing.assert_allclose(got[i, :3], ref[:3], rtol=RTOL, atol=0)
        assert got[i, 3:].tolist() == list(ref[3:])


@pytest.mark.parametrize("spacing", [ANISO, (1.25, 0.3, 3.7), 2.0], ids=["aniso", "skew", "scalar2"])
@pytest.mark.parametrize("shape", SR.SHAPES)
def test_metrics_match_the_oracle(shape, spacing):
    """all six named cases in one call; each axis in turn is longer than 256, so every tile variant runs"""
    _check_against_oracle(shape, spacing, 1)


@pytest.mark.parametrize("conn", [2, 3])
@pytest.mark.parametrize("shape", [(17, 33, 70), (4, 300, 3)])
def test_connectivity_matches_the_oracle(shape, conn):
    _check_against_oracle(shape, ANISO, conn)
    _check_against_oracle(shape, None, conn)                  # connectivity alone also takes the weighted path


def test_anisotropy_changes_the_nearest_voxel():
    """the smallest input on which a transform that ignores the weights is wrong: (11, 8, 8) is 3 voxels = 15 away along x,
    (8, 8, 13) is 5 voxels = 5 away along z"""
    a, b = np.zeros((17, 17, 17), np.uint8), np.zeros((17, 17, 17), np.uint8)
    a[8, 8, 8] = 1
    b[11, 8, 8] = b[8, 8, 13] = 1
    assert surface.surface_metrics(a, b, voxelspacing=(5, 1, 1))[0, 1:].tolist() == [5.0, 10.0, 1.0, 2.0]      # b -> a: 15 and 5
    assert surface.surface_metrics(a, b, voxelspacing=None)[0, 1:].tolist() == [3.0, 4.0, 1.0, 2.0]
    assert surface.surface_metrics(a, b, voxelspacing=1)[0, 1:].tolist() == [3.0, 4.0, 1.0, 2.0]
    assert surface.surface_metrics(a, b, voxelspacing=(5, 1, 1), q=100.0)[0, 0].item() == 15.0


def test_unit_spacing_given_explicitly_and_the_default_path():
    shape = (24, 40, 72)
    a, b = _stack(shape, 0), _stack(shape, 1)
    today = surface.surface_metrics(a, b)
    assert torch.equal(today, surface.surface_metrics(a, b, voxelspacing=None, connectivity=1))      # the histogram path: bit-equal
    assert torch.equal(today, surface.surface_metrics(a, b, None, 95.0, None, 1))
    explicit = surface.surface_metrics(a, b, voxelspacing=(1.0, 1.0, 1.0), connectivity=1)
    np.testing.assert_allclose(explicit.cpu().numpy(), today.cpu().numpy(), rtol=RTOL, atol=0)
    assert torch.equal(explicit[:, 3:], today[:, 3:])
    from_numpy = surface.surface_metrics(a.cpu().numpy(), b.cpu().numpy(), voxelspacing=(1.0, 1.0, 1.0))      # numpy in: the same bits
    assert torch.equal(explicit, from_numpy)


@pytest.mark.parametrize("q", [0.0, 50.0, 77.5, 100.0])
def test_other_percentiles(q):
    a, b = _cases((17, 33, 70))["blobs"]
    both = np.hstack((OE.surface_distances(a, b, ANISO), OE.surface_distances(b, a, ANISO)))
    got = surface.surface_metrics(a, b, q=q, voxelspacing=ANISO)[0, 0].item()
    np.testing.assert_allclose(got, np.percentile(both, q), rtol=RTOL, atol=0)
    twin = surface.metrics_from_distances(*SSR.distances(a, b, ANISO), q)
    np.testing.assert_allclose(got, twin[0], rtol=RTOL, atol=0)


def test_empty_masks():
    shape = (17, 33, 70)
    m = _cases(shape)["blobs"][0]
    e = np.zeros(shape, bool)
    a, b = np.stack([e, m, e, m]), np.stack([m, e, e, m])
    got = surface.surface_metrics(a, b, voxelspacing=ANISO).cpu().numpy()
    nb = int(SR.border6(m).sum())
    assert np.isnan(got[:3, :3]).all()
    assert got[:3, 3:].tolist() == [[0, nb], [nb, 0], [0, 0]]
    assert got[3].tolist() == [0.0, 0.0, 0.0, nb, nb]
    max_dist = float(np.linalg.norm(shape))
    a[3] = _cases(shape)["blobs"][1]
    dev = M.compute_hd95_device(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), max_dist, voxelspacing=ANISO)
    assert dev.is_cuda and dev.dtype == torch.float64 and dev.shape == (4,)
    assert dev[:3].tolist() == [max_dist] * 3
    np.testing.assert_allclose(dev[3].item(), OE.hd95(a[3], b[3], ANISO), rtol=RTOL, atol=0)
    conn3 = M.compute_hd95_device(a, b, max_dist, connectivity=3)
    np.testing.assert_allclose(conn3[3].item(), OE.hd95(a[3], b[3], None, 3), rtol=RTOL, atol=0)


def _label_maps():
    """the 4-class maps of tests/test_surface_gpu.py::test_class_form_on_a_label_map"""
    shape = (24, 40, 72)
    maps = [np.minimum(sum(SR._blobs(shape, 100 * seed + j).astype(np.int64) for j in range(4)), 3) for seed in range(4)]
    pred, gt = np.stack(maps[:2]), np.stack(maps[2:])
    pred[1][pred[1] == 3] = 0                                 # class 3 absent from the prediction of volume 1
    return pred, gt


def test_class_form_on_a_label_map():
    pred, gt = _label_maps()
    rows = []
    for gt_t in (torch.from_numpy(gt).to(DEV), torch.from_numpy(gt.astype(np.uint8)).to(DEV)):
        got = surface.surface_metrics(torch.from_numpy(pred.astype(np.uint8)).to(DEV), gt_t, classes=(1, 3), voxelspacing=ANISO)
        assert got.shape == (6, 5)
        rows.append(got)
        got = got.cpu().numpy()
        for v in range(2):
            for k in range(3):
                p, g = pred[v] == 1 + k, gt[v] == 1 + k
                assert got[v * 3 + k, 3:].tolist() == [SR.border6(p).sum(), SR.border6(g).sum()]
                if not (p.any() and g.any()):
                    assert (v, k) == (1, 2) and np.isnan(got[5, :3]).all() and got[5, 3] == 0
                    continue
                ref = [OE.hd95(p, g, ANISO), OE.asd(p, g, ANISO), OE.asd(g, p, ANISO)]
                np.testing.assert_allclose(got[v * 3 + k, :3], ref, rtol=RTOL, atol=0)
    assert torch.equal(rows[0][:5], rows[1][:5])


def test_pairs_go_in_chunks_over_the_workspace_budget(monkeypatch):
    """6 volumes x 2 classes with room for 2 volumes per launch sequence: the same bits as in one piece"""
    shape = (17, 33, 70)
    a = torch.from_numpy(np.stack([_cases(shape)[n][0] for n in NAMES]).astype(np.uint8) * 2).to(DEV)
    b = torch.from_numpy(np.stack([_cases(shape)[n][1] for n in NAMES]).astype(np.int64) * 2).to(DEV)
    a[:, ::2], b[:, 1::3] = a[:, ::2] // 2, b[:, 1::3] // 2                       # label maps with the classes 1 and 2
    whole = surface.surface_metrics(a, b, classes=(1, 2), voxelspacing=ANISO, connectivity=2)
    monkeypatch.setattr(surface, "WORKSPACE_BUDGET", 2 * int(_lib.load().dycon_surface_spaced_workspace(2, *shape)) + 5)
    parts = surface.surface_metrics(a, b, classes=(1, 2), voxelspacing=ANISO, connectivity=2)
    assert whole.shape == (12, 5) and whole[:, 3:].sum().item() > 0 and not torch.isnan(whole).all()
    assert torch.equal(whole.view(torch.int64), parts.view(torch.int64))         # bits, NaN rows included


def test_real_size_twice():
    """(2, 96, 96, 96) at (0.7, 0.7, 5.0): the same bits on both runs, and the host path's values"""
    shape = (96, 96, 96)
    a = np.stack([SR._blobs(shape, 5), SR._blobs(shape, 6)])
    b = np.stack([SR._blobs(shape, 7), SR._blobs(shape, 8)])
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    runs = [surface.surface_metrics(ta, tb, voxelspacing=ANISO) for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    got = runs[0].cpu().numpy()
    for s in range(2):
        ref = [OE.hd95(a[s], b[s], ANISO), OE.asd(a[s], b[s], ANISO), OE.asd(b[s], a[s], ANISO)]
        print(f"pair {s}: device {got[s, :3]!r} host {ref!r}")
        np.testing.assert_allclose(got[s, :3], ref, rtol=RTOL, atol=0)
        assert got[s, 3:].tolist() == [SR.border6(a[s]).sum(), SR.border6(b[s]).sum()]


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


def test_percase_with_a_spacing():
    gt, pred = _three_blobs(0), _three_blobs(2)
    p, g = (pred == 1).astype(np.uint8), (gt == 1).astype(np.int64)
    unit = SE.calculate_metric_percase(p, g)
    for spacing, conn in ((ANISO, 1), (2.0, 1), (ANISO, 3), (None, 2)):
        host = SE.calculate_metric_percase(p, g, voxelspacing=spacing, connectivity=conn)
        assert host[:2] == unit[:2]
        np.testing.assert_allclose(host[2:], [OE.hd95(p, g, spacing, conn), OE.asd(p, g, spacing, conn)], rtol=RTOL, atol=0)
        got = SE.calculate_metric_percase(p, g, device_surface=True, voxelspacing=spacing, connectivity=conn)
        np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
        on_dev = SE.calculate_metric_percase(torch.from_numpy(p).to(DEV), torch.from_numpy(g).to(DEV), device_surface=True,
                                             voxelspacing=spacing, connectivity=conn)
        assert on_dev == got
    assert SE.calculate_metric_percase(p, g, voxelspacing=ANISO)[2] != unit[2]           # the host branch no longer ignores it
    empty = np.zeros(SHAPE, np.uint8)
    for flag in (False, True):
        assert SE.calculate_metric_percase(p, empty, device_surface=flag, voxelspacing=ANISO) == (0.0, 0.0, 0.0, 0.0)
        with pytest.raises(RuntimeError, match="does not contain any binary object"):
            SE.calculate_metric_percase(empty, p, device_surface=flag, voxelspacing=ANISO)


def test_perclass_with_a_spacing():
    gt, pred = _three_blobs(0), _three_blobs(2)
    unit = EC.calculate_metric_perclass(pred, gt, 4)
    for spacing, conn in ((ANISO, 1), (ANISO, 2)):
        host = EC.calculate_metric_perclass(pred, gt, 4, voxelspacing=spacing, connectivity=conn)
        got = EC.calculate_metric_perclass(pred, gt, 4, device_surface=True, voxelspacing=spacing, connectivity=conn)
        np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
        np.testing.assert_array_equal(host[:, :2], unit[:, :2])
        for c in (1, 2, 3):
            np.testing.assert_allclose(host[c - 1, 2], OE.hd95(pred == c, gt == c, spacing, conn), rtol=RTOL, atol=0)
        assert (host[:, 2] != unit[:, 2]).all()
    gt, pred = _three_blobs(0), _three_blobs(1)
    pred[pred == 2] = 0                 # class 2: absent from the prediction
    gt[gt == 3] = 0                     # class 3: absent from the ground truth
    host = EC.calculate_metric_perclass(pred, gt, 5, voxelspacing=ANISO)
    got = EC.calculate_metric_perclass(pred, gt, 5, device_surface=True, voxelspacing=ANISO)
    np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
    assert got[0, 2] > 0 and got[1:].tolist() == [[0.0] * 4] * 3


def test_all_case_classes_with_a_spacing():
    """the one-hot 'network' of tests/test_eval_classes_gpu.py::test_all_case_classes: the prediction is the image's label map"""
    pred, gt = _three_blobs(0), _three_blobs(2)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return None, torch.cat([4.0 * (x == c).float() for c in range(4)], 1)

    net = Net().to(DEV)
    kw = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    image = pred.astype(np.float32)
    ref = EC.calculate_metric_perclass(pred, gt, 4, voxelspacing=ANISO, connectivity=2)            # host scipy with the spacing
    for flag in (False, True):
        got = EC.test_all_case_classes(net, [(image, gt)], 4, device_surface=flag, voxelspacing=ANISO, connectivity=2, **kw)
        np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0)
        own = EC.test_all_case_classes(net, [(image, gt, ANISO)], 4, device_surface=flag, voxelspacing=2.0, connectivity=2, **kw)
        np.testing.assert_allclose(own, ref, rtol=RTOL, atol=0)                                   # the case's spacing wins
    assert (ref[:, 2] != EC.test_all_case_classes(net, [(image, gt)], 4, **kw)[:, 2]).all()


def test_all_case_family_with_a_spacing(tmp_path):
    """the two-blob 'network' of tests/test_surface_gpu.py::test_all_case_family_device_surface with a spacing: device against host,
    a case's own spacing against the call's"""
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
    labels = [big.astype(np.uint8), _blob(shape, (16, 14, 14), 7).astype(np.uint8)]
    cases = [(image, lab) for lab in labels]
    unit = SE.test_all_case(net, cases, 2, **kw)
    host = SE.test_all_case(net, cases, 2, voxelspacing=ANISO, **kw)
    assert host[:2].tolist() == unit[:2].tolist() and host[2] != unit[2] and unit[2] > 10.0
    (tmp_path / "pred").mkdir()
    got = SE.test_all_case(net, cases, 2, device_surface=True, voxelspacing=ANISO, test_save_path=str(tmp_path) + "/pred/", **kw)
    np.testing.assert_allclose(got, host, rtol=RTOL, atol=0)
    assert (tmp_path / "performance.txt").read_text().startswith("average metric is")
    carried = [(image, lab, ANISO) for lab in labels]             # device_eval keeps test_3d_patch's parameter lists: the case carries it
    np.testing.assert_allclose(DE.test_all_case(net, carried, 2, **kw), host, rtol=RTOL, atol=0)
    np.testing.assert_allclose(DE.test_all_case_Pancreas(net, carried, 2, nms=1, **kw),
                               SE.test_all_case_Pancreas(net, cases, 2, nms=1, voxelspacing=ANISO, **kw), rtol=RTOL, atol=0)
    np.testing.assert_allclose(DE.test_all_case(net, cases, 2, **kw), unit, rtol=RTOL, atol=0)       # two-element cases: as before
    np.testing.assert_allclose(SE.test_all_case_ISLES22(net, [(i, l.astype(np.float64)) for i, l in cases], 2, device_surface=True,
                                                        voxelspacing=ANISO, **kw), host, rtol=RTOL, atol=0)
    # a case's own spacing replaces the call's: one case at (2, 2, 2), one at the call's
    mixed = [(image, labels[0], (2.0, 2.0, 2.0)), (image, labels[1])]
    each = [SE.test_all_case(net, [cases[0]], 2, device_surface=True, voxelspacing=2.0, **kw),
            SE.test_all_case(net, [cases[1]], 2, device_surface=True, voxelspacing=ANISO, **kw)]
    for fn, extra in ((SE.test_all_case, dict(device_surface=True)), (SE.test_all_case, {}),
                      (SE.test_all_case_BraTS19, dict(device_surface=True))):
        np.testing.assert_allclose(fn(net, mixed, 2, voxelspacing=ANISO, **extra, **kw), (each[0] + each[1]) / 2, rtol=RTOL, atol=0)
    np.testing.assert_allclose(SE.test_all_case(net, [mixed[0]], 2, **kw), each[0], rtol=RTOL, atol=0)      # no spacing in the call
    np.testing.assert_allclose(DE.test_all_case(net, [mixed[0]], 2, **kw), each[0], rtol=RTOL, atol=0)


def test_refusals():
    a = torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device=DEV)
    out = torch.empty((4, 5), dtype=torch.float64, device=DEV)
    need = int(_lib.load().dycon_surface_spaced_workspace(4, 4, 5, 6))
    ws = torch.empty(need // 8, dtype=torch.float64, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    import ctypes

    def call(a_bytes=1, b_bytes=1, n_vol=2, cls_lo=0, n_cls=1, shape=(4, 5, 6), spacing=(0.7, 0.7, 5.0), conn=1, q=95.0, ws_bytes=need):
        _lib.call("dycon_surface_spaced_metrics", a.data_ptr(), a_bytes, a.data_ptr(), b_bytes, n_vol, cls_lo, n_cls, *shape,
                  (ctypes.c_double * 3)(*spacing), conn, q, out.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    call()
    call(cls_lo=1, n_cls=2, conn=3)
    nan, inf = float("nan"), float("inf")
    for bad, match in ((dict(spacing=(0.7, 0.0, 5.0)), "spacing"), (dict(spacing=(-1.0, 1.0, 1.0)), "spacing"),
                       (dict(spacing=(1.0, 1.0, nan)), "spacing"), (dict(spacing=(inf, 1.0, 1.0)), "spacing"),
                       (dict(spacing=(1.0, 1e-200, 1.0)), "spacing"), (dict(conn=0), "connectivity"), (dict(conn=4), "connectivity"),
                       (dict(q=-0.5), "percentile"), (dict(q=100.5), "percentile"), (dict(q=nan), "percentile"),
                       (dict(b_bytes=4), "uint8 or int64"), (dict(a_bytes=8), "uint8"), (dict(cls_lo=0, n_cls=2), "class range"),
                       (dict(shape=(4, 5, 513)), "every axis"), (dict(shape=(0, 5, 6)), "every axis"),
                       (dict(cls_lo=1, n_cls=2, ws_bytes=need - 1), "workspace")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            call(**bad)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()[:, :3]).all() and out[:, 3:].sum().item() == 0          # all-zero volumes: NaN rows
