"""Connected components on the MI355X (csrc/components.hip, utils/components.py): roots, labels, component counts and the largest
component against scipy.ndimage bit for bit (tests/components_ref.py), and the device-resident evaluators built on them against
the host paths they replace.  Every comparison is on integers and exact, but for the metrics held to utils/test_3d_patch.py at the
rtol 1e-12 of tests/test_surface_gpu.py (the fp64 summation order of the surface means is the only difference)."""
import functools

import numpy as np
import pytest
import torch

import components_ref as CR

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import components as CC
from dycon_paper_replication_amd.utils import device_eval as DE
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import sliding_window as SW
from dycon_paper_replication_amd.utils import surface_eval as SE
from dycon_paper_replication_amd.utils import test_3d_patch as T3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12


@functools.lru_cache(maxsize=None)
def _oracle(key, connectivity):
    """(labels (n, X, Y, Z) int32, ncomp (n,), roots) of a batch built once per (input, connectivity)"""
    vols = _input(key)
    per = [CR.label(v, connectivity) for v in vols]
    return (np.stack([p[0] for p in per]), np.array([p[1] for p in per], np.int32),
            np.stack([CR.roots(*p) for p in per]))


@functools.lru_cache(maxsize=None)
def _input(key):
    kind, shape, arg = key
    if kind == "random":
        return np.stack([CR.random_mask(shape, arg, 100 * i + shape[0]) for i in range(3)])
    if kind == "named":
        return np.stack([CR.named(shape)[n] for n in arg])
    if kind == "blobs":
        return np.stack([_blobs_speckle(shape, arg + i) for i in range(2)])
    raise KeyError(kind)


def _blobs_speckle(shape, seed):
    """smoothed-noise blobs (the top 12 %) plus 1 % speckle"""
    from scipy import ndimage
    rng = np.random.default_rng(seed)
    x = ndimage.gaussian_filter(rng.standard_normal(shape), 3.0, mode="nearest")
    return ((x >= np.quantile(x, 0.88)) | (rng.random(shape) < 0.01)).astype(np.uint8)


def _check_against_oracle(key, connectivity, dtype=np.uint8):
    vols = _input(key)
    ref_labels, ref_n, ref_roots = _oracle(key, connectivity)
    t = torch.from_numpy(vols.astype(dtype) * (7 if dtype == np.int64 else 1)).to(DEV)       # binary: any non-zero value
    root = CC.component_roots(t, connectivity)
    labels, ncomp = CC.label_components(t, connectivity)
    assert root.is_cuda and root.dtype == torch.int32 and root.shape == t.shape
    assert labels.is_cuda and labels.dtype == torch.int32 and labels.shape == t.shape
    assert ncomp.dtype == torch.int32 and ncomp.shape == (len(vols),)
    print(f"{key} connectivity {connectivity}: components per volume {ref_n.tolist()}")
    np.testing.assert_array_equal(ncomp.cpu().numpy(), ref_n)
    np.testing.assert_array_equal(root.cpu().numpy(), ref_roots)
    np.testing.assert_array_equal(labels.cpu().numpy(), ref_labels)


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("density", [0.12, 0.35])
@pytest.mark.parametrize("shape", CR.SHAPES)
def test_random_masks_equal_scipy(shape, density, connectivity, dtype):
    """3 volumes per call: roots, labels and component counts"""
    _check_against_oracle(("random", shape, density), connectivity, dtype)


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("names", [tuple(CR.NAMES[:5]), tuple(CR.NAMES[5:])], ids=["first5", "last5"])
@pytest.mark.parametrize("shape", CR.SHAPES)
def test_named_cases_equal_scipy(shape, names, connectivity):
    """5 named volumes per call, so no volume may leak into the next: the corner case, whose last voxel is set, is followed by the
    frame, whose first voxel is set"""
    _check_against_oracle(("named", shape, names), connectivity)


def test_named_largest():
    shape = CR.SHAPES[0]
    cases = CR.named(shape)
    names = ["two_cubes", "empty", "corner", "faces", "frame", "serpentine"]
    t = torch.from_numpy(np.stack([cases[n] for n in names])).to(DEV)
    for connectivity in (1, 3):
        mask, size = CC.largest_component(t, connectivity, return_size=True)
        ref = [CR.largest(cases[n], connectivity) for n in names]
        np.testing.assert_array_equal(mask.cpu().numpy(), np.stack([r[0] for r in ref]))
        assert size.tolist() == [r[1] for r in ref]
    assert size.tolist()[:3] == [27, 0, 1]
    assert mask[0, 1, 1, 2] == 1 and mask[0, -2, -2, -3] == 0          # equal cubes: the earlier in raster order wins
    assert mask[3, :, :, 0].all() and not mask[3, :, :, -1].any()      # two equal faces likewise, and they do not touch


def test_one_96_cube_case():
    _check_against_oracle(("blobs", (96, 96, 96), 40), 3)


def test_by_value_equals_the_per_value_oracle():
    rng = np.random.default_rng(5)
    shape = CR.SHAPES[0]
    vols = np.stack([rng.integers(0, 4, shape) * (rng.random(shape) < 0.5), rng.integers(0, 3, shape)]).astype(np.int64)
    vols[0, 0, 0, :3] = (300, 300, -1)                        # outside 1..255: background
    for connectivity in (1, 2, 3):
        ref = [CR.label_by_value(v, connectivity) for v in vols]
        for dtype in (np.int64, np.uint8):
            v = vols.copy()
            if dtype == np.uint8:
                v[0, 0, 0, :3] = 0
            t = torch.from_numpy(v.astype(dtype)).to(DEV)
            labels, ncomp = CC.label_components(t, connectivity, by_value=True)
            root = CC.component_roots(t, connectivity, by_value=True)
            assert ncomp.tolist() == [r[1] for r in ref]
            np.testing.assert_array_equal(labels.cpu().numpy(), np.stack([r[0] for r in ref]))
            np.testing.assert_array_equal(root.cpu().numpy(), np.stack([r[2] for r in ref]))


def test_largest_component_equals_getLargestCC():
    """blobs plus speckle, a batch of 3 with one empty volume; numpy input gives the same bits as tensor input"""
    shape = CR.SHAPES[1]
    vols = np.stack([_blobs_speckle(shape, 1), np.zeros(shape, np.uint8), _blobs_speckle(shape, 2)])
    t = torch.from_numpy(vols).to(DEV)
    mask, size = CC.largest_component(t, return_size=True)
    assert mask.is_cuda and mask.dtype == torch.uint8 and mask.shape == t.shape and size.dtype == torch.int32
    for i, v in enumerate(vols):
        host = T3.getLargestCC(v)
        np.testing.assert_array_equal(mask[i].cpu().numpy(), np.asarray(host).astype(np.uint8))
        labels, n = CR.label(v, 3)
        assert size[i].item() == (np.bincount(labels.ravel())[1:].max() if n else 0)
        assert mask[i].sum().item() == size[i].item()
    assert size[1].item() == 0 and 0 < size[0].item() < vols[0].sum()
    assert torch.equal(CC.largest_component(vols), mask)
    assert torch.equal(CC.largest_component(vols[0]), mask[0])                       # (X, Y, Z) in, (X, Y, Z) out
    assert torch.equal(CC.largest_component(t.to(torch.int64) * 3), mask)
    assert torch.equal(CC.largest_component(t.bool()), mask)
    assert torch.equal(CC.label_components(vols)[0], CC.label_components(t)[0])
    assert torch.equal(CC.component_roots(vols, 1), CC.component_roots(t, 1))


def _class_map(shape, seed):
    """a 4-class map (values 0, 1, 3; class 2 absent): several components per class"""
    rng = np.random.default_rng(seed)
    return (_blobs_speckle(shape, seed) * rng.choice([1, 3], size=shape)).astype(np.uint8)


def test_largest_component_per_class():
    shape = CR.SHAPES[1]
    vols = np.stack([_class_map(shape, 3), _class_map(shape, 4)])
    ref = np.stack([CR.largest_per_class(v, 4) for v in vols])
    assert (ref == 1).any() and (ref == 3).any() and not (ref == 2).any() and (ref != vols).any()
    for arg in (vols, torch.from_numpy(vols).to(DEV), torch.from_numpy(vols.astype(np.int64)).to(DEV)):
        got = CC.largest_component_per_class(arg, 4)
        assert got.is_cuda and got.dtype == torch.uint8
        np.testing.assert_array_equal(got.cpu().numpy(), ref)
    only1 = CC.largest_component_per_class(vols, 2).cpu().numpy()          # value 3 lies outside 1..num_classes-1
    np.testing.assert_array_equal(only1, np.where(ref == 1, 1, 0))


def test_real_size_twice():
    """(2, 96, 96, 96): the same bits on both runs, and the oracle's"""
    key = ("blobs", (96, 96, 96), 50)
    t = torch.from_numpy(_input(key)).to(DEV)
    runs = []
    for _ in range(2):
        labels, ncomp = CC.label_components(t)
        mask, size = CC.largest_component(t, return_size=True)
        runs.append((CC.component_roots(t), labels, ncomp, mask, size))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    ref_labels, ref_n, ref_roots = _oracle(key, 3)
    root, labels, ncomp, mask, size = (x.cpu().numpy() for x in runs[0])
    np.testing.assert_array_equal(root, ref_roots)
    np.testing.assert_array_equal(labels, ref_labels)
    np.testing.assert_array_equal(ncomp, ref_n)
    ref = [CR.largest(v, 3) for v in _input(key)]
    np.testing.assert_array_equal(mask, np.stack([r[0] for r in ref]))
    assert size.tolist() == [r[1] for r in ref]


def test_chunks_under_the_workspace_budget(monkeypatch):
    shape = CR.SHAPES[2]
    vols = np.stack([CR.random_mask(shape, 0.3, i) * (1 + i % 3) for i in range(6)]).astype(np.uint8)
    t = torch.from_numpy(vols).to(DEV)
    whole = (CC.label_components(t, 2), CC.largest_component(t, 2, return_size=True), CC.largest_component_per_class(t, 4, 1))
    per_vol = int(_lib.load().dycon_cc_workspace(1, *shape)) + 4 * int(np.prod(shape))
    monkeypatch.setattr(CC, "WORKSPACE_BUDGET", 2 * per_vol + per_vol // 2)
    pieces, _ = CC._pieces(t)
    assert pieces == [(0, 2), (2, 2), (4, 2)]
    parts = (CC.label_components(t, 2), CC.largest_component(t, 2, return_size=True), CC.largest_component_per_class(t, 4, 1))
    for a, b in zip(whole[0] + whole[1] + (whole[2],), parts[0] + parts[1] + (parts[2],)):
        assert torch.equal(a, b)
    np.testing.assert_array_equal(parts[0][1].cpu().numpy(), [CR.label(v, 2)[1] for v in vols])


# ------------------------------------------------------------------ the device-resident evaluators
def _blob(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2


class _TwoBlobNet(torch.nn.Module):
    """the two-blob 'network' of tests/test_surface_gpu.py::test_all_case_family_device_surface: the image holds the logit"""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))         # the evaluators take the device from the parameters

    def forward(self, x):
        return None, torch.cat([-x, x], 1)


def _two_blob_cases():
    shape = (40, 40, 32)
    big, small = _blob(shape, (14, 14, 14), 7), _blob(shape, (32, 32, 24), 3)
    image = (big | small).astype(np.float32) * 4.0 - 2.0          # logit +2 inside the blobs, -2 outside
    cases = [(image, big.astype(np.uint8)), (image, _blob(shape, (16, 14, 14), 7).astype(np.uint8))]
    return image, cases, dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)


def test_single_case_device_equals_test_single_case():
    image, _, kw = _two_blob_cases()
    net = _TwoBlobNet().to(DEV)
    label, prob = SW.single_case_device(net, image, kw["stride_xy"], kw["stride_z"], kw["patch_size"])
    assert label.is_cuda and label.dtype == torch.uint8 and prob.is_cuda and prob.dtype == torch.float32
    host_label, host_score = SW.test_single_case(net, image, kw["stride_xy"], kw["stride_z"], kw["patch_size"], num_classes=2)
    np.testing.assert_array_equal(label.cpu().numpy().astype(np.int64), host_label)
    np.testing.assert_array_equal(prob.cpu().numpy(), host_score[1])
    small = image[:30, :28, :12]                                   # smaller than the window on every axis: padded and cropped
    label, prob = SW.single_case_device(net, torch.from_numpy(small).to(DEV), 8, 8, kw["patch_size"])
    host_label, host_score = SW.test_single_case(net, small, 8, 8, kw["patch_size"], num_classes=1)
    assert label.shape == small.shape
    np.testing.assert_array_equal(label.cpu().numpy().astype(np.int64), host_label)
    np.testing.assert_array_equal(prob.cpu().numpy(), host_score[0])


def test_device_eval_family_with_nms(tmp_path):
    _, cases, kw = _two_blob_cases()
    net = _TwoBlobNet().to(DEV)
    (tmp_path / "pred").mkdir()
    got = DE.test_all_case(net, cases, 2, nms=1, test_save_path=str(tmp_path) + "/pred/", **kw)
    assert (tmp_path / "performance.txt").read_text().startswith("average metric is")
    np.testing.assert_array_equal(got, SE.test_all_case(net, cases, 2, nms=1, device_surface=True, **kw))
    np.testing.assert_allclose(got, T3.test_all_case(net, cases, 2, nms=1, **kw), rtol=RTOL, atol=0)
    plain = DE.test_all_case(net, cases, 2, **kw)
    np.testing.assert_array_equal(plain, SE.test_all_case(net, cases, 2, device_surface=True, **kw))
    assert got[0] > plain[0] and got[2] < plain[2]              # the small blob is gone: Dice up, HD95 down
    for name, args in (("test_all_case_BraTS19", (net, cases, 2)), ("test_all_case_Pancreas", (net, cases, 2)),
                       ("test_all_case_ISLES22", (net, [(i, l.astype(np.float64)) for i, l in cases], 2))):
        ref = getattr(SE, name)(*args, nms=1, device_surface=True, **kw)
        np.testing.assert_array_equal(getattr(DE, name)(*args, nms=1, **kw), ref)
        np.testing.assert_allclose(ref, getattr(T3, name)(*args, nms=1, **kw), rtol=RTOL, atol=0)
        np.testing.assert_array_equal(getattr(DE, name)(*args, **kw), plain)
    empty = [(np.full_like(cases[0][0], -2.0), cases[0][1])]     # nothing predicted: (0, 0, 0, 0), as the host loop
    for nms in (0, 1):
        assert DE.test_all_case(net, empty, 2, nms=nms, **kw).tolist() == T3.test_all_case(net, empty, 2, nms=nms, **kw).tolist() == [0.0] * 4


def test_all_case_classes_with_nms():
    """the per-class extension: the prediction through the host per-class selection first gives the same metrics"""
    shape = (40, 40, 32)
    gt = np.zeros(shape, np.int64)
    for c, centre in ((1, (10, 10, 10)), (2, (28, 12, 20)), (3, (14, 30, 16))):
        gt[_blob(shape, centre, 5)] = c
    image = gt.copy()
    image[_blob(shape, (34, 34, 27), 2)] = 1                      # a second, smaller component of class 1
    image[_blob(shape, (5, 34, 5), 2)] = 3                        # and of class 3

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):                                      # the image holds the label: one-hot logits
            return None, torch.cat([4.0 * (x == c).float() for c in range(4)], 1)

    net = Net().to(DEV)
    kw = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    cases = [(image.astype(np.float32), gt)]
    plain = EC.test_all_case_classes(net, cases, 4, **kw)
    for device_surface in (False, True):
        got = EC.test_all_case_classes(net, cases, 4, nms=1, device_surface=device_surface, **kw)
        ref = EC.calculate_metric_perclass(CR.largest_per_class(image, 4), gt, 4, device_surface=device_surface)
        np.testing.assert_array_equal(got, ref)
    assert np.array_equal(got[:, :2], [[1.0, 1.0]] * 3) and plain[0, 0] < 1 and plain[2, 0] < 1 and plain[1, 0] == 1


def test_refusals():
    z5 = torch.zeros((1, 1, 4, 4, 4), dtype=torch.uint8, device=DEV)
    wide = torch.zeros((1, 4, 4, 513), dtype=torch.uint8, device=DEV)
    ok = torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device=DEV)
    for f in (CC.component_roots, CC.label_components, CC.largest_component, lambda v, *a: CC.largest_component_per_class(v, 3, *a)):
        with pytest.raises(ValueError, match=r"\(X, Y, Z\) or \(n_vol, X, Y, Z\)"):
            f(z5)
        with pytest.raises(ValueError, match=r"\(X, Y, Z\) or \(n_vol, X, Y, Z\)"):
            f(np.zeros((4, 4), np.uint8))
        with pytest.raises(ValueError, match="1..512"):
            f(wide)
        for bad in (0, 4, 1.5):
            with pytest.raises(ValueError, match="connectivity"):
                f(ok, bad)
        with pytest.raises(ValueError, match="CUDA tensor"):      # a tensor on another device than the kernels': numpy or CUDA only
            f(ok.cpu())
    with pytest.raises(ValueError, match="num_classes"):
        CC.largest_component_per_class(ok, 1)
    net = _TwoBlobNet()                                            # model on the CPU, or sent there: the evaluator refuses
    with pytest.raises(RuntimeError, match="MI355X only"):
        SW.single_case_device(net, np.zeros((8, 8, 8), np.float32), 4, 4, (8, 8, 8))
    with pytest.raises(RuntimeError, match="MI355X only"):
        SW.single_case_device(net.to(DEV), np.zeros((8, 8, 8), np.float32), 4, 4, (8, 8, 8), device="cpu")

    root = torch.zeros(ok.shape, dtype=torch.int32, device=DEV)
    out = torch.zeros_like(ok)
    two, win = (torch.zeros((2, 3), dtype=torch.int32, device=DEV) for _ in range(2))
    ws = torch.empty(int(_lib.load().dycon_cc_workspace(2, 4, 5, 6)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def roots(vol_bytes=1, n_vol=2, shape=(4, 5, 6), connectivity=3):
        _lib.call("dycon_cc_roots", ok.data_ptr(), vol_bytes, n_vol, *shape, connectivity, 0, root.data_ptr(), stream)

    def largest(vol_bytes=1, shape=(4, 5, 6), n_cls=3, ws_bytes=ws.numel()):
        _lib.call("dycon_cc_largest", ok.data_ptr(), vol_bytes, root.data_ptr(), 2, *shape, n_cls, out.data_ptr(), two.data_ptr(),
                  win.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    roots()
    largest()
    for bad, match in ((dict(vol_bytes=4), "uint8 or int64"), (dict(shape=(4, 5, 513)), "every axis"), (dict(shape=(0, 5, 6)), "every axis"),
                       (dict(n_vol=0), "every axis"), (dict(connectivity=4), "connectivity"), (dict(connectivity=0), "connectivity")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            roots(**bad)
    for bad, match in ((dict(vol_bytes=2), "uint8 or int64"), (dict(n_cls=256), "n_cls"), (dict(n_cls=-1), "n_cls"),
                       (dict(ws_bytes=ws.numel() - 1), "workspace"), (dict(shape=(4, 513, 6)), "every axis")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            largest(**bad)
    with pytest.raises(_lib.DyconLibraryError, match="workspace"):
        _lib.call("dycon_cc_labels", root.data_ptr(), 2, 4, 5, 6, root.data_ptr(), two.data_ptr(), ws.data_ptr(), 16, stream)
    assert _lib.load().dycon_cc_workspace(1, 4, 5, 513) == 0
    torch.cuda.synchronize()
