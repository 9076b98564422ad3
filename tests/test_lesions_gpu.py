"""Lesion statistics and the ISLES22 test protocol on the MI355X (csrc/lesions.hip, utils/lesions.py, utils/isles_eval.py) against
scipy (tests/lesion_ref.py).  Counts and tables are integers and compared exactly.  Scores made of counts are the same fp64 formula
on the same integers and held to rtol 1e-12, the bound of tests/test_surface_gpu.py; HD95 and ASD are held to the host path at that
same bound.  The shapes are the smallest at which the kernels can go wrong: a row longer than a wave, volumes that are no multiple of
64 voxels, one lesion that takes every atomic, 64 distinct roots in a wave, several volumes in one call."""
import functools

import numpy as np
import pytest
import torch

import lesion_ref as LR

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import components as CC
from dycon_paper_replication_amd.utils import isles_eval as IE
from dycon_paper_replication_amd.utils import lesions as LS
from dycon_paper_replication_amd.utils import surface_eval as SE

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12
SHAPE = (17, 13, 70)                                  # odd sizes, one axis longer than a wave, 15470 voxels: no multiple of 64
F = {name: k for k, name in enumerate(LS.COUNT_FIELDS)}


def _dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype) * (5 if dtype == np.int64 else 1)).to(DEV)     # any non-zero value


def _assert_pair(pred, gt, connectivity, min_voxels, tables=True):
    """one (X, Y, Z) pair: counts and both tables against the reference"""
    ref = LR.counts(pred, gt, connectivity, min_voxels)
    got = LS.lesion_counts(_dev(pred), _dev(gt), connectivity, min_voxels)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (8,)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    if tables:
        for of in ("gt", "pred"):
            t = LS.lesion_table(_dev(pred), _dev(gt), of, connectivity, min_voxels)
            assert t.dtype == np.int64 and t.ndim == 2 and t.shape[1] == 3
            np.testing.assert_array_equal(t, LR.table(pred, gt, of, connectivity, min_voxels))
    return ref


@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("name", sorted(LR.HAND))
def test_hand_made_cases(name, connectivity):
    pred, gt = LR.HAND[name]
    ref = _assert_pair(pred, gt, connectivity, 1)
    _assert_pair(pred, gt, connectivity, 2)
    if name == "checker_opposite":                    # 64 distinct roots in a wave at connectivity 1; 210 voxels, 105 of background
        assert ref.tolist() == ([105, 105, 0, 105, 105, 105, 105, 0] if connectivity == 1 else [1, 1, 0, 1, 1, 105, 105, 0])
    if name == "checker_same" and connectivity == 1:
        assert ref.tolist() == [105, 105, 105, 0, 0, 105, 105, 105]
    if name == "cubes":
        assert ref.tolist() == [2, 2, 2, 0, 0, 28, 28, 2]
        assert LS.lesion_counts(pred, gt, connectivity, 2).tolist() == [1, 1, 0, 1, 1, 27, 27, 0]     # the filter turns a hit into a miss
    if name == "touching":
        assert ref.tolist() == [1, 1, 0, 1, 1, 1, 1, 0]


def test_one_lesion_takes_every_atomic():
    ones = np.ones((24, 20, 33), np.uint8)
    for connectivity in (1, 3):
        ref = _assert_pair(ones, ones, connectivity, 1)
        assert ref.tolist() == [1, 1, 1, 0, 0, 15840, 15840, 15840]
    assert LS.lesion_table(ones, ones, "pred").tolist() == [[1, 15840, 15840]]
    assert LS.lesion_counts(ones, ones, min_voxels=15841).tolist() == [0] * 8                          # and the filter removes it whole


@functools.lru_cache(maxsize=None)
def _random(density):
    """three independent (pred, gt) pairs"""
    pairs = [LR.random_pair(SHAPE, density, seed) for seed in range(3)]
    return np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])


@functools.lru_cache(maxsize=None)
def _random_ref(density, connectivity, min_voxels):
    pred, gt = _random(density)
    return np.stack([LR.counts(p, g, connectivity, min_voxels) for p, g in zip(pred, gt)])


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
@pytest.mark.parametrize("min_voxels", [1, 3])
@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("density", [0.02, 0.3, 0.6])
def test_random_masks_equal_scipy(density, connectivity, min_voxels, dtype):
    """three volumes in one call, then one call per volume"""
    pred, gt = _random(density)
    ref = _random_ref(density, connectivity, min_voxels)
    print(f"density {density} connectivity {connectivity} min_voxels {min_voxels}: tp/fn/fp per volume "
          f"{ref[:, [F['tp'], F['fn'], F['fp']]].tolist()}")
    if (density, connectivity, min_voxels) == (0.3, 1, 1):          # no agreement on trivial cases: every detection count is in play
        assert (ref[:, [F["tp"], F["fn"], F["fp"]]] > 0).all()
    tp, tg = _dev(pred, dtype), _dev(gt, dtype)
    got = LS.lesion_counts(tp, tg, connectivity, min_voxels)
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == (3, 8)
    np.testing.assert_array_equal(got.cpu().numpy(), ref)
    for v in range(3):
        np.testing.assert_array_equal(LS.lesion_counts(tp[v], tg[v], connectivity, min_voxels).cpu().numpy(), ref[v])


@pytest.mark.parametrize("min_voxels", [1, 3])
@pytest.mark.parametrize("connectivity", [1, 3])
@pytest.mark.parametrize("density", [0.02, 0.3])
def test_lesion_tables_equal_scipy(density, connectivity, min_voxels):
    """from hundreds of lesions per volume (density 0.3, 6 neighbours) down to one (26 neighbours) and none (density 0.02 under the
    size filter)"""
    pred, gt = _random(density)
    for of in ("gt", "pred"):
        tables = LS.lesion_table(_dev(pred), _dev(gt), of, connectivity, min_voxels)
        assert isinstance(tables, list) and len(tables) == 3
        for v, t in enumerate(tables):
            ref = LR.table(pred[v], gt[v], of, connectivity, min_voxels)
            if (density, connectivity) == (0.3, 1):
                assert len(ref) > 100
            np.testing.assert_array_equal(t, ref)
    one = LS.lesion_table(pred[1], gt[1], "gt", connectivity, min_voxels)             # (X, Y, Z) in: one array out
    np.testing.assert_array_equal(one, LR.table(pred[1], gt[1], "gt", connectivity, min_voxels))


def test_empty_masks():
    zero = np.zeros((9, 9, 9), np.uint8)
    some = LR.random_pair((9, 9, 9), 0.2, 3)[0]
    n, vox = LR.counts(some, some, 3, 1)[[0, 5]]
    assert n >= 1
    assert _assert_pair(zero, zero, 3, 1).tolist() == [0] * 8
    assert _assert_pair(zero, some, 3, 1).tolist() == [n, 0, 0, n, 0, vox, 0, 0]       # empty prediction: every lesion missed
    assert _assert_pair(some, zero, 3, 1).tolist() == [0, n, 0, 0, n, 0, vox, 0]       # empty ground truth: every lesion false
    assert LS.lesion_table(zero, some, "pred").shape == (0, 3)
    batch_p, batch_g = np.stack([zero, some, zero, some]), np.stack([some, zero, zero, some])
    got = LS.lesion_counts(batch_p, batch_g).cpu().numpy()
    np.testing.assert_array_equal(got, np.stack([LR.counts(p, g) for p, g in zip(batch_p, batch_g)]))


def test_operands_and_repeatability():
    pred, gt = _random(0.3)
    ref = _random_ref(0.3, 3, 1)
    tp, tg = _dev(pred), _dev(gt)
    first = LS.lesion_counts(tp, tg)
    assert torch.equal(first, LS.lesion_counts(tp, tg))                                # the same bits on every run
    assert torch.equal(first, LS.lesion_counts(pred, gt))                              # numpy in
    assert torch.equal(first, LS.lesion_counts(tp.bool(), tg.float()))                 # any dtype: non-zero is foreground
    wide_p, wide_g = torch.zeros((3, 17, 13, 140), dtype=torch.uint8, device=DEV), torch.zeros((3, 34, 13, 70), dtype=torch.uint8, device=DEV)
    wide_p[..., ::2] = tp
    wide_g[:, ::2] = tg
    assert not wide_p[..., ::2].is_contiguous() and not wide_g[:, ::2].is_contiguous()
    assert torch.equal(first, LS.lesion_counts(wide_p[..., ::2], wide_g[:, ::2]))      # non-contiguous views
    np.testing.assert_array_equal(first.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="one shape"):
        LS.lesion_counts(tp, tg[:2])
    with pytest.raises(ValueError, match="one shape"):
        LS.lesion_counts(tp[:1], tg[0])


def test_chunks_under_the_workspace_budget(monkeypatch):
    """the last launch sequence holds fewer volumes than the workspace was sized for"""
    pred, gt = _random(0.3)
    tp, tg = _dev(pred), _dev(gt)
    whole = LS.lesion_counts(tp, tg, 1, 3)
    per_vol = int(_lib.load().dycon_lesion_workspace(1, *SHAPE)) + 8 * int(np.prod(SHAPE))
    monkeypatch.setattr(CC, "WORKSPACE_BUDGET", 2 * per_vol + per_vol // 2)
    assert CC._pieces(tp, "dycon_lesion_workspace", root_maps=2)[0] == [(0, 2), (2, 1)]
    assert torch.equal(LS.lesion_counts(tp, tg, 1, 3), whole)
    np.testing.assert_array_equal(whole.cpu().numpy(), _random_ref(0.3, 1, 3))
    for v, t in enumerate(LS.lesion_table(tp, tg, "pred", 1, 3)):
        np.testing.assert_array_equal(t, LR.table(pred[v], gt[v], "pred", 1, 3))


def test_lesion_metrics():
    pred, gt = _random(0.3)
    spacing = (0.5, 2.0, 1.25)
    for connectivity, min_voxels, empty in ((1, 1, 1.0), (3, 3, 0.0)):
        got = LS.lesion_metrics(_dev(pred), _dev(gt), voxelspacing=spacing, connectivity=connectivity, min_voxels=min_voxels,
                                empty_value=empty)
        for v, row in enumerate(_random_ref(0.3, connectivity, min_voxels)):
            ref = LR.metrics(row, 0.5 * 2.0 * 1.25, empty)
            for name in ref:
                np.testing.assert_allclose(got[name][v], ref[name], rtol=RTOL, atol=0)
    zero = np.zeros((9, 9, 9), np.uint8)
    one = LS.lesion_metrics(zero, zero, empty_value=0.5)
    assert {k: float(v) for k, v in one.items()} == LR.metrics([0] * 8, 1.0, 0.5)
    assert LS.lesion_metrics(pred[0], gt[0], voxelspacing=2.0)["abs_volume_diff"] == 8.0 * abs(int(pred[0].sum()) - int(gt[0].sum()))


def test_c_abi_refusals():
    shape = (4, 5, 6)
    root = torch.zeros((2,) + shape, dtype=torch.int32, device=DEV)
    counts = torch.zeros((2, 8), dtype=torch.int64, device=DEV)
    ws = torch.empty(int(_lib.load().dycon_lesion_workspace(2, *shape)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(pred=root.data_ptr(), n_vol=2, shape=shape, min_voxels=1, ws_bytes=ws.numel()):
        _lib.call("dycon_lesion_counts", pred, root.data_ptr(), n_vol, *shape, min_voxels, counts.data_ptr(), ws.data_ptr(), ws_bytes,
                  stream)

    call()
    assert counts.tolist() == [[0] * 8] * 2
    for bad, match in ((dict(pred=None), "null pointer"), (dict(n_vol=0), "every axis"), (dict(shape=(4, 5, 513)), "every axis"),
                       (dict(min_voxels=0), "min_voxels"), (dict(ws_bytes=ws.numel() - 1), "workspace")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            call(**bad)
    torch.cuda.synchronize()


def test_root_values_outside_the_volume_are_background():
    """include/dycon_hip.h: a value outside 1..X*Y*Z in a root map is read as background, so it addresses nothing"""
    pred, gt = LR.random_pair((9, 9, 9), 0.2, 5)
    pred[0, 0, :4] = gt[0, 0, :4] = 0
    root_p, root_g = CC.component_roots(_dev(pred)[None]), CC.component_roots(_dev(gt)[None])
    root_p[0, 0, 0, :4] = torch.tensor([-7, 730, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)      # 729 voxels
    root_g[0, 0, 0, :4] = torch.tensor([730, -1, 0, 2 ** 30], dtype=torch.int32, device=DEV)
    counts = torch.empty((1, 8), dtype=torch.int64, device=DEV)
    ws = torch.empty(int(_lib.load().dycon_lesion_workspace(1, 9, 9, 9)), dtype=torch.uint8, device=DEV)
    _lib.call("dycon_lesion_counts", root_p.data_ptr(), root_g.data_ptr(), 1, 9, 9, 9, 1, counts.data_ptr(), ws.data_ptr(), ws.numel(),
              torch.cuda.current_stream().cuda_stream)
    np.testing.assert_array_equal(counts[0].cpu().numpy(), LR.counts(pred, gt, 3, 1))


# ------------------------------------------------------------------ the protocol of code/test_ISLES22.py
def _blob(shape, centre, radius):
    x, y, z = np.indices(shape)
    return ((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _four_cases():
    """(pred, gt) at 16^3, one per branch of the protocol: both empty, empty prediction, empty ground truth, and two lesions each of
    which one is hit (a true positive, a miss and a false positive)"""
    shape = (16, 16, 16)
    zero = np.zeros(shape, np.uint8)
    a, b, c = _blob(shape, (5, 5, 5), 3), _blob(shape, (6, 5, 5), 3), _blob(shape, (12, 12, 11), 2)
    d = _blob(shape, (3, 12, 12), 1)
    return [(zero, zero), (zero, a), (a | c, zero), (b | d, a | c)]


@functools.lru_cache(maxsize=None)
def _four_refs():
    return [LR.isles_case(p, g) for p, g in _four_cases()]


class _ImageIsLogit(torch.nn.Module):
    """(None, logits) with logits = (-x, x): the class-1 softmax is > 0.5 exactly where the image is > 0"""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))         # the evaluator takes the device from the parameters

    def forward(self, x):
        return None, torch.cat([-x, x], 1)


def _assert_case(got, ref):
    assert tuple(got)[:5] == IE.CASE_FIELDS
    for name in ("dice", "sensitivity", "specificity"):
        assert got[name] == ref[name], name                       # the same fp64 expression on the same integers
    for name in ("hd95", "asd"):
        np.testing.assert_allclose(got[name], ref[name], rtol=RTOL, atol=0, err_msg=name)


@pytest.mark.parametrize("device_surface", [True, False])
def test_isles_case_metrics_four_branches(device_surface):
    refs = _four_refs()
    far = float(np.linalg.norm((16, 16, 16)))
    assert refs[0] == dict(dice=1.0, hd95=0.0, asd=0.0, sensitivity=1.0, specificity=1.0)
    assert refs[1] == dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=1.0)
    assert refs[2] == dict(dice=0.0, hd95=far, asd=far, sensitivity=0.0, specificity=0.0)
    assert 0 < refs[3]["dice"] < 1 and refs[3]["hd95"] > refs[3]["asd"] > 0 and 0 < refs[3]["sensitivity"] < 1 > refs[3]["specificity"]
    for (pred, gt), ref in zip(_four_cases(), refs):
        _assert_case(IE.isles_case_metrics(pred, gt, device_surface=device_surface), ref)
        _assert_case(IE.isles_case_metrics(_dev(pred), _dev(gt, np.int64), device_surface=device_surface), ref)
    pred, gt = _four_cases()[3]
    spacing = (1.0, 0.5, 2.0)
    ref = LR.isles_case(pred, gt, percase=lambda p, g: SE.calculate_metric_percase(p, g, voxelspacing=spacing))
    assert ref["hd95"] != refs[3]["hd95"]
    _assert_case(IE.isles_case_metrics(_dev(pred), gt, device_surface=device_surface, voxelspacing=spacing), ref)


@pytest.mark.parametrize("patch_size", [None, (16, 16, 16)], ids=["whole_volume", "window"])
def test_evaluate_isles22(patch_size):
    net = _ImageIsLogit().to(DEV)
    pairs, refs = _four_cases(), _four_refs()
    cases = [(p.astype(np.float32) * 4.0 - 2.0, g.astype(np.float64)) for p, g in pairs]       # logit +2 inside the prediction, -2 outside
    out = IE.evaluate_isles22(net, cases, patch_size=patch_size, min_voxels=2)
    assert set(out) == {"per_case", "summary"}
    assert tuple(out["per_case"]) == tuple(out["summary"]) == IE.CASE_FIELDS + IE.LESION_FIELDS
    for k, ref in enumerate(refs):
        _assert_case({name: out["per_case"][name][k] for name in out["per_case"]}, ref)
        lesion = LR.metrics(LR.counts(*pairs[k], 3, 2), 1.0, 1.0)
        for name in IE.LESION_FIELDS:
            np.testing.assert_allclose(out["per_case"][name][k], lesion[name], rtol=RTOL, atol=0, err_msg=name)
    assert out["per_case"]["lesion_f1"].tolist() == [1.0, 0.0, 0.0, 0.5]
    assert out["per_case"]["lesion_count_diff"].tolist() == [0.0, 1.0, 2.0, 0.0]
    for name, values in out["per_case"].items():
        assert values.dtype == np.float64 and values.shape == (4,)
        assert out["summary"][name] == (np.mean(values), np.std(values))
    plain = IE.evaluate_isles22(net, cases, patch_size=patch_size, lesion=False)
    assert tuple(plain["per_case"]) == IE.CASE_FIELDS
    for name in IE.CASE_FIELDS:
        np.testing.assert_array_equal(plain["per_case"][name], out["per_case"][name])
    # a case that carries its spacing: HD95, ASD and the volume difference are in its units
    spacing = (1.0, 0.5, 2.0)
    spaced = IE.evaluate_isles22(net, [cases[3] + (spacing,)], patch_size=patch_size)
    ref = LR.isles_case(*pairs[3], percase=lambda p, g: SE.calculate_metric_percase(p, g, voxelspacing=spacing))
    _assert_case({name: spaced["per_case"][name][0] for name in spaced["per_case"]}, ref)
    assert spaced["per_case"]["abs_volume_diff"][0] == abs(int(pairs[3][0].sum()) - int(pairs[3][1].sum())) * 1.0
    assert spaced["summary"]["hd95"] == (spaced["per_case"]["hd95"][0], 0.0)
