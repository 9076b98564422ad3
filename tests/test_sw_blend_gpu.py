"""`sliding_window.Blend` on the MI355X: dycon_sw_gather_mirror, dycon_sw_accumulate_weighted, the driver and the evaluators.

Yardsticks: np.flip of the zero-padded volume's slices for the gather (bit equality); the unweighted entry points for unit tables
and mask 0 (bit equality: 1 * p and n + 1 are exact); the fp64 restatement tests/sw_blend_ref.py for everything else, fed random logits
for the kernel alone and the CPU oracle nets end to end, at the bounds of tests/test_ensemble_gpu.py.

Case A: (40, 36, 20), windows (32, 32, 16), stride 16 / 4 -> 8 windows, batch_size 3.
Case B: (24, 40, 12), stride 8 / 4 -> 2 windows, padded on two axes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sw_blend_ref as BR
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
from dycon_paper_replication_amd.utils import case_loop, device_eval, isles_eval, surface_eval
from dycon_paper_replication_amd.utils import ensemble_eval as EE
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import sliding_window as SW
from dycon_paper_replication_amd.utils import test_3d_patch as T3
from dycon_paper_replication_amd.utils.sliding_window import Blend
from oracle import nets as ON

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATCH = (32, 32, 16)
CASES = {"A": dict(shape=(40, 36, 20), sxy=16, sz=4, batch_size=3), "B": dict(shape=(24, 40, 12), sxy=8, sz=4, batch_size=4)}
INT3 = ctypes.c_int * 3


def _image(shape):
    return np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------- 1. the gather
@pytest.mark.parametrize("shape,patch", [((24, 40, 12), (32, 32, 16)), ((13, 9, 7), (8, 8, 6)), ((5, 11, 3), (8, 6, 7))],
                         ids=["caseB", "no-pad", "odd-last-axis"])
def test_gather_mirror_equals_flipped_slices_of_the_padded_volume(shape, patch):
    vol = _image(shape)
    padded = np.pad(vol, EE._center_pads(shape, patch), mode="constant", constant_values=0)
    far = tuple(padded.shape[a] - patch[a] for a in range(3))
    rng = np.random.default_rng(2)
    table = [tuple(int(rng.integers(0, far[a] + 1)) for a in range(3)) + (mask,) for mask in rng.permutation(8).tolist()]
    table[0] = (0, 0, 0) + table[0][3:]
    table[-1] = far + table[-1][3:]
    assert sorted(e[3] for e in table) == list(range(8))                         # every mask once
    ent = torch.tensor(table, dtype=torch.int32, device=DEV)
    dvol = torch.from_numpy(vol).to(DEV)

    def want(x, y, z, mask):
        win = padded[x:x + patch[0], y:y + patch[1], z:z + patch[2]]
        return np.flip(win, tuple(a for a in range(3) if mask >> a & 1))

    for first, n in ((0, 8), (2, 3), (7, 1)):
        out = torch.full((n + 1, 1) + patch, 7.0, dtype=torch.float32, device=DEV)
        _lib.call("dycon_sw_gather_mirror", dvol.data_ptr(), *shape, ent.data_ptr(), len(table), first, n, *patch, out.data_ptr(), _stream())
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], np.stack([want(*e) for e in table[first:first + n]])[:, None])
        assert (got[n] == 7.0).all()                                             # nothing behind the n windows is written
    for first, n in ((6, 3), (8, 1), (-1, 2)):
        with pytest.raises(_lib.DyconLibraryError, match="sw_gather_mirror"):
            _lib.call("dycon_sw_gather_mirror", dvol.data_ptr(), *shape, ent.data_ptr(), len(table), first, n, *patch, out.data_ptr(), _stream())


# ---------------------------------------------------------------- 2. / 3. the accumulate on random logits
A_PATCH, A_VOL, A_ORIGINS = (8, 8, 4), (12, 8, 6), [(0, 0, 0), (4, 0, 2)]


def _random_logits(M, n, C, seed):
    rng = np.random.default_rng(seed)
    return [(3.0 * rng.standard_normal((n,) + A_PATCH + (C,))).astype(np.float32) for _ in range(M)]


def _weighted(logits, C, all_classes, entries, tabs, score, cnt, box=None):
    """one dycon_sw_accumulate_weighted launch; logits, entries, tabs, score, cnt: device tensors"""
    ptrs = [l.data_ptr() for l in logits] + [None] * (4 - len(logits))
    lo, hi = (None, None) if box is None else (INT3(*box[0]), INT3(*box[1]))
    _lib.call("dycon_sw_accumulate_weighted", *ptrs, len(logits), C, int(all_classes), len(entries), *A_PATCH, entries.data_ptr(),
              *(t.data_ptr() for t in tabs), score.data_ptr(), cnt.data_ptr(), *A_VOL, lo, hi, _stream())


def _maps(C=None):
    score = torch.zeros(((C,) if C else ()) + A_VOL, dtype=torch.float32, device=DEV)
    return score, torch.zeros(A_VOL, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("M,C,all_classes,box", [(1, 2, False, None), (1, 3, False, None), (2, 2, False, None), (2, 8, False, None),
                                                 (4, 2, False, None), (4, 8, False, None), (1, 3, True, ((0, 0, 0), (12, 8, 6))),
                                                 (1, 3, True, ((2, 0, 1), (10, 7, 5)))])
def test_unit_weights_and_mask_0_are_the_existing_kernels(M, C, all_classes, box):
    logits = [torch.from_numpy(l).to(DEV) for l in _random_logits(M, 2, C, 100 * M + 10 * C + all_classes)]
    org = torch.tensor(A_ORIGINS, dtype=torch.int32, device=DEV)
    ent = torch.tensor([o + (0,) for o in A_ORIGINS], dtype=torch.int32, device=DEV)
    ones = [torch.ones(p, dtype=torch.float32, device=DEV) for p in A_PATCH]
    score, cnt = _maps(C if all_classes else None)
    ref_score, ref_cnt = _maps(C if all_classes else None)
    maps = (2, *A_PATCH, org.data_ptr(), ref_score.data_ptr(), ref_cnt.data_ptr(), *A_VOL)
    for _ in range(2):                                                           # two chunks: the maps accumulate
        _weighted(logits, C, all_classes, ent, ones, score, cnt, box)
        if all_classes:
            _lib.call("dycon_sw_accumulate_all", logits[0].data_ptr(), C, *maps, INT3(*box[0]), INT3(*box[1]), _stream())
        elif M > 1:
            _lib.call("dycon_sw_accumulate_ens", *[l.data_ptr() for l in logits], *[None] * (4 - M), M, C, *maps, _stream())
        elif C == 2:
            _lib.call("dycon_sw_accumulate", logits[0].data_ptr(), *maps, _stream())
        else:
            _lib.call("dycon_sw_accumulate_c", logits[0].data_ptr(), C, *maps, _stream())
    assert torch.equal(score, ref_score) and torch.equal(cnt, ref_cnt)
    assert set(cnt.unique().tolist()) == {0.0, 2.0, 4.0}                         # uncovered, covered once, the overlap; two chunks
    assert float(score.abs().max()) > 0


A_ENTRIES = [o + (mask,) for o in A_ORIGINS for mask in (0, 5, 7)]


@pytest.mark.parametrize("M,C,all_classes,ramp_axis", [(1, 2, False, None), (1, 8, False, None), (3, 2, False, None), (3, 8, False, None),
                                                       (1, 2, True, None), (1, 8, True, None), (1, 2, False, 0), (3, 8, False, 2),
                                                       (1, 8, True, 0), (1, 2, True, 2)])
def test_gaussian_tables_and_mixed_masks_against_fp64(M, C, all_classes, ramp_axis):
    """`ramp_axis`: that axis's table is an asymmetric ramp, so a kernel that weights by the mirrored coordinate, or un-flips the wrong
    axis, cannot pass.  cnt: two roundings in w = (g0 * g1) * g2 and one per add, k - 1 inside the kernel and one into the zeroed map."""
    tabs = list(SW.window_weights(A_PATCH, Blend("gaussian")))
    if ramp_axis is not None:
        tabs[ramp_axis] = np.linspace(0.25, 1.0, A_PATCH[ramp_axis]).astype(np.float32)
        assert not np.array_equal(tabs[ramp_axis], tabs[ramp_axis][::-1])
    host = _random_logits(M, len(A_ENTRIES), C, 1000 + 100 * M + 10 * C + all_classes)
    ref_score, ref_cnt = BR.accumulate(np.stack(host), A_ENTRIES, A_PATCH, A_VOL, tabs, all_classes)
    logits = [torch.from_numpy(l).to(DEV) for l in host]
    ent = torch.tensor(A_ENTRIES, dtype=torch.int32, device=DEV)
    dtabs = [torch.from_numpy(t).to(DEV) for t in tabs]
    runs = []
    for _ in range(2):
        score, cnt = _maps(C if all_classes else None)
        _weighted(logits, C, all_classes, ent, dtabs, score, cnt)
        runs.append((score, cnt))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    score, cnt = runs[0][0].cpu().numpy().astype(np.float64), runs[0][1].cpu().numpy().astype(np.float64)
    k = np.zeros(A_VOL)
    for x, y, z, _ in A_ENTRIES:
        k[x:x + A_PATCH[0], y:y + A_PATCH[1], z:z + A_PATCH[2]] += 1
    covered = k > 0
    assert set(np.unique(k).tolist()) == {0.0, 3.0, 6.0}
    assert (cnt[~covered] == 0).all() and (score[..., ~covered] == 0).all()      # uncovered voxels stay untouched
    cnt_err = np.abs(cnt - ref_cnt)[covered] / ref_cnt[covered]
    score_err = np.abs(score - ref_score)[..., covered] / ref_score[..., covered]
    print(f"M={M} C={C} all={all_classes} ramp={ramp_axis}: cnt rel err {cnt_err.max():.3e} (bound {9 * 2.0 ** -24:.3e}); "
          f"score rel err {score_err.max():.3e}")
    assert (cnt_err <= ((k + 3) * 2.0 ** -24)[covered]).all()
    np.testing.assert_allclose(score[..., covered], ref_score[..., covered], rtol=1e-4, atol=0)
    # the finalize entry points are reused unchanged: they divide a float score by a float cnt
    label = torch.empty(A_VOL, dtype=torch.uint8, device=DEV)
    prob = torch.empty_like(runs[0][0])
    ref_prob = ref_score[..., covered] / ref_cnt[covered]
    if all_classes:
        _lib.call("dycon_sw_finalize_argmax", runs[0][0].data_ptr(), runs[0][1].data_ptr(), C, cnt.size, label.data_ptr(), prob.data_ptr(),
                  _stream())
        top = np.sort(ref_prob, 0)
        decided = top[-1] - top[-2] > 2.2e-4                                     # twice the bound on one probability
        ref_label = ref_prob.argmax(0)
    else:
        _lib.call("dycon_sw_finalize", runs[0][0].data_ptr(), runs[0][1].data_ptr(), cnt.size, 0.5, label.data_ptr(), prob.data_ptr(),
                  _stream())
        decided = np.abs(ref_prob - 0.5) > 1.1e-4
        ref_label = ref_prob > 0.5
    np.testing.assert_allclose(prob.cpu().numpy()[..., covered], ref_prob, rtol=1e-4, atol=1e-5)
    assert np.array_equal(label.cpu().numpy()[covered][decided], ref_label[decided])
    assert decided.mean() > 0.99


# ---------------------------------------------------------------- 4. end to end against the CPU oracle nets
@functools.lru_cache(maxsize=None)
def _params(net_type, seed, C):
    return (ON.make_vnet_params if net_type == "vnet" else ON.make_unet_params)(seed, n_classes=C)


@functools.lru_cache(maxsize=None)
def _model(net_type, seed, C=2):
    model = net_factory_3d(net_type, 1, C, 2, dtype=torch.float32).to(DEV)
    model.load_state_dict(_params(net_type, seed, C))
    return model


def _oracle_net(net_type, seed, C=2):
    return lambda t: ON.forward(net_type, t, _params(net_type, seed, C), bn_training=False)[1]


@functools.lru_cache(maxsize=None)
def _restated(case, nets, C, blend, all_classes=False):
    """(label, prob) of the fp64 restatement over the CPU oracle nets: computed once, never written to"""
    c = CASES[case]
    out = BR.single_case([_oracle_net(kind, seed, C) for kind, seed in nets], _image(c["shape"]), c["sxy"], c["sz"], PATCH,
                         weighting=blend.weighting, sigma_scale=blend.sigma_scale, mirror_axes=blend.mirror_axes, all_classes=all_classes)
    for a in out:
        a.setflags(write=False)
    return out


def _check_against_the_oracle(name, lab, score, lab_plain, lab_ref, score_ref, undecided, blend):
    """the bounds of test_ensemble_matches_the_oracle; and the option reached the kernel: the label map moved against blend=None"""
    changed = float((lab != lab_plain).mean())
    print(f"{name}: |score - restated| {np.abs(score - score_ref).max():.3e}; undecided {undecided.mean():.5f}; "
          f"labels changed against blend=None {changed:.4f}")
    np.testing.assert_allclose(score, score_ref, rtol=1e-4, atol=1e-5)
    assert undecided.mean() <= 0.005
    assert np.array_equal(lab[~undecided], lab_ref[~undecided])
    assert changed > (0.05 if blend.mirror_axes else 0.01)


# labels changed against the plain mean, on the fp64 restatement with the CPU oracle nets (undecided share in brackets):
#   V-Net 3 / B gaussian + mirror (0, 1, 2)          10.6 %  (0)
#   V-Net 3 / A gaussian                              3.9 %  (0.00028)
#   U-Net 7 / B constant + mirror (0, 2)             22.9 %  (0.00035)
#   U-Net 7, C = 3 / B gaussian + mirror (0, 2)      41.4 %  (0.00130, top-two margin < 2.2e-4)
#   V-Nets 3 + 5 / B gaussian + mirror (0, 2)        17.7 %  (0.00043)
# Half of each is above the thresholds, 1 % for Gaussian weighting alone and 5 % with mirroring, so those stand.
@pytest.mark.parametrize("case,net,blend,batch_size", [("B", ("vnet", 3), Blend("gaussian", mirror_axes=(0, 1, 2)), 3),
                                                       ("A", ("vnet", 3), Blend("gaussian"), 3),
                                                       ("B", ("unet_3D", 7), Blend("constant", mirror_axes=(0, 2)), 4)],
                         ids=["B-vnet-gaussian-mirror012", "A-vnet-gaussian", "B-unet-constant-mirror02"])
def test_single_case_matches_the_restatement(case, net, blend, batch_size):
    """B with mirror (0, 1, 2) at batch_size 3: 16 entries in chunks of 3, so chunks split a window's flips"""
    c = CASES[case]
    image, model = _image(c["shape"]), _model(*net)
    lab_ref, score_ref = _restated(case, (net,), 2, blend)
    model.train()
    lab, score = T3.test_single_case(model, image, c["sxy"], c["sz"], PATCH, num_classes=2, batch_size=batch_size, blend=blend)
    assert model.training                                                        # the model's mode is restored
    model.eval()
    lab_plain = SW.single_case_device(model, image, c["sxy"], c["sz"], PATCH, batch_size=batch_size)[0].cpu().numpy()
    assert not model.training
    assert lab.shape == c["shape"] and lab.dtype == np.int64 and score.shape == (2,) + c["shape"] and score.dtype == np.float32
    assert np.array_equal(score[0], score[1])                                    # the reference's broadcast (:338-339)
    _check_against_the_oracle(f"{case} {net} {blend}", lab, score[0], lab_plain, lab_ref, score_ref, np.abs(score_ref - 0.5) < 1e-4, blend)


def test_single_case_classes_matches_the_restatement():
    """undecided: the two largest probabilities closer than 2.2e-4, twice the score bound (1e-4 * p + 1e-5 with p <= 1)"""
    c, blend, net = CASES["B"], Blend("gaussian", mirror_axes=(0, 2)), ("unet_3D", 7)
    image, model = _image(c["shape"]), _model(*net, 3)
    lab_ref, score_ref = _restated("B", (net,), 3, blend, True)
    model.train()
    lab, score = EC.test_single_case_classes(model, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"], blend=blend)
    assert model.training
    lab_plain = EC.single_case_classes_device(model, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"])[0].cpu().numpy()
    assert lab.shape == c["shape"] and score.shape == (3,) + c["shape"] and score.dtype == np.float32
    top = np.sort(score_ref, 0)
    _check_against_the_oracle(f"B {net} C=3 {blend}", lab, score, lab_plain, lab_ref, score_ref, top[-1] - top[-2] < 2.2e-4, blend)
    assert np.abs(score.sum(0, dtype=np.float64) - 1).max() <= 1e-5 and len(np.unique(lab)) == 3


def test_ensemble_matches_the_restatement():
    c, blend, pair = CASES["B"], Blend("gaussian", mirror_axes=(0, 2)), (("vnet", 3), ("vnet", 5))
    image, models = _image(c["shape"]), [_model(*n) for n in pair]
    lab_ref, score_ref = _restated("B", pair, 2, blend)
    models[0].train()
    models[1].eval()
    lab, score = EE.single_case_plus_device(*models, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"], blend=blend)
    assert models[0].training and not models[1].training                         # every model's mode is restored
    lab_plain = EE.single_case_plus_device(*models, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"])[0].cpu().numpy()
    assert lab.is_cuda and lab.dtype == torch.uint8 and score.dtype == torch.float32 and tuple(score.shape) == c["shape"]
    _check_against_the_oracle(f"B {pair} {blend}", lab.cpu().numpy(), score.cpu().numpy(), lab_plain, lab_ref, score_ref,
                              np.abs(score_ref - 0.5) < 1e-4, blend)


# ---------------------------------------------------------------- 5. default and identity
@pytest.mark.parametrize("case,net_type,C", [("A", "vnet", 2), ("B", "unet_3D", 3)], ids=["A-vnet-2", "B-unet-3"])
def test_constant_blend_without_mirroring_gives_the_bits_of_no_blend(case, net_type, C):
    c = CASES[case]
    image, m = _image(c["shape"]), _model(net_type, 3, C)
    args = (image, c["sxy"], c["sz"], PATCH)
    for run in (lambda **kw: SW.single_case_device(m, *args, batch_size=c["batch_size"], **kw),
                lambda **kw: EE.single_case_plus_device(m, _model(net_type, 5, C), *args, batch_size=c["batch_size"], **kw),
                lambda **kw: EC.single_case_classes_device(m, *args, batch_size=c["batch_size"], **kw)):
        label, prob = run(blend=Blend("constant"))
        ref_label, ref_prob = run(blend=None)
        assert label.is_cuda and label.dtype == torch.uint8 and prob.dtype == torch.float32
        assert torch.equal(prob, ref_prob) and torch.equal(label, ref_label)
        assert torch.equal(run()[1], ref_prob)                                   # the default is blend=None
        assert 0 < int((label != 0).sum()) < label.numel()


# ---------------------------------------------------------------- 6. the case loops
def _blob(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2


class _RuleNet(torch.nn.Module):
    """tests/test_ensemble_gpu.py: logit difference +1 where the image value is one of `values`, -3 elsewhere.  A pointwise rule of the
    image is flip-equivariant, and a weighted mean of equal values is that value: no blend moves its label map."""

    def __init__(self, values, outputs=2):
        super().__init__()
        self.values, self.outputs = values, outputs
        self.anchor = torch.nn.Parameter(torch.zeros(1))         # the evaluators take the device from the parameters

    def forward(self, x):
        hit = torch.zeros_like(x, dtype=torch.bool)
        for v in self.values:
            hit |= x == v
        d = torch.where(hit, 1.0, -3.0).to(x.dtype)
        logits = torch.cat([-d / 2, d / 2], 1)
        return (logits, None) if self.outputs == 2 else (None, logits, None)


def test_case_loops_with_a_pointwise_rule(monkeypatch):
    """the blended device-resident loop is surface_eval.test_all_case(device_surface=True, blend=...): utils/test_3d_patch.py keeps its
    content, and tests/test_components_cpu.py gives device_eval.test_all_case that module's parameter names"""
    shape = (40, 40, 32)
    big, halo, small = _blob(shape, (14, 14, 14), 7), _blob(shape, (14, 14, 14), 10), _blob(shape, (32, 32, 24), 3)
    left = np.indices(shape)[0] < 14
    image = np.zeros(shape, np.float32)
    image[halo & left], image[halo & ~left] = 1, 2
    image[big | small] = 3
    u8 = lambda a: a.astype(np.uint8)                                            # noqa: E731
    cases = [(image, u8(big)), (image, u8(_blob(shape, (16, 14, 14), 7))), (image[::-1].copy(), u8(big))]
    kw_plus = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    kw = dict(kw_plus, batch_size=5)
    blend = Blend("gaussian", mirror_axes=(0, 1, 2))
    single = _RuleNet((1, 3), outputs=3).to(DEV)
    host = T3.test_all_case(single, cases[:1], 2, **kw)
    # with nothing but a blend the loop is surface_eval's own, through the host maps of test_single_case
    assert surface_eval.test_all_case(single, cases[:1], 2, blend=blend, **kw).tolist() == host.tolist()
    plain = {nms: device_eval.test_all_case(single, cases, 2, nms=nms, **kw) for nms in (0, 1)}

    def no_host_maps(*a, **k):
        raise AssertionError("the device-resident loop copied the label map to the host")

    monkeypatch.setattr(T3, "test_single_case", no_host_maps)
    for nms in (0, 1):
        assert 0 < plain[nms][0] < 1 and plain[nms][2] > 0
        got = surface_eval.test_all_case(single, cases, 2, nms=nms, device_surface=True, blend=blend, **kw)
        assert got.tolist() == plain[nms].tolist()                              # the metrics of device_eval.test_all_case, blend=None
    spaced = surface_eval.test_all_case(single, [cases[1] + ((2.0, 2.0, 2.0),)], 2, nms=1, device_surface=True, blend=blend, **kw)
    unit = surface_eval.test_all_case(single, [cases[1]], 2, nms=1, device_surface=True, blend=blend, **kw)
    np.testing.assert_allclose(spaced[2:], 2.0 * unit[2:], rtol=1e-6)
    monkeypatch.undo()
    # the pair: only the averaged logits give the intersection of the two rules, with and without the blend
    net_l, net_r = _RuleNet((1, 3)).to(DEV), _RuleNet((2, 3)).to(DEV)
    lab, _ = EE.single_case_plus_device(net_l, net_r, image, 8, 8, (32, 32, 16), batch_size=5, blend=blend)
    assert np.array_equal(lab.cpu().numpy(), u8(big | small))
    assert torch.equal(lab, EE.single_case_plus_device(net_l, net_r, image, 8, 8, (32, 32, 16), batch_size=5)[0])
    # test_all_case_plus keeps its pinned parameter list (tests/test_ensemble_cpu.py); its device-resident loop is these two calls
    pair = device_eval._device_case(lambda im: EE.single_case_plus_device(net_l, net_r, im, 8, 8, (32, 32, 16), batch_size=5, blend=blend), 1)
    got = case_loop.mean_over_cases(cases, pair, np.zeros(4), triples=True)
    assert got.tolist() == T3.test_all_case_plus(net_l, net_r, cases, 2, nms=1, device_resident=True, batch_size=5, **kw_plus).tolist()


def test_isles_whole_volume_forward_refuses_a_blend():
    net = _RuleNet((1,), outputs=3).to(DEV)
    image = np.zeros((16, 16, 16), np.float32)
    image[4:9, 4:9, 4:9] = 1
    case = [(image, (image == 1).astype(np.uint8))]
    with pytest.raises(ValueError, match="whole-volume"):
        isles_eval.evaluate_isles22(net, case, blend=Blend("gaussian", mirror_axes=(0,)), lesion=False)
    plain = isles_eval.evaluate_isles22(net, case, patch_size=(8, 8, 8), stride_xy=4, stride_z=4, lesion=False)
    blended = isles_eval.evaluate_isles22(net, case, patch_size=(8, 8, 8), stride_xy=4, stride_z=4, lesion=False,
                                          blend=Blend("gaussian", mirror_axes=(0,)))
    assert plain["per_case"]["dice"].tolist() == blended["per_case"]["dice"].tolist() == [1.0]
