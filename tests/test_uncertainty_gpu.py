"""Uncertainty maps and calibration on the MI355X: dycon_sw_accumulate_moments, dycon_sw_finalize_uncertainty,
dycon_calibration_counts, `utils.uncertainty`.

Yardsticks: dycon_sw_accumulate_weighted and dycon_sw_finalize_argmax for score, cnt, label and prob (bit equality); the fp64
restatement tests/uncertainty_ref.py for the maps, at the bound tests/test_sw_blend_gpu.py applies to blended probability maps
(rtol 1e-4, atol 1e-5), and, mutual information being a difference of two such maps, twice (1e-4 * ln C + 1e-5) absolute for it; the
same restatement for the calibration counts: integers equal, fp64 sums within V * 2**-52 relative (the order of the sum).

Volume (28, 22, 18), windows 16^3 at stride 8: 12 windows.  The thin volume (28, 22, 12) is padded to 16 on its last axis: 6."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import sw_blend_ref as BR
import uncertainty_ref as UR
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.networks.VNet import VNet
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import sliding_window as SW
from dycon_paper_replication_amd.utils import uncertainty as U
from dycon_paper_replication_amd.utils.sliding_window import Blend
from oracle import nets as ON

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATCH, VOL, THIN, STRIDE = (16, 16, 16), (28, 22, 18), (28, 22, 12), 8
INT3 = ctypes.c_int * 3
FLOAT_MAPS = ("entropy", "expected_entropy", "variance")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _mi_bound(C):
    return 2 * (1e-4 * math.log(C) + 1e-5)


# ---------------------------------------------------------------- 1. the kernels on synthetic logits
@functools.lru_cache(maxsize=None)
def _entries():
    """every window in every orientation, shuffled: 96 entries, accumulated in calls of 1, 64 and 31"""
    wins = BR.windows(VOL, PATCH, STRIDE, STRIDE)
    assert len(wins) == 12
    ents = [w + (m,) for w in wins for m in range(8)]
    order = np.random.default_rng(5).permutation(len(ents))
    return [ents[i] for i in order]


CALLS = (1, 64, 31)


def _kernel_logits(C, saturated):
    rng = np.random.default_rng(40 + C)
    shape = (len(_entries()),) + PATCH + (C,)
    if saturated:
        assert C == 2                                                            # (+80, -80) or (-80, +80): one-hot softmaxes in fp32
        return (np.where(rng.random(shape[:-1] + (1,)) < 0.5, 80.0, -80.0) * np.array([1.0, -1.0])).astype(np.float32)
    return (3.0 * rng.standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize("C,saturated", [(2, False), (3, False), (8, False), (2, True)], ids=["C2", "C3", "C8", "C2-saturated"])
def test_moments_and_finalize_kernels(C, saturated):
    ents = _entries()
    host = _kernel_logits(C, saturated)
    tabs = list(SW.window_weights(PATCH, Blend("gaussian")))
    dtabs = [torch.from_numpy(t).to(DEV) for t in tabs]
    table = torch.tensor(ents, dtype=torch.int32, device=DEV)
    logits = torch.from_numpy(host).to(DEV)
    f32 = dict(dtype=torch.float32, device=DEV)
    score, sq, ref_score = (torch.zeros((C,) + VOL, **f32) for _ in range(3))
    cnt, hsum, ref_cnt = (torch.zeros(VOL, **f32) for _ in range(3))
    first = 0
    for n in CALLS:
        lo, hi = SW.chunk_box(np.asarray(ents[first:first + n])[:, :3], PATCH)
        if n == 1:
            assert tuple(h - l for l, h in zip(lo, hi)) == PATCH                 # a box smaller than the volume
        chunk = logits[first:first + n]
        common = (n, *PATCH, table.data_ptr() + 16 * first, *(t.data_ptr() for t in dtabs))
        _lib.call("dycon_sw_accumulate_moments", chunk.data_ptr(), C, *common, score.data_ptr(), cnt.data_ptr(), hsum.data_ptr(),
                  sq.data_ptr(), *VOL, INT3(*lo), INT3(*hi), _stream())
        _lib.call("dycon_sw_accumulate_weighted", chunk.data_ptr(), None, None, None, 1, C, 1, *common, ref_score.data_ptr(),
                  ref_cnt.data_ptr(), *VOL, INT3(*lo), INT3(*hi), _stream())
        first += n
    assert first == len(ents)
    assert torch.equal(score, ref_score) and torch.equal(cnt, ref_cnt)           # the weighted kernel's bits
    assert float(cnt.min()) > 0
    ref = UR.finalize(*UR.moments([host], ents, PATCH, VOL, tabs))
    np.testing.assert_allclose(hsum.cpu().numpy(), ref["expected_entropy"] * cnt.cpu().numpy().astype(np.float64), rtol=1e-4, atol=1e-5)
    label, ref_label = (torch.empty(VOL, dtype=torch.uint8, device=DEV) for _ in range(2))
    maps = {k: torch.empty(VOL, **f32) for k in ("entropy", "expected_entropy", "mutual_info", "variance")}
    _lib.call("dycon_sw_finalize_argmax", ref_score.data_ptr(), ref_cnt.data_ptr(), C, cnt.numel(), ref_label.data_ptr(),
              ref_score.data_ptr(), _stream())
    _lib.call("dycon_sw_finalize_uncertainty", score.data_ptr(), cnt.data_ptr(), hsum.data_ptr(), sq.data_ptr(), C, cnt.numel(),
              label.data_ptr(), *(maps[k].data_ptr() for k in ("entropy", "expected_entropy", "mutual_info", "variance")), _stream())
    assert torch.equal(label, ref_label) and torch.equal(score, ref_score)       # dycon_sw_finalize_argmax's bits
    got = {k: v.cpu().numpy() for k, v in maps.items()}
    for k in FLOAT_MAPS + ("mutual_info",):
        err = np.abs(got[k] - ref[k])
        print(f"C={C} saturated={saturated} {k}: max |err| {err.max():.3e}, max {np.abs(ref[k]).max():.3e}")
        assert not np.isnan(got[k]).any()
    assert not torch.isnan(score).any()
    for k in FLOAT_MAPS:
        np.testing.assert_allclose(got[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)
    assert np.abs(got["mutual_info"] - ref["mutual_info"]).max() <= _mi_bound(C)
    assert (got["mutual_info"] >= 0).all() and (got["variance"] >= 0).all()
    assert ref["mutual_info"].max() > 0.05                                       # random members disagree: the maps are not trivially 0
    if saturated:
        assert float(hsum.abs().max()) == 0.0                                    # one-hot members: entropy 0, not NaN
    bad = INT3(0, 0, 0), INT3(29, 22, 18)
    with pytest.raises(_lib.DyconLibraryError, match="sw_accumulate_moments"):
        _lib.call("dycon_sw_accumulate_moments", logits.data_ptr(), C, 1, *PATCH, table.data_ptr(), *(t.data_ptr() for t in dtabs),
                  score.data_ptr(), cnt.data_ptr(), hsum.data_ptr(), sq.data_ptr(), *VOL, *bad, _stream())


# ---------------------------------------------------------------- 2. the calibration counts
def _calibration_case(C, seed):
    """random softmaxes with hand-placed confidences: exactly 1.0, the bin edges k / 16 and k / 15, ties"""
    rng = np.random.default_rng(seed)
    V = VOL[0] * VOL[1] * VOL[2]
    z = 2.5 * rng.standard_normal((C, V))
    prob = BR.softmax64(z).astype(np.float32)
    edges = [np.float32(k / 16) for k in range(8, 17)] + [np.float32(k / 15) for k in range(8, 16)]
    for j, c in enumerate(edges * 3):
        col = np.zeros(C, np.float32)
        col[j % C], col[(j + 1) % C] = c, np.float32(1) - c
        prob[:, 7 * j] = col
    prob[:, 5] = np.float32(1.0 / C) if C == 2 else np.array([0.4, 0.4, 0.2], np.float32)      # a tie: the lowest index predicts
    label = rng.integers(0, C, V)
    agree = rng.random(V) < 0.7
    label[agree] = prob.argmax(0)[agree]
    mask = (rng.random(V) < 0.6).astype(np.uint8)
    mask[:7 * 3 * len(edges)] = 1                                                # the hand-placed voxels are scored
    unc = (rng.random(V) * math.log(C)).astype(np.float32)
    unc[:3] = np.float32(math.log(C)), 0.0, np.float32(math.log(C)) / 15
    return prob, label.astype(np.uint8), mask, unc


def _counts(prob, label, mask, unc, u_max, C, K):
    V = label.numel()
    counts = torch.full((4 * K + 2,), -1, dtype=torch.int64, device=DEV)         # the entry point zeroes them
    sums = torch.full((K + 2,), -1.0, dtype=torch.float64, device=DEV)
    ws_bytes = _lib.load().dycon_calibration_workspace(V, K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=DEV)
    _lib.call("dycon_calibration_counts", prob.data_ptr(), label.data_ptr(), None if mask is None else mask.data_ptr(),
              None if unc is None else unc.data_ptr(), u_max, C, V, K, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    return counts.cpu().numpy(), sums.cpu().numpy()


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("K", [15, 16])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
def test_calibration_counts(C, K, masked):
    prob, label, mask, unc = _calibration_case(C, 10 * C + K)
    V = label.size
    ref = UR.calibration_counts(prob, label, K, mask if masked else None, unc, math.log(C))
    dev = [torch.from_numpy(a).to(DEV) for a in (prob, label, mask, unc)]
    args = (dev[0], dev[1], dev[2] if masked else None, dev[3], math.log(C), C, K)
    counts, sums = _counts(*args)
    again = _counts(*args)
    assert counts.tobytes() == again[0].tobytes() and sums.tobytes() == again[1].tobytes()       # the same bits on every run
    assert counts[:K].tolist() == ref["n"].tolist() and counts[K:2 * K].tolist() == ref["correct"].tolist()
    assert counts[2 * K:4 * K].reshape(2, K).tolist() == ref["unc_hist"].tolist()
    assert counts[4 * K] == ref["n_scored"] == counts[:K].sum() and counts[4 * K + 1] == 0
    assert ref["n"][K - 1] >= 3 and (ref["n"] > 0).sum() >= K // 2                # the edge cases landed; many bins are in use
    tol = V * 2.0 ** -52
    for name, got, want in (("brier_sum", sums[K], ref["brier_sum"]), ("nll_sum", sums[K + 1], ref["nll_sum"])):
        print(f"C={C} K={K} masked={masked} {name}: rel err {abs(got - want) / want:.3e} (bound {tol:.3e})")
        assert abs(got - want) <= tol * want, name
    used = ref["n"] > 0
    assert (sums[:K][~used] == 0).all()
    assert (np.abs(sums[:K] - ref["conf_sum"])[used] <= tol * ref["conf_sum"][used]).all()
    # without an uncertainty map the two histograms stay empty and nothing else moves
    plain = _counts(dev[0], dev[1], dev[2] if masked else None, None, 1.0, C, K)
    assert (plain[0][2 * K:4 * K] == 0).all() and plain[0][:2 * K].tolist() == counts[:2 * K].tolist()
    assert plain[1].tobytes() == sums.tobytes()
    # the public function: host arithmetic on these outputs
    res = U.calibration(dev[0].reshape((C,) + VOL), label.reshape(VOL), bins=K, mask=mask.reshape(VOL) if masked else None,
                        uncertainty=dev[3].reshape(VOL))
    ece, mce = UR.ece_mce(ref["n"], ref["correct"], ref["conf_sum"])
    assert res["n"] == ref["n_scored"] and res["ece"] == pytest.approx(ece, rel=1e-9) and res["mce"] == pytest.approx(mce, rel=1e-9)
    assert res["brier"] == pytest.approx(ref["brier_sum"] / ref["n_scored"], rel=1e-9)
    assert res["nll"] == pytest.approx(ref["nll_sum"] / ref["n_scored"], rel=1e-9)
    assert res["accuracy"] == ref["correct"].sum() / ref["n_scored"]
    assert res["error_auroc"] == pytest.approx(UR.error_auroc(ref["unc_hist"]), rel=1e-9) and 0 <= res["aurc"] <= 1
    assert res["reliability"].shape == (K, 3) and res["reliability"][:, 0].tolist() == ref["n"].tolist()


def test_calibration_refuses_a_label_outside_the_classes():
    prob, label, mask, _ = _calibration_case(3, 1)
    label = label.copy()
    hit = int(np.flatnonzero(mask)[0])
    label[hit] = 3
    with pytest.raises(ValueError, match="label outside"):
        U.calibration(prob, label, bins=15)
    counts, _ = _counts(torch.from_numpy(prob).to(DEV), torch.from_numpy(label).to(DEV), None, None, 1.0, 3, 15)
    assert counts[4 * 15 + 1] == 1 and counts[4 * 15] == label.size - 1          # counted there and nowhere else
    masked_out = mask.copy()
    masked_out[hit] = 0
    assert U.calibration(prob, label, bins=15, mask=masked_out)["n"] == int(masked_out.sum())    # a voxel that is not scored is not read
    with pytest.raises(ValueError, match="label outside"):
        U.calibration(prob, np.where(np.arange(label.size) == hit, -1, label.astype(np.int64)), bins=15)
    with pytest.raises(_lib.DyconLibraryError, match="calibration_counts"):
        _counts(torch.from_numpy(prob).to(DEV), torch.from_numpy(label).to(DEV), None, None, 1.0, 3, 65)


# ---------------------------------------------------------------- 3. the driver
def _image(shape):
    return np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _model(net_type, seed, C=2):
    model = net_factory_3d(net_type, 1, C, 2, dtype=torch.float32).to(DEV)
    model.load_state_dict((ON.make_vnet_params if net_type == "vnet" else ON.make_unet_params)(seed, n_classes=C))
    return model.eval()


def _member(model):
    """the model's own logits of one window, for the restatement"""
    def net(t):
        assert not model.training
        return model(t.to(DEV))[1].float()
    return net


@functools.lru_cache(maxsize=None)
def _restated(nets, shape, C, blend):
    """the six maps of the fp64 restatement driven by the GPU models' logits: computed once, never written to"""
    out = UR.single_case([_member(_model(kind, seed, C)) for kind, seed in nets], _image(shape), STRIDE, STRIDE, PATCH,
                         weighting=blend.weighting, sigma_scale=blend.sigma_scale, mirror_axes=blend.mirror_axes)
    for a in out.values():
        a.setflags(write=False)
    return out


def _check_against_the_restatement(name, got, ref, C):
    assert got.label.dtype == torch.uint8 and all(t.is_cuda and t.dtype == torch.float32 for t in got[1:])
    assert tuple(got.prob.shape) == ref["prob"].shape and tuple(got.label.shape) == tuple(got.entropy.shape) == ref["label"].shape
    host = {k: getattr(got, k).cpu().numpy() for k in UR.MAPS}
    for k in UR.MAPS[1:]:
        print(f"{name} {k}: max |err| {np.abs(host[k] - ref[k]).max():.3e}, max {np.abs(ref[k]).max():.3e}")
        assert not np.isnan(host[k]).any()
    for k in ("prob",) + FLOAT_MAPS:
        np.testing.assert_allclose(host[k], ref[k], rtol=1e-4, atol=1e-5, err_msg=k)
    assert np.abs(host["mutual_info"] - ref["mutual_info"]).max() <= _mi_bound(C)
    top = np.sort(ref["prob"], 0)
    decided = top[-1] - top[-2] > 2.2e-4                                         # twice the bound on one probability
    assert decided.mean() > 0.99 and np.array_equal(host["label"][decided], ref["label"][decided])


CONFIGS = [("vnet", VOL, 2), ("unet_3D", THIN, 3)]
BLENDS = [Blend("constant"), Blend("gaussian"), Blend("gaussian", mirror_axes=(0, 2))]


@pytest.mark.parametrize("net_type,shape,C", CONFIGS, ids=["vnet-vol", "unet-thin"])
@pytest.mark.parametrize("blend", BLENDS, ids=["constant", "gaussian", "gaussian-mirror02"])
def test_one_model_gives_the_bits_of_the_classes_evaluator(net_type, shape, C, blend):
    model, image = _model(net_type, 3, C), _image(shape)
    got = U.single_case_uncertainty_device(model, image, STRIDE, STRIDE, PATCH, batch_size=5, blend=blend)
    label, prob = EC.single_case_classes_device(model, image, STRIDE, STRIDE, PATCH, batch_size=5, blend=blend)
    assert tuple(got.label.shape) == shape and tuple(got.prob.shape) == (C,) + shape
    assert torch.equal(got.label, label) and torch.equal(got.prob, prob)
    if blend == BLENDS[0]:                                                        # blend=None is Blend("constant")
        default = U.single_case_uncertainty_device(model, image, STRIDE, STRIDE, PATCH, batch_size=5)
        assert all(torch.equal(a, b) for a, b in zip(default, got))
        as_numpy = U.test_single_case_uncertainty([model], image, STRIDE, STRIDE, PATCH, batch_size=5)
        assert as_numpy.label.dtype == np.int64 and np.array_equal(as_numpy.label, label.cpu().numpy())
        assert np.array_equal(as_numpy.entropy, got.entropy.cpu().numpy())


@pytest.mark.parametrize("net_type,shape,C,blend", [("vnet", VOL, 2, BLENDS[2]), ("unet_3D", THIN, 3, BLENDS[1])],
                         ids=["vnet-vol-gaussian-mirror02", "unet-thin-gaussian"])
def test_single_case_matches_the_restatement(net_type, shape, C, blend):
    model = _model(net_type, 3, C)
    model.train()
    try:
        got = U.single_case_uncertainty_device(model, _image(shape), STRIDE, STRIDE, PATCH, batch_size=5, blend=blend)
        assert model.training                                                    # the model's mode is restored
    finally:
        model.eval()
    _check_against_the_restatement(f"{net_type} {shape} {blend}", got, _restated(((net_type, 3),), shape, C, blend), C)


def test_two_models_are_members():
    nets, blend = (("vnet", 3), ("vnet", 5)), BLENDS[1]
    models = [_model(*n) for n in nets]
    got = U.single_case_uncertainty_device(models, _image(THIN), STRIDE, STRIDE, PATCH, batch_size=4, blend=blend)
    ref = _restated(nets, THIN, 2, blend)
    _check_against_the_restatement(f"{nets} {blend}", got, ref, 2)
    assert ref["mutual_info"].max() > 1e-3                                       # two models disagree somewhere
    # the mean of softmaxes is not the softmax of mean logits (the `_plus` evaluators): the single model's maps differ
    one = U.single_case_uncertainty_device(models[0], _image(THIN), STRIDE, STRIDE, PATCH, batch_size=4, blend=blend)
    assert not torch.equal(one.prob, got.prob)


def _buffers(model):
    return {k: v.clone() for k, v in model.named_buffers()}


def test_monte_carlo_dropout():
    image = _image(THIN)
    vnet, unet = _model("vnet", 3), _model("unet_3D", 7)
    assert vnet.has_dropout and unet.has_dropout
    run = lambda m, seed, T=3: U.single_case_uncertainty_device(m, image, STRIDE, STRIDE, PATCH, batch_size=4, blend=BLENDS[1],   # noqa: E731
                                                                mc_passes=T, seed=seed)
    vnet.train()
    vnet.weights_static = False
    try:
        a, b, other = run(vnet, 11), run(vnet, 11), run(vnet, 12)
        assert vnet.training and vnet.weights_static is False                    # mode and weights_static are restored
    finally:
        vnet.eval()
    assert all(torch.equal(x, y) for x, y in zip(a, b))                          # the same seed gives the same bits
    assert not torch.equal(a.prob, other.prob) and not torch.equal(a.mutual_info, other.mutual_info)
    plain = run(vnet, 11, T=1)
    assert not torch.equal(plain.prob, a.prob)                                   # the masks were on
    assert float(a.mutual_info.max()) > 0
    for t in a[2:]:
        assert bool(torch.isfinite(t).all()) and float(t.min()) >= 0
    # BatchNorm (the U-Net's projection head) reads its running statistics and updates nothing
    names = [k for k, _ in unet.named_buffers()]
    assert any(k.endswith("running_mean") for k in names) and any(k.endswith("num_batches_tracked") for k in names)
    before = _buffers(unet)
    unet.train()
    try:
        maps = run(unet, 3)
        assert unet.training
    finally:
        unet.eval()
    after = _buffers(unet)
    assert all(torch.equal(before[k], after[k]) for k in names)
    assert bool(torch.isfinite(maps.entropy).all()) and float(maps.mutual_info.max()) > 0


def test_monte_carlo_needs_dropout_sites():
    model = VNet(n_channels=1, n_classes=2, has_dropout=False, dtype=torch.float32).to(DEV)
    with pytest.raises(ValueError, match="has_dropout"):
        U.single_case_uncertainty_device(model, _image(THIN), STRIDE, STRIDE, PATCH, mc_passes=2)
    with pytest.raises(ValueError, match="has_dropout"):
        U.single_case_uncertainty_device([_model("vnet", 3), torch.nn.Conv3d(1, 2, 1).to(DEV)], _image(THIN), STRIDE, STRIDE, PATCH,
                                         mc_passes=2)


def test_all_case_uncertainty():
    model = _model("vnet", 3)
    rng = np.random.default_rng(9)
    cases = [(_image(shape), (rng.random(shape) < 0.4).astype(np.uint8)) for shape in (VOL, THIN)]
    out = U.test_all_case_uncertainty(model, cases, 2, PATCH, STRIDE, STRIDE, blend=BLENDS[1], bins=15, uncertainty="entropy")
    assert len(out["per_case"]) == 2 and set(out["mean"]) == set(U.SCALARS)
    for k in ("ece", "brier", "nll", "error_auroc"):
        assert all(math.isfinite(c[k]) for c in out["per_case"]) and math.isfinite(out["mean"][k])
        assert out["mean"][k] == pytest.approx(np.mean([c[k] for c in out["per_case"]]), rel=1e-12)
    for (image, label), case in zip(cases, out["per_case"]):
        maps = U.single_case_uncertainty_device(model, image, STRIDE, STRIDE, PATCH, blend=BLENDS[1])
        direct = U.calibration(maps.prob, label, bins=15, uncertainty=maps.entropy)
        assert case["ece"] == direct["ece"] and case["n"] == label.size and case["error_auroc"] == direct["error_auroc"]
    with pytest.raises(ValueError, match="num_classes"):
        U.test_all_case_uncertainty(model, cases[:1], 3, PATCH, STRIDE, STRIDE)
