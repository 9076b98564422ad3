"""The model-ensemble sliding window on the MI355X (csrc/ensemble.hip, utils/ensemble_eval.py).

Yardsticks: oracle.evaluate.test_single_case fed a callable that averages two oracle nets' logits (the reference's lines :460-463) at
the bound tests/test_eval_gpu.py holds the single-model evaluator to; sliding_window.single_case_device for the self-ensemble (bit
equality: (a + a) / 2 == a); slices of the zero-padded volume for the gather (bit equality); a torch fp32 restatement for the
accumulate; the host path of test_all_case_plus for the device-resident one; apply_plan_host for the LA-order batch.

Case A: (40, 36, 20), windows (32, 32, 16), stride 16 / 4 -> 8 windows in chunks of 3 + 3 + 2, the last windows clamped.
Case B: (24, 40, 12), stride 8 / 4 -> 2 windows in one chunk of 4, padded on two axes."""
import functools

import numpy as np
import pytest
import torch

import device_cache_ref as R
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.dataloaders import DeviceVolumeCache, apply_plan_host, assemble_batch, draw_plan
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
from dycon_paper_replication_amd.utils import ensemble_eval as EE
from dycon_paper_replication_amd.utils import sliding_window as SW
from dycon_paper_replication_amd.utils import test_3d_patch as T3
from oracle import evaluate as OE
from oracle import nets as ON

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12                                     # tests/test_components_gpu.py: device_eval against test_3d_patch
PATCH = (32, 32, 16)
CASES = {"A": dict(shape=(40, 36, 20), sxy=16, sz=4, batch_size=3, windows=8),
         "B": dict(shape=(24, 40, 12), sxy=8, sz=4, batch_size=4, windows=2)}


def _image(shape):
    return np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _params(net_type, seed, C):
    return (ON.make_vnet_params if net_type == "vnet" else ON.make_unet_params)(seed, n_classes=C)


@functools.lru_cache(maxsize=None)
def _model(net_type, seed, C=2):
    model = net_factory_3d(net_type, 1, C, 2, dtype=torch.float32).to(DEV)
    model.load_state_dict(_params(net_type, seed, C))
    return model


@functools.lru_cache(maxsize=None)
def _oracle(case, pair):
    """(label, score) of the CPU restatement over the averaged logits: computed once, never written to"""
    c = CASES[case]

    def avg_logits(t):
        l, r = (ON.forward(kind, t, _params(kind, seed, 2), bn_training=False)[1] for kind, seed in pair)
        return (l + r) / 2                                                       # :460-462

    label, score = OE.test_single_case(avg_logits, _image(c["shape"]), c["sxy"], c["sz"], PATCH, num_classes=2)
    label.setflags(write=False)
    score.setflags(write=False)
    return label, score


@pytest.mark.parametrize("case,pair", [("A", (("vnet", 3), ("vnet", 5))), ("B", (("vnet", 3), ("vnet", 5))),
                                       ("B", (("vnet", 3), ("unet_3D", 7)))], ids=["A-vnets", "B-vnets", "B-vnet-unet"])
def test_ensemble_matches_the_oracle(case, pair):
    c = CASES[case]
    image = _image(c["shape"])
    assert len(T3._windows(tuple(max(s, p) for s, p in zip(c["shape"], PATCH)), PATCH, c["sxy"], c["sz"])) == c["windows"]
    lab_ref, score_ref = _oracle(case, pair)
    models = [_model(kind, seed) for kind, seed in pair]
    models[0].train()
    models[1].eval()
    lab, score = T3.test_single_case_plus(*models, image, c["sxy"], c["sz"], PATCH, num_classes=2, batch_size=c["batch_size"])
    assert lab.shape == lab_ref.shape == c["shape"] and lab.dtype == np.int64
    assert score.shape == score_ref.shape == (2,) + c["shape"] and score.dtype == np.float32
    assert np.array_equal(score[0], score[1])                                    # the reference's broadcast (:467-468)
    undecided = np.abs(score_ref[0] - 0.5) < 1e-4
    singles = [SW.single_case_device(m, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"])[0].cpu().numpy() for m in models]
    differ = [float((lab != s).mean()) for s in singles]
    print(f"case {case} {pair}: |score - oracle| {np.abs(score - score_ref).max():.3e}; undecided {undecided.mean():.5f}; "
          f"ensemble label != member label on {differ} of the voxels")
    np.testing.assert_allclose(score, score_ref, rtol=1e-4, atol=1e-5)
    assert undecided.mean() <= 0.005
    assert np.array_equal(lab[~undecided], lab_ref[~undecided])
    # a path that drops one model cannot pass.  CPU oracle: 15 % / 38 % (A) and 17 % / 33 % (B) for the V-Nets, 15 % / 17 % for the
    # V-Net / U-Net pair
    assert min(differ) > 0.05
    assert models[0].training and not models[1].training                         # every model's mode is restored


@pytest.mark.parametrize("case,net_type,C", [("A", "vnet", 2), ("B", "unet_3D", 3)], ids=["A-vnet-2", "B-unet-3"])
def test_self_ensemble_is_the_single_model_evaluator_bit_for_bit(case, net_type, C):
    c = CASES[case]
    image, m = _image(c["shape"]), _model(net_type, 3, C)
    label, prob = EE.single_case_plus_device(m, m, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"])
    ref_label, ref_prob = SW.single_case_device(m, image, c["sxy"], c["sz"], PATCH, batch_size=c["batch_size"])
    assert label.is_cuda and label.dtype == torch.uint8 and prob.is_cuda and prob.dtype == torch.float32
    assert tuple(label.shape) == tuple(prob.shape) == c["shape"]
    assert torch.equal(prob, ref_prob) and torch.equal(label, ref_label)
    assert 0 < int(label.sum()) < label.numel()


@pytest.mark.parametrize("shape,patch", [((24, 40, 12), (32, 32, 16)), ((13, 9, 7), (8, 8, 6)), ((5, 11, 3), (8, 6, 7))],
                         ids=["caseB", "no-pad", "odd-last-axis"])
def test_gather_equals_slices_of_the_padded_volume(shape, patch):
    vol = _image(shape)
    pads = EE._center_pads(shape, patch)
    padded = np.pad(vol, pads, mode="constant", constant_values=0)
    rng = np.random.default_rng(1)
    table = [tuple(int(rng.integers(0, padded.shape[a] - patch[a] + 1)) for a in range(3)) for _ in range(6)]
    table[0] = (0, 0, 0)
    table[-1] = tuple(padded.shape[a] - patch[a] for a in range(3))
    org = torch.tensor(table, dtype=torch.int32, device=DEV)
    dvol = torch.from_numpy(vol).to(DEV)
    stream = torch.cuda.current_stream().cuda_stream
    for first, n in ((0, 6), (2, 3), (5, 1)):                                    # the whole table; first > 0 and n < the table; the last
        out = torch.full((n + 1, 1) + patch, 7.0, dtype=torch.float32, device=DEV)
        _lib.call("dycon_sw_gather", dvol.data_ptr(), *shape, org.data_ptr(), len(table), first, n, *patch, out.data_ptr(), stream)
        want = np.stack([padded[x:x + patch[0], y:y + patch[1], z:z + patch[2]] for x, y, z in table[first:first + n]])[:, None]
        got = out.cpu().numpy()
        assert np.array_equal(got[:n], want)
        assert np.array_equal(got[:n], EE.gather_windows_host(vol, table[first:first + n], patch))
        assert (got[n] == 7.0).all()                                             # nothing behind the n windows is written
    with pytest.raises(_lib.DyconLibraryError, match="sw_gather"):
        _lib.call("dycon_sw_gather", dvol.data_ptr(), *shape, org.data_ptr(), len(table), 4, 3, *patch, out.data_ptr(), stream)


def _accumulate_restated(logits, origins, patch, vol):
    """torch fp32 on the device's inputs: mean logits in model order, softmax, class 1 into score, 1 into cnt, window by window"""
    x = logits[0] + logits[1]
    for l in logits[2:]:
        x = x + l
    p1 = torch.softmax(x / float(len(logits)), dim=-1)[..., 1]
    score, cnt = torch.zeros(vol, dtype=torch.float32), torch.zeros(vol, dtype=torch.float32)
    for n, (a, b, c) in enumerate(origins):
        sl = (slice(a, a + patch[0]), slice(b, b + patch[1]), slice(c, c + patch[2]))
        score[sl] += p1[n]
        cnt[sl] += 1
    return score, cnt


@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("M", [2, 3, 4])
def test_accumulate_ens_on_random_logits(M, C):
    patch, vol, origins = (8, 8, 4), (12, 8, 6), [(0, 0, 0), (4, 0, 2)]
    rng = np.random.default_rng(10 * M + C)
    logits = [torch.from_numpy((3.0 * rng.standard_normal((2,) + patch + (C,))).astype(np.float32)) for _ in range(M)]
    dev = [l.to(DEV) for l in logits]
    org = torch.tensor(origins, dtype=torch.int32, device=DEV)
    ptrs = [l.data_ptr() for l in dev] + [None] * (4 - M)
    runs = []
    for _ in range(2):
        score = torch.zeros(vol, dtype=torch.float32, device=DEV)
        cnt = torch.zeros_like(score)
        for _ in range(2):                                                       # two chunks: the maps accumulate
            _lib.call("dycon_sw_accumulate_ens", *ptrs, M, C, 2, *patch, org.data_ptr(), score.data_ptr(), cnt.data_ptr(), *vol,
                      torch.cuda.current_stream().cuda_stream)
        runs.append((score.cpu(), cnt.cpu()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    ref_score, ref_cnt = _accumulate_restated(logits, origins, patch, vol)
    assert torch.equal(runs[0][1], 2 * ref_cnt)
    assert set(ref_cnt.unique().tolist()) == {0.0, 1.0, 2.0}                     # uncovered, covered once, the overlap
    np.testing.assert_allclose(runs[0][0].numpy(), 2 * ref_score.numpy(), rtol=1e-4, atol=1e-5)


def _blob(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2


class _RuleNet(torch.nn.Module):
    """logit difference +1 where the image value is one of `values`, -3 elsewhere; a 2-tuple, as the reference's `_plus` models"""

    def __init__(self, values):
        super().__init__()
        self.values = values
        self.anchor = torch.nn.Parameter(torch.zeros(1))         # the evaluators take the device from the parameters

    def forward(self, x):
        hit = torch.zeros_like(x, dtype=torch.bool)
        for v in self.values:
            hit |= x == v
        d = torch.where(hit, 1.0, -3.0).to(x.dtype)
        return torch.cat([-d / 2, d / 2], 1), None


def test_all_case_plus_with_stub_models(tmp_path):
    """image values: 3 where both rules hold, 1 / 2 where one does.  Mean logit difference: +1 on 3, -1 on 1 and 2, -3 on 0: only the
    averaged logits give the intersection"""
    shape = (40, 40, 32)
    big, halo, small = _blob(shape, (14, 14, 14), 7), _blob(shape, (14, 14, 14), 10), _blob(shape, (32, 32, 24), 3)
    left = np.indices(shape)[0] < 14
    image = np.zeros(shape, np.float32)
    image[halo & left], image[halo & ~left] = 1, 2
    image[big | small] = 3
    net_l, net_r = _RuleNet((1, 3)).to(DEV), _RuleNet((2, 3)).to(DEV)
    kw = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    both, mask_l, mask_r = (big | small), (image == 1) | (image == 3), (image == 2) | (image == 3)
    u8 = lambda a: a.astype(np.uint8)                                            # noqa: E731
    lab, _ = T3.test_single_case_plus(net_l, net_r, image, 8, 8, (32, 32, 16), num_classes=2)
    assert np.array_equal(lab, both)
    for m, mask in ((net_l, mask_l), (net_r, mask_r)):                           # each member alone predicts its own rule
        assert np.array_equal(SW.single_case_device(_Second(m), image, 8, 8, (32, 32, 16))[0].cpu().numpy(), u8(mask))
    (tmp_path / "pred").mkdir()
    got = T3.test_all_case_plus(net_l, net_r, [(image, u8(both))], 2, test_save_path=str(tmp_path / "pred"), **kw)
    assert got[0] == 1.0 and got[1] == 1.0 and got[2] == 0.0 and got[3] == 0.0
    assert (tmp_path / "pred" / "performance.txt").read_text().startswith("average metric is")
    for mask in (mask_l, mask_r):
        assert T3.test_all_case_plus(net_l, net_r, [(image, u8(mask))], 2, **kw)[0] < 1.0
    plain = T3.test_all_case_plus(net_l, net_r, [(image, u8(big))], 2, **kw)
    nms = T3.test_all_case_plus(net_l, net_r, [(image, u8(big))], 2, nms=1, save_result=False, **kw)
    assert nms[0] == 1.0 and nms[2] == 0.0 and plain[0] < 1.0 and plain[2] > 10.0          # the far blob is gone
    empty = [(np.zeros(shape, np.float32), u8(big))]
    cases = [(image, u8(big)), (image, u8(_blob(shape, (16, 14, 14), 7))), empty[0]]
    for n in (0, 1):
        assert T3.test_all_case_plus(net_l, net_r, empty, 2, nms=n, **kw).tolist() == [0.0] * 4
        assert T3.test_all_case_plus(net_l, net_r, empty, 2, nms=n, device_resident=True, **kw).tolist() == [0.0] * 4
        host = T3.test_all_case_plus(net_l, net_r, cases, 2, nms=n, **kw)
        resident = T3.test_all_case_plus(net_l, net_r, cases, 2, nms=n, device_resident=True, batch_size=3, **kw)
        np.testing.assert_allclose(resident, host, rtol=RTOL, atol=0)
    spaced = T3.test_all_case_plus(net_l, net_r, [cases[1] + ((2.0, 2.0, 2.0),)], 2, nms=1, device_resident=True, **kw)
    unit = T3.test_all_case_plus(net_l, net_r, [cases[1]], 2, nms=1, device_resident=True, **kw)
    np.testing.assert_allclose(spaced[2:], 2.0 * unit[2:], rtol=1e-6)
    assert spaced[0] == unit[0]


class _Second(torch.nn.Module):
    """a `_plus` model (logits, features) behind the (tanh, logits, features) outputs the single-model evaluator unpacks"""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        logits, feats = self.net(x)
        return None, logits, feats


def test_var_all_case_LA_family(tmp_path, monkeypatch):
    """the LA validation loops (:28-49, :354-373) over a list file: the reference's two on-disk layouts, Dice 0 for an empty
    prediction, the sum over the number of listed cases.  h5py is absent, so the reader is replaced by a table keyed by the path."""
    shape = (40, 40, 32)
    big, halo = _blob(shape, (14, 14, 14), 7), _blob(shape, (14, 14, 14), 10)
    image = np.zeros(shape, np.float32)
    image[halo & (np.indices(shape)[0] < 14)], image[halo & (np.indices(shape)[0] >= 14)] = 1, 2
    image[big] = 3
    label = _blob(shape, (16, 14, 14), 7).astype(np.uint8)
    mask_l = (image == 1) | (image == 3)
    (tmp_path / "test.list").write_text("caseA\ncaseB\nempty\n")
    table = {}
    for folder in ("LA_data", "2018LA_Seg_Training Set"):
        for name, img in (("caseA", image), ("caseB", image[::-1].copy()), ("empty", np.zeros(shape, np.float32))):
            table[f"{tmp_path}/{folder}/{name}/mri_norm2.h5"] = (img, label if name != "caseB" else label[::-1].copy())
    read = []

    def fake_read_case(case, label_key):
        assert label_key == "label"
        read.append(case)
        return table[case]

    monkeypatch.setattr(T3, "_read_case", fake_read_case)
    dice = lambda p, g: 2.0 * (p & (g != 0)).sum() / (p.sum() + (g != 0).sum())      # noqa: E731
    net_l, net_r = _RuleNet((1, 3)).to(DEV), _RuleNet((2, 3)).to(DEV)
    kw = dict(patch_size=(32, 32, 16), stride_xy=8, stride_z=8)
    got = T3.var_all_case_LA(_Second(net_l), str(tmp_path), 2, **kw)
    assert read == [f"{tmp_path}/LA_data/{n}/mri_norm2.h5" for n in ("caseA", "caseB", "empty")]
    assert got == pytest.approx(2 * dice(mask_l, label) / 3, rel=1e-12) and 0 < got < 2 / 3
    del read[:]
    got = T3.var_all_case_LA_plus(net_l, net_r, 2, root_dir=str(tmp_path), **kw)
    assert read == [f"{tmp_path}/2018LA_Seg_Training Set/{n}/mri_norm2.h5" for n in ("caseA", "caseB", "empty")]
    assert got == pytest.approx(2 * dice(big, label) / 3, rel=1e-12) and got != pytest.approx(2 * dice(mask_l, label) / 3)


def test_la_order_batch_on_the_device():
    """one assemble_batch of a rot/flip-first plan: dycon_assemble_batch is unchanged, the mapped origins are what it executes"""
    patch, shapes = (12, 12, 8), [(23, 17, 12), (9, 20, 11), (16, 14, 9)]
    cases = R.make_cases(shapes, 23, image_dtype=np.float64)
    cache = DeviceVolumeCache(cases, device=DEV)
    images, labels = zip(*(cache.host_case(i) for i in range(len(cache))))
    np.random.seed(11)
    plan = draw_plan(cache.shapes, [0, 1, 2] * 6, patch, order="rotflip_crop")
    assert len({(int(k), int(a)) for k, a in zip(plan["k"], plan["flip_axis"])}) >= 6 and (plan["origin"] < 0).any()
    want = apply_plan_host(plan, images, labels)
    got = assemble_batch(cache, plan, label_dtype=torch.int64)
    assert np.array_equal(got["image"].cpu().numpy(), want["image"])
    assert np.array_equal(got["label"].cpu().numpy(), want["label"].astype(np.int64))
    np.random.seed(11)
    ref_i, ref_l = R.chain_batch(cases, [0, 1, 2] * 6, R.Compose([R.D.RandomRotFlip(), R.D.RandomCrop(patch), R.D.ToTensor()]))
    assert np.array_equal(got["image"].cpu().numpy(), ref_i) and np.array_equal(got["label"].cpu().numpy(), ref_l)
