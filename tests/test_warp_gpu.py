"""dycon_assemble_batch_warp / dycon_warp_volume / dycon_intensity_augment, elastic_field and the DeviceBatchLoader with warp and
intensity on the GPU: bit for bit against the numpy twins of dataloaders/device_warp.py (which tests/test_warp_cpu.py holds to
scipy) and, for single volumes, against scipy itself.  Gamma alone has a bound: one fp32 ulp."""
import functools

import numpy as np
import pytest
import torch
from scipy import ndimage

import warp_ref as WR
from dycon_paper_replication_amd import ops
from dycon_paper_replication_amd.dataloaders import DeviceBatchLoader, DeviceVolumeCache, assemble_batch, draw_plan
from dycon_paper_replication_amd.dataloaders import device_warp as W
from dycon_paper_replication_amd.dataloaders.brats19 import TwoStreamBatchSampler
from dycon_paper_replication_amd.dataloaders.device_cache import PLAN_DTYPE
from dycon_paper_replication_amd.utils.filters import gaussian_filter_host

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NP_OF = {torch.uint8: np.uint8, torch.int64: np.int64, torch.float32: np.float32}


@functools.lru_cache(maxsize=None)
def _cache():
    cache = DeviceVolumeCache(WR.cases(), device=DEV)
    host = [cache.host_case(i) for i in range(len(cache))]
    return cache, [h[0] for h in host], [h[1] for h in host]


@functools.lru_cache(maxsize=None)
def _twin(kind, B=len(WR.K_FLIP)):
    """the reference of a case, computed once and shared: (plan, displacement, twin outputs with onehot=3)"""
    _, images, labels = _cache()
    plan, disp = WR.make_plan(kind, 3, B)
    out = W.apply_warp_plan_host(plan, images, labels, disp, onehot=3)
    WR.check_band(out)
    return plan, disp, out


def _dev(disp):
    return None if disp is None else torch.from_numpy(disp).to(DEV)


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("kind", WR.KINDS)
def test_assemble_batch_warp_equals_the_twin(kind, label_dtype):
    """12 samples: every rot90 count with every flip, the three cases in turn (one smaller than the patch)"""
    cache = _cache()[0]
    plan, disp, ref = _twin(kind)
    out = W.assemble_batch_warp(cache, plan, displacement=_dev(disp), label_dtype=label_dtype)
    assert out["image"].dtype == torch.float32 and out["label"].dtype == label_dtype and "onehot_label" not in out
    assert WR.same_bits(out["image"].cpu().numpy(), ref["image"])
    assert np.array_equal(out["label"].cpu().numpy(), ref["label"].astype(NP_OF[label_dtype]))
    if kind == "shift":                                                # the identity: dycon_assemble_batch's bits, warped or not
        plain = np.zeros(len(plan), dtype=PLAN_DTYPE)
        for f in PLAN_DTYPE.names:
            plain[f] = plan[f]
        base = assemble_batch(cache, plain, label_dtype=label_dtype)
        idle = plan.copy()
        idle["warp"] = 0
        for got in (out, W.assemble_batch_warp(cache, idle, label_dtype=label_dtype)):
            assert torch.equal(got["image"].view(torch.int32), base["image"].view(torch.int32))
            assert torch.equal(got["label"], base["label"])


@pytest.mark.parametrize("onehot_dtype", W.ONEHOT_DTYPES, ids=["u8", "f32", "i64"])
def test_onehot_planes_from_the_same_launch(onehot_dtype):
    cache = _cache()[0]
    plan, disp, ref = _twin("general_disp")
    out = W.assemble_batch_warp(cache, plan, displacement=_dev(disp), onehot=3, onehot_dtype=onehot_dtype)
    assert out["onehot_label"].dtype == onehot_dtype and tuple(out["onehot_label"].shape) == ref["onehot_label"].shape
    assert np.array_equal(out["onehot_label"].cpu().numpy(), ref["onehot_label"].astype(NP_OF[onehot_dtype]))
    assert WR.same_bits(out["image"].cpu().numpy(), ref["image"]) and np.array_equal(out["label"].cpu().numpy(), ref["label"])
    assert ref["onehot_label"].sum(axis=1).max() == 1 and ref["onehot_label"][:, 1:].any()


def test_seventeen_samples_take_two_launches():
    """16 + 1: the displacement, the image, the label and the one-hot planes of the second launch start at sample 16"""
    cache = _cache()[0]
    plan, disp, ref = _twin("general_disp", 17)
    assert plan["elastic"][16] == 1
    out = W.assemble_batch_warp(cache, plan, displacement=_dev(disp), label_dtype=torch.int64, onehot=3, onehot_dtype=torch.uint8)
    assert WR.same_bits(out["image"].cpu().numpy(), ref["image"])
    assert np.array_equal(out["label"].cpu().numpy(), ref["label"].astype(np.int64))
    assert np.array_equal(out["onehot_label"].cpu().numpy(), ref["onehot_label"])
    # writing into given tensors allocates nothing and gives the same bits
    again = W.assemble_batch_warp(cache, plan, out={k: torch.zeros_like(v) for k, v in out.items()}, displacement=_dev(disp),
                                  label_dtype=torch.int64, onehot=3, onehot_dtype=torch.uint8)
    assert all(torch.equal(again[k], out[k]) for k in out)


def test_vector_stores_when_the_patch_allows():
    """patch (8, 8, 8): 16-byte stores of images, labels and planes; the twin is the reference"""
    cache, images, labels = _cache()
    rng = np.random.default_rng(8)
    plan = np.zeros(4, dtype=W.WARP_PLAN_DTYPE)
    for n in range(4):
        origin = rng.integers(-1, 3, 3)
        m, off = W.affine_of(rng.uniform(0.8, 1.25), rng.uniform(-20, 20, 3), origin, (8, 8, 8))
        plan[n] = (n % 3, origin, n, n % 3 - 1, (8, 8, 8), 1, m.reshape(9), off, 1, (0, 0, 0), n & 1, 0, 0, 1, 0, 1, 0)
    disp = (1.5 * rng.standard_normal((4, 3, 8, 8, 8))).astype(np.float32)
    ref = W.apply_warp_plan_host(plan, images, labels, disp, onehot=3)
    WR.check_band(ref)
    out = W.assemble_batch_warp(cache, plan, displacement=_dev(disp), onehot=3, onehot_dtype=torch.float32)
    assert WR.same_bits(out["image"].cpu().numpy(), ref["image"]) and np.array_equal(out["label"].cpu().numpy(), ref["label"])
    assert np.array_equal(out["onehot_label"].cpu().numpy(), ref["onehot_label"].astype(np.float32))


@pytest.mark.parametrize("with_disp", [False, True], ids=["affine", "coords"])
def test_warp_volume_equals_scipy(with_disp):
    """order 1 on fp32 and fp64, order 0 on every dtype offered, against scipy itself; a volume smaller than the output, integer
    coordinates that hit the edge n - 1, a general matrix"""
    rng = np.random.default_rng(13)
    inside = total = 0
    for n, shape, kind in (((11, 10, 9), (8, 8, 6), "general"), ((5, 4, 3), (7, 6, 9), "integer"), ((20, 17, 12), (9, 33, 5), "general"),
                           ((8, 8, 5), (8, 8, 6), "scale")):
        if kind == "integer":
            m, off = np.eye(3), np.array([-1.0, 0.0, -2.0])
        elif kind == "scale":
            m, off = np.diag(rng.uniform(0.8, 1.25, 3)), rng.uniform(-1, 1, 3)
        else:
            m, off = W.affine_of(rng.uniform(0.8, 1.25), rng.uniform(-20, 20, 3), rng.integers(0, 3, 3), shape)
        disp = (1.5 * rng.standard_normal((3,) + shape)).astype(np.float32) if with_disp else None
        v = rng.standard_normal(n)
        arrays = [(v.astype(np.float32), 1), (v, 1)] + [(np.abs(4 * v).astype(dt), 0) for dt in (np.uint8, np.float32, np.float64, np.int64)]
        arrays.append((v > 0, 0))
        for a, order in arrays:
            if disp is None:
                ref = ndimage.affine_transform(a, m, off, output_shape=shape, order=order, mode="constant", cval=0)
            else:
                ref = ndimage.map_coordinates(a, W.source_coordinates(m, off, shape, disp), order=order, mode="constant", cval=0)
            got = W.warp_volume(torch.from_numpy(a).to(DEV), m, off, shape, order, _dev(disp))
            assert got.dtype == torch.from_numpy(a).dtype and tuple(got.shape) == shape
            assert WR.same_bits(got.cpu().numpy(), ref), (n, shape, a.dtype, order)
            assert WR.same_bits(W.warp_volume_host(a, m, off, shape, order, disp), ref)
        ins = W.warp_volume_host(np.ones(n, np.uint8), m, off, shape, 0, disp)
        inside, total = inside + int(ins.sum()), total + ins.size
    assert 0.2 * total < inside < 0.95 * total


def test_elastic_field_is_smoothed_philox_noise():
    """alpha[n] * gaussian_filter(noise[n], sigma[n], mode='constant') of the noise read back from the same seed and offset -- the
    twin's bits and scipy's -- and two calls give the same bits"""
    B, patch, alpha, sigma = 3, (8, 8, 6), [12.0, 0.0, 30.5], [1.5, 2.0, 3.0]
    field = W.elastic_field(B, patch, alpha, sigma, seed=7, offset=5 << 32, device=DEV)
    noise = W.elastic_noise(B, patch, 7, 5 << 32, device=DEV)
    assert torch.equal(noise, ops.add_noise(torch.zeros_like(noise), None, 1.0, float("inf"), 7, 5 << 32))
    nz = noise.cpu().numpy()
    assert abs(nz.mean()) < 0.1 and 0.9 < nz.std() < 1.1 and np.isfinite(nz).all()
    for n in range(B):
        ref = np.float32(alpha[n]) * gaussian_filter_host(nz[n], sigma[n], "constant")
        sp = np.float32(alpha[n]) * np.stack([ndimage.gaussian_filter(v, sigma[n], mode="constant") for v in nz[n]])
        assert WR.same_bits(ref, sp)
        assert WR.same_bits(field[n].cpu().numpy(), ref)
    assert float(field[0].abs().max()) > 0.5 and not field[1].any()
    again = W.elastic_field(B, patch, alpha, sigma, seed=7, offset=5 << 32, device=DEV)
    assert torch.equal(again.view(torch.int32), field.view(torch.int32))
    other = W.elastic_field(B, patch, alpha, sigma, seed=7, offset=6 << 32, device=DEV)
    assert not torch.equal(other[0], field[0])


def test_intensity_gamma_one_is_exact():
    rng = np.random.default_rng(17)
    x = rng.uniform(-0.2, 1.2, (3, 1, 9, 7, 5)).astype(np.float32)
    par = [(1.2, -0.05, 1.0, 0.0, 1.0), (0.8, 0.1, 1.0, -0.5, 2.0), (1.0, 0.0, 1.0, 0.1, 0.9)]
    t = torch.from_numpy(x).to(DEV)
    got = W.intensity_augment(t, *[[p[i] for p in par] for i in range(5)])
    ref = np.stack([W.intensity_host(x[n], *par[n]) for n in range(3)])
    assert WR.same_bits(got.cpu().numpy(), ref)
    assert (ref == 0).any() and (ref == 1).any() and len(np.unique(ref)) > 400          # clipped at both ends, and not only clipped
    # a subset, in place: the others are not touched
    y = t.clone()
    assert W.intensity_augment(y, 1.2, -0.05, 1.0, samples=[2], out=y) is y
    assert torch.equal(y[:2], t[:2]) and WR.same_bits(y[2].cpu().numpy(), W.intensity_host(x[2], 1.2, -0.05))


@pytest.mark.parametrize("gamma", [0.7, 1.5])
def test_intensity_gamma_within_one_ulp(gamma):
    """the device's double pow is not libm's; both are accurate to a few fp64 ulp, so after the final rounding to fp32 the two can
    differ only across one fp32 rounding boundary"""
    x = np.random.default_rng(19).uniform(-0.1, 1.1, (2, 1, 16, 16, 16)).astype(np.float32)
    got = W.intensity_augment(torch.from_numpy(x).to(DEV), 1.1, 0.02, gamma).cpu().numpy()
    ref = W.intensity_host(x, 1.1, 0.02, gamma)
    d = WR.ulp_distance(got, ref)
    print(f"gamma {gamma}: {int((d > 0).sum())} of {d.size} voxels differ, largest distance {int(d.max())} ulp")
    assert np.isfinite(got).all() and d.max() <= 1
    assert not np.array_equal(ref, W.intensity_host(x, 1.1, 0.02, 1.0))


def _sampler():
    return TwoStreamBatchSampler([0, 1, 0, 1, 0, 1], [2], 3, 1)          # three batches an epoch


def _loader(cache, **kw):
    return DeviceBatchLoader(cache, _sampler(), WR.PATCH, **kw)


def test_loader_end_to_end_equals_the_twin_chain():
    """three seeded batches with warp, intensity and noise: the twin chain on host copies of the cache, given the same plans and
    the field read back; gamma samples within one ulp before the noise is added, everything else bit for bit"""
    cache, images, labels = _cache()
    warp = W.Warp(p_affine=0.8, p_elastic=0.6, alpha=(5.0, 20.0), sigma=(1.0, 2.0))
    inten = W.Intensity(p_gain=0.5, p_bias=0.5, p_gamma=0.5, p_blur=0.5, range=(-1.0, 1.5))
    kw = dict(warp=warp, intensity=inten, aug_seed=3, onehot=3, onehot_dtype=torch.uint8)
    np.random.seed(21)
    plans = list(_loader(cache, **kw).plans())[:3]
    np.random.seed(21)
    loader, seen = _loader(cache, **kw), {"elastic": 0, "blur": 0, "gamma": 0, "gain": 0, "plain": 0}
    kept = []
    for n, batch in zip(range(3), loader):
        plan = plans[n]
        kept.append((batch, {k: v.clone() for k, v in batch.items()}))
        field = W.elastic_field(len(plan), WR.PATCH, np.where(plan["elastic"] != 0, plan["alpha"], 0.0),
                                np.where(plan["elastic"] != 0, plan["sigma"], 1.0), 3, n << 32, device=DEV).cpu().numpy()
        ref = W.apply_warp_plan_host(plan, images, labels, field, onehot=3)
        img = ref["image"]
        for s, rec in enumerate(plan):
            if rec["blur_sigma"] > 0:
                img[s, 0] = gaussian_filter_host(img[s, 0], rec["blur_sigma"])
            if rec["gain"] != 1 or rec["bias"] != 0 or rec["gamma"] != 1:
                img[s, 0] = W.intensity_host(img[s, 0], rec["gain"], rec["bias"], rec["gamma"], -1.0, 1.5)
            d = WR.ulp_distance(batch["image"][s].cpu().numpy(), img[s])
            assert d.max() <= (1 if rec["gamma"] != 1 else 0), (n, s, int(d.max()))
            seen["elastic"] += int(rec["elastic"]); seen["blur"] += int(rec["blur_sigma"] > 0); seen["gamma"] += int(rec["gamma"] != 1)
            seen["gain"] += int(rec["gain"] != 1); seen["plain"] += int(rec["gamma"] == 1)
        assert np.array_equal(batch["label"].cpu().numpy(), ref["label"])
        assert np.array_equal(batch["onehot_label"].cpu().numpy(), ref["onehot_label"])
    assert all(v > 0 for v in seen.values()), seen
    # the ring: batch 1 is intact after batch 2 was produced, and batch 2 went into batch 0's buffers
    assert all(torch.equal(kept[1][0][k], kept[1][1][k]) for k in kept[1][1])
    assert all(kept[2][0][k].data_ptr() == kept[0][0][k].data_ptr() for k in kept[0][1])
    # a second loader from the same seeds gives the same bits: the field comes from (aug_seed, batch number) alone
    np.random.seed(21)
    for n, batch in zip(range(3), _loader(cache, **kw)):
        if n == 2:
            assert all(torch.equal(batch[k], kept[2][0][k]) for k in batch)


def test_loader_with_noise_keeps_the_ring():
    """noise_sigma after the intensity step: the noisy image equals ops.add_noise of the noise-free chain"""
    cache = _cache()[0]
    kw = dict(warp=W.Warp(p_affine=1.0), intensity=W.Intensity(p_gain=1.0))
    np.random.seed(22)
    clean = [{k: v.clone() for k, v in b.items()} for _, b in zip(range(3), _loader(cache, **kw))]
    np.random.seed(22)
    got = []
    for n, b in zip(range(3), _loader(cache, noise_sigma=0.1, noise_seed=9, **kw)):
        got.append(b)
        assert torch.equal(b["image"], ops.add_noise(clean[n]["image"], None, 0.1, 0.2, 9, n << 32))
        assert torch.equal(b["label"], clean[n]["label"])
    assert got[2]["image"].data_ptr() == got[0]["image"].data_ptr() != got[1]["image"].data_ptr()


def test_default_loader_equals_assemble_batch():
    cache = _cache()[0]
    np.random.seed(23)
    plans = [draw_plan(cache.shapes, [int(i) for i in b], WR.PATCH) for b in _sampler()][:2]
    np.random.seed(23)
    loader = _loader(cache)
    assert loader._aug is None
    for plan, batch in zip(plans, loader):
        ref = assemble_batch(cache, plan)
        assert sorted(batch) == ["image", "label"]
        assert torch.equal(batch["image"].view(torch.int32), ref["image"].view(torch.int32)) and torch.equal(batch["label"], ref["label"])
