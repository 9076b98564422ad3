"""Guard-band tests of the warp / filter entry points: no kernel reads or writes outside its tensors.

Every test runs its call inside tests/guard.py's guarded(), in the manner of tests/test_guard_ops_gpu.py: the inputs are wrap()ped,
the cache arenas, outputs, workspaces and field buffers the package allocates get 0xFF bands too.  Then (a) check(): every band is
intact; (b) every floating-point result is finite (a read past the end that reaches the arithmetic meets NaN); (c) the same call on
ordinary tensors gives the same bits.  The shapes are the small ones of the parity tests: the corner index == n of the order-1 rule,
the halo reads of the filter (radius above the axis length, the largest radius) and the 16 + 1 split of the assembly launch."""
import numpy as np
import pytest
import torch

import warp_ref as WR
from guard import guarded

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd.dataloaders import DeviceBatchLoader, DeviceVolumeCache
    from dycon_paper_replication_amd.dataloaders import device_warp as W
    from dycon_paper_replication_amd.dataloaders.brats19 import TwoStreamBatchSampler
    from dycon_paper_replication_amd.utils import filters as F

DEV = "cuda:0"


def _run_both(run, what):
    """run(wrap) -> {name: tensor}: once under the guard, once on ordinary tensors; asserts (a), (b), (c)"""
    with guarded() as g:
        got = run(g.wrap)
    n = g.check()                                                                  # (a)
    print(f"{what}: {n} guarded allocations checked")
    plain = run(lambda t: t.clone())
    torch.cuda.synchronize()
    assert sorted(got) == sorted(plain) and n >= len(got)
    for k, a in got.items():
        if a.is_floating_point():
            assert bool(torch.isfinite(a).all()), f"{what} {k}: NaN / Inf under the guard"      # (b)
        assert torch.equal(a.view(torch.uint8), plain[k].view(torch.uint8)), f"{what} {k}"          # (c)
    return got


@pytest.mark.parametrize("mode", WR.GAUSS_MODES)
def test_gaussian_filter(mode):
    def run(wrap):
        out = {}
        for n, (shape, sigma) in enumerate(WR.GAUSS_CASES):
            x = wrap(torch.from_numpy(np.random.default_rng(n).standard_normal(shape).astype(np.float32)).to(DEV))
            out[f"c{n}"] = F.gaussian_filter(x, sigma, mode)
            y = wrap(x)
            out[f"c{n}.inplace"] = F.gaussian_filter(y, sigma, mode, out=y)
        return out
    got = _run_both(run, f"gaussian_filter {mode}")
    assert all(torch.equal(got[f"c{n}"], got[f"c{n}.inplace"]) for n in range(len(WR.GAUSS_CASES)))


@pytest.mark.parametrize("kind", WR.KINDS)
def test_assemble_batch_warp(kind):
    """17 samples (16 + 1), one-hot planes, the case smaller than the patch; `shift` puts integer coordinates on the edge n - 1,
    where the upper corner has the index n"""
    plan, disp = WR.make_plan(kind, 3, 17)

    def run(wrap):
        cache = DeviceVolumeCache(WR.cases(), device=DEV)                          # its arenas are torch.zeros: guarded
        d = None if disp is None else wrap(torch.from_numpy(disp).to(DEV))
        return W.assemble_batch_warp(cache, plan, displacement=d, label_dtype=torch.int64, onehot=3, onehot_dtype=torch.float32)
    got = _run_both(run, f"assemble_batch_warp {kind}")
    assert got["image"].any() and got["label"].any()


def test_warp_volume_and_intensity():
    rng = np.random.default_rng(3)
    v = rng.standard_normal((11, 10, 9))
    m, off = W.affine_of(1.1, (10, -15, 20), (1, 0, 2), (8, 8, 6))
    disp = rng.standard_normal((3, 8, 8, 6)).astype(np.float32)
    batch = rng.uniform(-0.1, 1.1, (18, 1, 5, 7, 3)).astype(np.float32)            # 18 samples: two launches

    def run(wrap):
        d = wrap(torch.from_numpy(disp).to(DEV))
        out = {}
        for name, a, order in (("f32", v.astype(np.float32), 1), ("f64", v, 1), ("u8", np.abs(4 * v).astype(np.uint8), 0),
                               ("i64", (4 * v).astype(np.int64), 0)):
            t = wrap(torch.from_numpy(a).to(DEV))
            out[name] = W.warp_volume(t, m, off, (8, 8, 6), order)
            out[name + ".disp"] = W.warp_volume(t, m, off, (8, 8, 6), order, d)
            out[name + ".edge"] = W.warp_volume(t, np.eye(3), (3, 2, 1), (8, 8, 8), order)       # coordinates n - 1 exactly
        x = wrap(torch.from_numpy(batch).to(DEV))
        out["intensity"] = W.intensity_augment(x, 1.2, 0.05, 0.8)
        out["intensity.subset"] = W.intensity_augment(x, 0.9, 0.0, 1.0, samples=[17, 0, 4])
        return out
    got = _run_both(run, "warp_volume / intensity_augment")
    ref = torch.from_numpy(v.astype(np.float32)[3:11, 2:10, 1:9]).to(DEV)          # z index 7 reads the coordinate 8 = n - 1 exactly
    assert torch.equal(got["f32.edge"], ref) and bool(ref[:, :, -1].all())


def test_elastic_field_and_loader():
    def run(wrap):
        out = {"field": W.elastic_field(3, WR.PATCH, [10.0, 20.0, 5.0], [1.0, 16.0, 2.5], seed=1, offset=7, device=DEV)}
        cache = DeviceVolumeCache(WR.cases(), device=DEV)
        np.random.seed(5)
        loader = DeviceBatchLoader(cache, TwoStreamBatchSampler([0, 1, 0, 1, 0, 1], [2], 3, 1), WR.PATCH, noise_sigma=0.1,
                                   warp=W.Warp(p_affine=1.0, p_elastic=0.7, alpha=(5.0, 20.0), sigma=(1.0, 2.0)),
                                   intensity=W.Intensity(p_gain=0.5, p_gamma=0.5, p_blur=0.7))
        for n, b in enumerate(loader):
            out.update({f"b{n}.{k}": v.clone() for k, v in b.items()})
        return out
    got = _run_both(run, "elastic_field / DeviceBatchLoader")
    assert "b2.image" in got
