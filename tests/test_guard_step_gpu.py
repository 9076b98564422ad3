"""Guard-band tests, whole paths: two eager training steps of every configuration, and one sliding-window evaluation, inside
tests/guard.py's guarded().  The trainer is constructed inside the block, so its flat parameter, teacher, gradient and momentum
arenas get bands as well as every activation, workspace, slab and packed weight of the step.  At the (48, 48, 32) patch the top
level runs the LDS / persistent convolutions (73 728 voxels) and the deeper levels gemm / tile / halo, down to a 3 x 3 x 2
bottleneck, where M = 18 B is far from a multiple of 64.

After each step check() must find every band intact; after the two steps the loss terms are finite, and they and the arenas agree
with the same two steps on ordinary tensors from the same seed to the 1e-6 relative bound of
test_trainer_gpu.test_checkpoint_resume_continues_the_run (the kernels are deterministic up to the double atomic loss sums)."""
import contextlib

import numpy as np
import pytest
import torch

from guard import guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PATCH = (48, 48, 32)
TERMS = ("loss", "ce", "dice", "cons", "fecl", "uncl")

# all labeled_bs = 1 of batch_size = 2, replay off (eager steps only)
CONFIGS = [
    ("vnet_bf16", dict(model="vnet")),
    ("vnet_fp32", dict(model="vnet", dtype=torch.float32)),
    ("unet_bf16", dict(model="unet_3D")),
    ("isles", dict(model="vnet", dice_variant="multiclass", teacher_mode="eval", poly_lr=True, feature_scaler=4)),
    ("classes3", dict(model="vnet", num_classes=3)),
    ("unet_aspp", dict(model="unet_3D", use_aspp=True)),
    ("gambling", dict(model="vnet", use_gambling=1)),
]


def _two_steps(kw, vol, lab, g=None, names=None):
    """two eager steps; with a Guard: inputs wrapped, check() after each step; with `names`: the launches captured as test_ledger
    captures them (the guarded run goes without, as production steps do)"""
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    from test_dispatch_parity_gpu import launched
    tr = DyconTrainer(TrainConfig(batch_size=2, labeled_bs=1, replay=False, **kw), DEV)
    if g is not None:
        vol, lab = g.wrap(vol), g.wrap(lab)
    checked = []
    with (launched(names) if names is not None else contextlib.nullcontext()):
        for _ in range(2):
            out = tr.step(vol, lab, epoch=0)
            torch.cuda.synchronize()
            if g is not None:
                checked.append(g.check())
    terms = {k: float(out[k]) for k in TERMS}
    return terms, {k: getattr(tr, k).clone() for k in ("flat_p", "flat_t", "flat_m")}, checked


@pytest.mark.parametrize("cid,kw", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_two_steps_guarded(cid, kw):
    from dycon_paper_replication_amd.synthetic import make_batch
    vol, lab, _ = make_batch(5, 2, PATCH)
    vol, lab = vol.to(DEV), lab.to(DEV)
    with guarded() as g:
        terms, flats, checked = _two_steps(kw, vol, lab, g)
    sites = g.sites()
    print(f"{cid}: guarded allocations checked after step 1 / 2: {checked}, from {len(sites)} call sites; terms {terms}")
    arenas = [s for s in sites if s.startswith("dycon_paper_replication_amd/trainer.py")]
    assert len(arenas) >= 4, f"the trainer's arenas were not guarded: {sorted(sites)}"
    names = set()
    terms0, flats0, _ = _two_steps(kw, vol, lab, names=names)
    print(f"{cid}: launched {sorted(names)}")
    for k in TERMS:
        assert np.isfinite(terms[k]), f"{cid}: {k} = {terms[k]} under the guard (ordinary tensors: {terms0[k]})" + \
            (": an out-of-bounds read reached the arithmetic" if np.isfinite(terms0[k]) else "")
        assert abs(terms[k] - terms0[k]) <= 1e-6 * abs(terms0[k]), f"{cid}: {k} {terms[k]!r} under the guard, {terms0[k]!r} without"
    for k, x in flats.items():
        assert bool(torch.isfinite(x).all()), f"{cid}: {k} holds NaN / Inf under the guard"
        assert float((x - flats0[k]).abs().max()) <= 1e-6 * float(flats0[k].abs().max()), f"{cid}: {k} differs from the unguarded run"


def test_single_case_guarded():
    """the evaluator on a (100, 97, 70) volume with (96, 96, 64) windows, strides (16, 4), four windows per batch: the score and count
    volumes, the label map and the last, clamped windows are banded; same label map as on ordinary tensors"""
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.utils import test_3d_patch as T3
    from test_dispatch_parity_gpu import launched
    torch.manual_seed(3)
    model = net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).cuda()
    image = np.random.default_rng(70).standard_normal((100, 97, 70)).astype(np.float32)
    names = set()
    with guarded() as g:
        with launched(names):            # (the first call packs the model's weights: pack_batch_kernel is launched under the guard)
            label, score = T3.test_single_case(model, image, 16, 4, (96, 96, 64), num_classes=2, batch_size=4)
    n = g.check()
    sites = g.sites()
    print(f"test_single_case: {n} guarded allocations checked, from {len(sites)} call sites; launched {sorted(names)}")
    assert any(s.startswith("dycon_paper_replication_amd/utils/sliding_window.py") for s in sites), sorted(sites)
    assert "pack_batch_kernel" in names          # (the module route's one-launch repack: test_guard_ops_gpu.REACHED_BY_A_GUARDED_PATH)
    label0, score0 = T3.test_single_case(model, image, 16, 4, (96, 96, 64), num_classes=2, batch_size=4)
    assert np.isfinite(score).all(), "NaN / Inf in the score map under the guard: an out-of-bounds read reached the arithmetic"
    assert label.shape == (100, 97, 70) and np.array_equal(label, label0)
    assert np.array_equal(score, score0)
