"""TrainConfig(num_classes=C) on the GPU: the C-class one-pass voxel losses against the reference (tests/golden/voxel_losses_nc.npz,
made by tests/golden/make_golden_trainer_nc.py), the 3-class trainer against the reference's ISLES trace (step_isles_nc3.npz), replay
against eager with every schedule scalar moving, bf16 against the fp32 mode, and the untouched 2-class launch list."""
import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import ops
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    from dycon_paper_replication_amd.utils import losses as UL
from oracle import nets as ON
from test_engine_gpu import within_budget

DEV = "cuda:0"
T = torch.from_numpy
KEYS = ("loss", "ce", "dice", "cons", "fecl", "uncl")
NEW_NAMES = ("dycon_seg_lossesc_fwd", "dycon_seg_lossesc_bwd", "dycon_seg_lossesc_finalize", "dycon_step_lossesc")
# (value rtol, value atol, gradient rtol, gradient atol) of tests/test_ops_gpu.py::test_voxel_losses_golden / test_uncl_golden
TOL = {"ce": (1e-5, 1e-6, 1e-4, 1e-8), "dice": (1e-5, 1e-6, 1e-4, 1e-8), "dice_mc": (1e-5, 1e-6, 1e-4, 1e-8),
       "cons_mse": (1e-5, 1e-7, 1e-4, 1e-9), "cons_kl": (1e-4, 1e-7, 1e-4, 1e-9),
       "uncl0": (1e-5, 1e-6, 1e-4, 1e-8), "uncl1": (1e-5, 1e-6, 1e-4, 1e-8)}
VAL_SLOT = {"ce": 0, "dice": 1, "dice_mc": 2, "cons_mse": 3, "cons_kl": 4, "uncl0": 5, "uncl1": 5}
COEF_SLOT = {"ce": 0, "dice": 1, "dice_mc": 2, "cons_mse": 3, "cons_kl": 3, "uncl0": 4, "uncl1": 4}
CASES = ("c3", "c4", "c5", "c8", "c4_absent", "c5_large")


def nd(t):
    """NCDHW cpu -> NDHWC cuda"""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV, torch.float32)


def nc(t):
    """NDHWC cuda -> NCDHW cpu"""
    return t.float().cpu().permute(0, 4, 1, 2, 3).contiguous()


def _stats(t):
    t = t.detach().double().cpu()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def draw(seed, shape, classes, absent=None):
    """the fixture's inputs (make_golden_trainer_nc.draw): default_rng(seed) -> a, b at scale 2.0, then the labels"""
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((3, classes) + tuple(shape)) * 2.0).astype(np.float32)
    b = (rng.standard_normal((3, classes) + tuple(shape)) * 2.0).astype(np.float32)
    present = np.array([c for c in range(classes) if c != absent])
    lab = present[rng.integers(0, len(present), (3,) + tuple(shape))].astype(np.int64)
    return T(a), T(b), T(lab)


def _case(g, tag):
    C, absent = int(g[f"{tag}.classes"]), int(g[f"{tag}.absent"])
    a, b, lab = draw(int(g[f"{tag}.seed"]), [int(v) for v in g[f"{tag}.shape"]], C, None if absent < 0 else absent)
    np.testing.assert_allclose(_stats(a), g[f"{tag}.a_stats"], rtol=1e-12)          # the fixture's draws
    np.testing.assert_allclose(_stats(b), g[f"{tag}.b_stats"], rtol=1e-12)
    assert np.array_equal(np.bincount(lab.numpy().reshape(-1), minlength=C), g[f"{tag}.label_counts"])
    return a, b, lab, C


def _tol(g, tag, term, k):
    """the issue's tolerances, x k for the fast sequences; twice the reference's own fp32 distance where that is larger"""
    vr, va, gr, ga = TOL[term]
    dv, dg = g[f"{tag}.{term}.fp32_dist"]
    return k * max(vr, 2 * float(dv)), va, k * max(gr, 2 * float(dg)), k * ga


def _check_grad(g, tag, term, got, rtol, atol):
    got = got.double().numpy()
    if f"{tag}.{term}_grad.f64" in g.files:
        np.testing.assert_allclose(got, g[f"{tag}.{term}_grad.f64"], rtol=rtol, atol=atol, err_msg=f"{tag} {term} gradient")
        return
    # the large case: every 8th voxel per axis element-wise, and the three sums over ALL elements.  With |x - r| <= rtol |r| + atol
    # per element: |sum x - sum r| and |sum |x| - sum |r|| <= rtol S1 + n atol, |sum x^2 - sum r^2| <= (2 + rtol) rtol S2 + 2 atol (1 + rtol) S1
    np.testing.assert_allclose(got[..., ::8, ::8, ::8], g[f"{tag}.{term}_grad_sub.f64"], rtol=rtol, atol=atol, err_msg=f"{tag} {term} gradient (sub-sample)")
    s, r = _stats(torch.from_numpy(got)), g[f"{tag}.{term}_grad_stats.f64"]
    print(f"{tag} {term} gradient statistics: got {s}, fp64 {r}")
    lin = rtol * r[1] + got.size * atol
    assert abs(s[0] - r[0]) <= lin and abs(s[1] - r[1]) <= lin, f"{tag} {term} gradient sums: {s} vs {r}"
    assert abs(s[2] - r[2]) <= (2 + rtol) * rtol * r[2] + 2 * atol * (1 + rtol) * r[1], f"{tag} {term} gradient square sum: {s[2]} vs {r[2]}"


@pytest.mark.parametrize("fast", [False, True], ids=["libm", "fast"])
@pytest.mark.parametrize("tag", CASES)
def test_kernel_vs_reference(tag, fast):
    """(a) CE / Dice on the labelled split LB = 1 of 3, the consistency terms with LB = 0, UnCL at both betas; the c4 case with uint8
    labels.  Values and gradients against the reference's fp64 twin."""
    g = load_golden("voxel_losses_nc")
    a, b, lab, C = _case(g, tag)
    s, t = nd(a), nd(b)
    labd = lab.to(DEV).to(torch.uint8) if tag == "c4" else lab.to(DEV)
    B, V, LB = 3, a[0, 0].numel(), int(g["LB"])
    k = 10.0 if fast else 1.0
    betas = [float(v) for v in g["betas"]]
    assert ops.seg_lossesc_nsums(C) == 5 + 3 * C

    def check(term, vals, grad_fn):
        vr, va, gr, ga = _tol(g, tag, term, k)
        ref = float(g[f"{tag}.{term}.f64"])
        print(f"{tag} {term}: got {float(vals[VAL_SLOT[term]]):.9g}, fp64 {ref:.9g}, reference fp32 {float(g[f'{tag}.{term}']):.9g}")
        np.testing.assert_allclose(float(vals[VAL_SLOT[term]]), ref, rtol=vr, atol=va, err_msg=f"{tag} {term}")
        _check_grad(g, tag, term, nc(grad_fn()), gr, ga)

    def coef(term):
        c = torch.zeros(5, device=DEV)
        c[COEF_SLOT[term]] = 1
        return c

    # labelled terms (the unlabelled samples feed the consistency sums, which are not read here)
    sums = ops.seg_lossesc_fwd(s, t, labd, LB, betas[0], fast=fast)
    vals = ops.seg_lossesc_finalize(sums, B, LB, V, C, betas[0])
    for term in ("ce", "dice", "dice_mc"):
        check(term, vals, lambda: ops.seg_lossesc_bwd(s, t, labd, LB, betas[0], sums, coef(term), 0, fast=fast))
    # consistency and UnCL over all three samples
    for i, beta in enumerate(betas):
        sums = ops.seg_lossesc_fwd(s, t, labd, 0, beta, fast=fast)
        vals = ops.seg_lossesc_finalize(sums, B, 0, V, C, beta)
        check(f"uncl{i}", vals, lambda: ops.seg_lossesc_bwd(s, t, labd, 0, beta, sums, coef("uncl0"), 0, fast=fast))
        if i == 0:
            check("cons_mse", vals, lambda: ops.seg_lossesc_bwd(s, t, labd, 0, beta, sums, coef("cons_mse"), 0, fast=fast))
            check("cons_kl", vals, lambda: ops.seg_lossesc_bwd(s, t, labd, 0, beta, sums, coef("cons_kl"), 1, fast=fast))
            # a forward asked for ONE kind accumulates that kind only, to the same bits per element (the atomics' order aside)
            for kind, slot, other in ((0, 3, 4), (1, 4, 3)):
                one = ops.seg_lossesc_finalize(ops.seg_lossesc_fwd(s, t, labd, 0, beta, kind, fast=fast), B, 0, V, C, beta)
                assert float(one[other]) == 0.0
                np.testing.assert_allclose(float(one[slot]), float(vals[slot]), rtol=1e-6)


@pytest.mark.parametrize("fast", [False, True], ids=["libm", "fast"])
def test_two_classes_cross_check(fast):
    """(b) the C-class kernels at C = 2 on the 2-class reference fixture, at tests/test_ops_gpu.py::test_voxel_losses_golden's tolerances"""
    g = load_golden("voxel_losses")
    a, b, lab = T(g["a"]), T(g["b"]), T(g["label"])
    B, V = a.shape[0], a[0, 0].numel()
    k = 10.0 if fast else 1.0
    s, t, labd = nd(a), nd(b), lab.to(DEV)
    sums = ops.seg_lossesc_fwd(s, t, labd, B, 1.0, fast=fast)
    vals = ops.seg_lossesc_finalize(sums, B, B, V, 2, 1.0).cpu().numpy()
    np.testing.assert_allclose(vals[0], g["ce"], rtol=k * 1e-5, atol=1e-6)
    np.testing.assert_allclose(vals[1], g["dice"], rtol=k * 1e-5, atol=1e-6)
    np.testing.assert_allclose(vals[2], g["dice_mc"], rtol=k * 1e-5, atol=1e-6)
    for j, key in ((0, "ce_grad"), (1, "dice_grad"), (2, "dice_mc_grad")):
        coef = torch.zeros(5, device=DEV)
        coef[j] = 1
        got = nc(ops.seg_lossesc_bwd(s, t, labd, B, 1.0, sums, coef, fast=fast)).numpy()
        np.testing.assert_allclose(got, g[key], rtol=k * 1e-4, atol=k * 1e-8, err_msg=key)
    lab8 = labd.to(torch.uint8)
    sums = ops.seg_lossesc_fwd(s, t, lab8, 0, 1.0, fast=fast)
    vals = ops.seg_lossesc_finalize(sums, B, 0, V, 2, 1.0).cpu().numpy()
    np.testing.assert_allclose(vals[3], g["cons_mse"], rtol=k * 1e-5, atol=1e-7)
    np.testing.assert_allclose(vals[4], g["cons_kl"], rtol=k * 1e-4, atol=1e-7)
    coef = torch.tensor([0, 0, 0, 1.0, 0], device=DEV)
    for kind, key in ((0, "cons_mse_grad"), (1, "cons_kl_grad")):
        got = nc(ops.seg_lossesc_bwd(s, t, lab8, 0, 1.0, sums, coef, kind, fast=fast)).numpy()
        np.testing.assert_allclose(got, g[key], rtol=k * 1e-4, atol=k * 1e-9, err_msg=key)


def test_fused_voxel_losses_three_classes_autograd():
    """utils.losses.fused_voxel_losses dispatches on shape[1] and stays differentiable: d(sum_k w_k vals_k)/da against the weighted
    sum of the fixture's gradients"""
    g = load_golden("voxel_losses_nc")
    a, b, lab, C = _case(g, "c3")
    beta, LB = float(g["betas"][0]), int(g["LB"])
    x = a.to(DEV).requires_grad_(True)
    # CE / Dice from the labelled split; the consistency terms and UnCL of the fixture are over all samples (LB = 0)
    w_lab, w_all = {"ce": 0.7, "dice": 1.3, "dice_mc": 0.9}, {"cons_mse": 2.0, "cons_kl": 0.5, "uncl0": 1.1}
    v_lab = UL.fused_voxel_losses(x, b.to(DEV), lab.to(DEV), LB, beta)
    v_all = UL.fused_voxel_losses(x, b.to(DEV), lab.to(DEV), 0, beta)
    assert v_lab.shape == (6,)
    total = sum(w * v_lab[VAL_SLOT[k]] for k, w in w_lab.items()) + sum(w * v_all[VAL_SLOT[k]] for k, w in w_all.items())
    ref = sum(w * float(g[f"c3.{k}.f64"]) for k, w in {**w_lab, **w_all}.items())
    w = {**w_lab, **w_all}
    # every term at its own tolerance, weighted and summed (the terms' gradients may cancel: no relative bound on the sum itself)
    np.testing.assert_allclose(float(total.detach()), ref, rtol=0, atol=sum(wk * (TOL[k][0] * abs(float(g[f"c3.{k}.f64"])) + TOL[k][1]) for k, wk in w.items()))
    (gx,) = torch.autograd.grad(total, x)
    grads = {k: g[f"c3.{k}_grad.f64"].astype(np.float64) for k in w}
    gref = sum(wk * grads[k] for k, wk in w.items())
    bound = sum(wk * (TOL[k][2] * np.abs(grads[k]) + TOL[k][3]) for k, wk in w.items())
    err = np.abs(gx.double().cpu().numpy() - gref)
    assert (err <= bound).all(), f"gradient off by up to {float((err / bound).max()):.2f} x the bound"
    assert float(UL.cross_entropy_from_logits(a[:1].to(DEV), lab[:1].to(DEV))) == pytest.approx(float(g["c3.ce.f64"]), rel=1e-5)


# ------------------------------------------------------------------------------------------------------ (c) trainer vs the reference
def _nc3(kind):
    return {k[len(kind) + 1:]: v for k, v in load_golden("step_isles_nc3").items() if k.startswith(kind + ".")}


def _nc3_trainer(g, kind, dtype=torch.float32, overlap=True):
    net_type = "unet_3D" if kind == "unet" else "vnet"
    mk = ON.make_unet_params if kind == "unet" else ON.make_vnet_params
    s0, s1 = [int(v) for v in g["seeds"]]
    NC = int(g["classes"])
    cfg = TrainConfig(model=net_type, num_classes=NC, labeled_bs=int(g["LB"]), batch_size=int(g["B"]), dtype=dtype, feature_scaler=2,
                      dice_variant="multiclass", poly_lr=True, base_lr=float(g["base_lr"]), max_iterations=int(g["max_iterations"]),
                      overlap_teacher=overlap, overlap_wgrad=overlap, overlap_features=overlap)
    return DyconTrainer(cfg, DEV, student_init=mk(s0, n_classes=NC), teacher_init=mk(s1, n_classes=NC)), mk, s0, NC


def _nc3_batches(g):
    """volumes and noise from rng_seed exactly as the fixture drew them (per step: volume, then noise), checked against its statistics"""
    B, S = int(g["B"]), int(g["S"])
    rng = np.random.default_rng(int(g["rng_seed"]))
    for step in range(2):
        vol = T(rng.standard_normal((B, 1, S, S, S)).astype(np.float32))
        noise = torch.clamp(T(rng.standard_normal((B, 1, S, S, S)).astype(np.float32)) * 0.1, -0.2, 0.2)
        np.testing.assert_allclose(_stats(vol), g[f"s{step}.vol_stats"], rtol=1e-12)
        np.testing.assert_allclose(_stats(noise), g[f"s{step}.noise_stats"], rtol=1e-12)
        yield step, vol.to(DEV), T(g[f"s{step}.label"]).to(DEV), noise.to(DEV)


@pytest.mark.parametrize("streams", ["overlapped", "single"])
@pytest.mark.parametrize("kind", ["unet", "vnet"])
def test_three_class_trainer_vs_reference_trace(kind, streams):
    """DyconTrainer(num_classes=3) against the reference's ISLES loop body with three classes (two steps, fp32, dropout off), with
    tests/test_nclasses_gpu.py::test_isles_step_body_three_classes' bounds"""
    g = _nc3(kind)
    tr, mk, s0, NC = _nc3_trainer(g, kind, overlap=streams == "overlapped")
    assert NC == 3 and tr.acc20.numel() == (5 + 3 * NC) + 4
    names = list(g["param_names"])
    assert names == tr.names
    off = DropoutSpec("off")
    for step, vol, lab, noise in _nc3_batches(g):
        out = tr.step(vol, lab, noise=noise, s_drop=off, t_drop=off, epoch=int(g[f"s{step}.epoch"]), beta=float(g[f"s{step}.beta"]))
        ref = g[f"s{step}.scalars.f64"]   # loss, ce, dice, cons, fecl, uncl, cons_weight, grad_norm -- the trace's fp64 twin
        got = [float(out[k]) for k in KEYS] + [out["cons_weight"], float(out["grad_sumsq"].sqrt())]
        print(f"step {step} scalars: got {got}\n  fp64 {list(ref)}\n  fp32 {list(g[f's{step}.scalars'])}")
        np.testing.assert_allclose(got[:7], ref[:7], rtol=1e-4, atol=1e-6, err_msg=f"loss scalars step {step}")
        np.testing.assert_allclose(got[7], ref[7], rtol=1e-4, err_msg=f"grad norm step {step}")
        np.testing.assert_array_equal(out["mask"].cpu().numpy().reshape(g[f"s{step}.mask"].shape), g[f"s{step}.mask"])
        assert out["s_logits"].shape[-1] == NC
        lo = out["s_logits"].cpu().permute(0, 4, 1, 2, 3)[..., ::4, ::4, ::4]
        within_budget(lo.numpy(), g[f"s{step}.logits_sub"], g[f"s{step}.logits_sub.f64"], f"student logits step {step}")
        for key, t in (("logits_stats", out["s_logits"]), ("t_logits_stats", out["t_logits"]), ("feat_stats", out["s_feat"])):
            r64 = g[f"s{step}.{key}.f64"]
            np.testing.assert_allclose(_stats(t), r64, rtol=1e-4, atol=1e-4 * r64[1], err_msg=f"{key} step {step}")
        for k, ref_s, ref_t in zip(names, g[f"s{step}.student_stats.f64"], g[f"s{step}.teacher_stats.f64"]):
            np.testing.assert_allclose(_stats(tr.p[k]), ref_s, rtol=1e-4, atol=1e-4, err_msg=f"student {k} step {step}")
            np.testing.assert_allclose(_stats(tr.t[k]), ref_t, rtol=1e-4, atol=1e-4, err_msg=f"teacher {k} step {step}")
    assert tr.iter_num == 2 and tr.skipped_steps == 0
    sd, ref_sd = tr.state_dict(), mk(s0, n_classes=NC)      # state_dict contract: the reference factory's keys and shapes for 3 classes
    assert list(sd) == list(ref_sd)
    assert all(tuple(sd[k].shape) == tuple(ref_sd[k].shape) for k in sd)


# ------------------------------------------------------------------------------------------------------ (d) replay == eager
def _labels3(vol, lab):
    """three label values from a synthetic batch: class 2 where the background volume is bright"""
    return torch.where((lab == 0) & (vol[:, 0] > 1.0), torch.full_like(lab, 2), lab)


@pytest.mark.parametrize("net", ["vnet", "unet_3D"])
def test_replay_equals_eager_three_classes(net):
    """tests/test_trainer_gpu.py::test_replay_equals_eager at C = 3 with EVERY patched scalar moving: an explicit epoch per step
    (beta and the FeCL threshold) and iterations 146..152 with a 2-epoch ramp (the consistency weight steps at iteration 150, a
    replayed step).  A replay patch index missing for a C-class entry point re-issues the recorded step's scalar and fails here."""
    from dycon_paper_replication_amd.synthetic import make_batch
    batches = [make_batch(500 + i, 2, (32, 32, 32)) for i in range(7)]
    runs = {}
    for replay in (False, True):
        tr = DyconTrainer(TrainConfig(model=net, num_classes=3, labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=9, replay=replay,
                                      consistency_rampup=2.0, dice_variant="multiclass"), DEV)
        tr.iter_num = 146
        losses, sched = [], []
        for i, (vol, lab, _) in enumerate(batches):
            vol, lab = vol.to(DEV), lab.to(DEV)
            lab3 = _labels3(vol, lab)
            assert set(torch.unique(lab3).tolist()) == {0, 1, 2}
            out = tr.step(vol, lab3, epoch=200 * i)
            losses.append([float(out[k]) for k in KEYS])
            sched.append((out["beta"], out["cons_weight"]))
        assert (tr._rp is not None) == replay and tr.iter_num == 153
        if replay:
            assert {"dycon_seg_lossesc_fwd", "dycon_seg_lossesc_bwd", "dycon_step_lossesc"} <= set(tr._rp["by_name"])
        assert len({b for b, _ in sched}) == 7 and len({c for _, c in sched[3:]}) == 2      # both move over the replayed steps
        runs[replay] = (np.array(losses), tr.flat_p.clone(), tr.flat_t.clone(), tr.flat_m.clone())
    np.testing.assert_allclose(runs[True][0], runs[False][0], rtol=1e-5, atol=1e-6)
    for a, b in zip(runs[True][1:], runs[False][1:]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


# ------------------------------------------------------------------------------------------------------ (e) bf16 vs fp32 mode
@pytest.mark.parametrize("kind", ["unet", "vnet"])
def test_bf16_step_three_classes_tracks_fp32(kind):
    """step 0 of the fixture's batch in bf16 storage (fast exp / log sequences in the loss pass) against the fp32 mode of the same
    initialisation, which test_three_class_trainer_vs_reference_trace pins to the reference: the project's bf16 bound, 3e-2 relative"""
    g = _nc3(kind)
    rows = {}
    for dt in (torch.float32, torch.bfloat16):
        tr, _, _, _ = _nc3_trainer(g, kind, dtype=dt)
        off = DropoutSpec("off")
        _, vol, lab, noise = next(iter(_nc3_batches(g)))
        out = tr.step(vol, lab, noise=noise, s_drop=off, t_drop=off, epoch=int(g["s0.epoch"]), beta=float(g["s0.beta"]))
        rows[dt] = np.array([float(out[k]) for k in KEYS])
    print(f"{kind} step 0: fp32 {rows[torch.float32]}\n  bf16 {rows[torch.bfloat16]}")
    np.testing.assert_allclose(rows[torch.bfloat16], rows[torch.float32], rtol=3e-2)


# ------------------------------------------------------------------------------------------------------ (f) two classes untouched
def test_two_classes_issue_the_two_class_launches():
    from dycon_paper_replication_amd.synthetic import make_batch
    tr = DyconTrainer(TrainConfig(model="vnet", num_classes=2, labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=9), DEV)
    assert tr.acc20.numel() == 20
    vol, lab, _ = make_batch(500, 2, (32, 32, 32))
    for _ in range(3):
        tr.step(vol.to(DEV), lab.to(DEV))
    names = set(tr._rp["by_name"])
    assert {"dycon_seg_losses_fwd", "dycon_seg_losses_bwd", "dycon_step_losses"} <= names
    assert not names & set(NEW_NAMES)
