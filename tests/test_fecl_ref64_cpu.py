"""CPU: the explicit pair-weight fp64 FeCL reference (tests/fecl_ref64.py) against the oracle through autograd, against the
reference's own fixtures, and the threshold-gap conditions of every clustered GPU case (tests/test_fecl_clustered_gpu.py)."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden
from fecl_ref64 import CASE_THR, CROSS_EMPTY, case, case_inputs, assert_gap, clustered, fecl_pairs64
from oracle import losses as OL

T = torch.from_numpy
THR = 0.5          # threshold_rampup(epoch >= rampup_epochs): the oracle takes an epoch, the reference under test the threshold
RAMP = 1500


def _oracle(f, mask, t, u, focal):
    B, N, _ = f.shape
    fr = f.clone().requires_grad_(True)
    ur = u.clone().requires_grad_(True) if u is not None else None
    loss = OL.fecl(fr, mask.double().view(B, 1, N), t, ur, RAMP, 0.6, 2.0, focal, RAMP, 1.0)
    loss.backward()
    return loss.detach(), fr.grad, (ur.grad if ur is not None else None)


def _mask_sets(B, N):
    kinds = ["mixed", "oneclass", "singleton"] + (["block_aligned"] if N > 128 else [])
    if B == 1:
        return [[k] for k in kinds]
    sets = [["mixed", "oneclass", "singleton"]]
    if N > 128:
        sets.append(["block_aligned", "mixed", "singleton"])
    return sets


def _assert_grad(got, ref, what):
    """rtol 1e-10 on every element.  The floor 1e-18 is the scale of the literal 1e-18 guards: with no other-label column (n_i = 0)
    the value of an element is decided by them (autograd's 1/d - E/d^2 against the analytic 1e-18 / d^2), far below any gradient
    the loss produces otherwise."""
    err = (got - ref).abs()
    bad = err > 1e-10 * ref.abs() + 1e-18
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements off, worst |err| {float(err[bad].max()):.3e}"


@pytest.mark.parametrize("N,Dm,B", list(itertools.product((37, 64, 130), (16, 64), (1, 3))))
def test_pairs64_equals_oracle_autograd(N, Dm, B):
    """loss, d/dfeat, d/du against OL.fecl in float64 through autograd: every focal / teacher / gambling combination, every mask shape"""
    for masks in _mask_sets(B, N):
        # teacher noise 1: f_i.t_i stays below 1 after the bf16 rounding (the oracle multiplies log(1 - S + 1e-18) by the 0 / 1
        # mask and would return NaN); different-label pairs of one cluster still lie on both sides of THR
        fb, tb, mask = clustered(B, N, Dm, seed=N + Dm + B, K=min(12, Dm), teacher_noise=1.0, masks=masks)
        f, t = fb.double(), tb.double()
        u0 = 0.05 + 0.95 * torch.rand(B, N, generator=torch.Generator().manual_seed(N), dtype=torch.float64)
        for focal, use_t, use_g in itertools.product((False, True), repeat=3):
            what = f"N {N} Dm {Dm} B {B} {masks} focal {focal} teacher {use_t} gambling {use_g}"
            u = u0 if use_g else None
            loss, g, gu = _oracle(f, mask, t if use_t else None, u, focal)
            r = fecl_pairs64(f, mask, t if use_t else None, u, THR, 0.6, 2.0, focal, 1.0, block=50)
            assert abs(float(r.loss) - float(loss)) <= 1e-10 * abs(float(loss)), what
            cnt = float(r.cross_cnt)
            stud = float(r.student_sum) / (B * N) + (float(r.cross_num) / (cnt + 1e-18) if use_t and cnt > 0 else 0.0)
            assert abs(stud - float(loss)) <= 1e-10 * abs(float(loss)), what        # the three accumulators give the same loss
            _assert_grad(r.grad, g, what + " grad")
            if use_g:
                _assert_grad(r.grad_u[..., None], gu[..., None], what + " grad_u")
            else:
                assert r.grad_u is None
            assert bool((r.absgrad * (1 + 1e-12) + 1e-300 >= r.grad.abs()).all()), what + ": absgrad < |grad|"
            assert bool(torch.isfinite(r.grad).all()) and bool(torch.isfinite(r.absgrad).all()), what
            if use_t and "mixed" in masks:
                assert cnt > 0, what + ": the cross branch is empty"


def _cross_with_fp32_similarities(feat, teach, mask, thr):
    """the cross branch as the module docstring of fecl_ref64 states it, in float64, on similarities S rounded to float32 first:
    (cross_num, cross_cnt, d (cross_num / (cross_cnt + 1e-18)) / d feat)"""
    f, t = feat.double(), teach.double()
    S = (f @ t.transpose(1, 2)).float().double()
    hard = (mask[:, :, None] != mask[:, None, :]) & (S > thr)
    num = -torch.log(torch.where(hard, 1 - S + 1e-18, torch.ones_like(S))).sum()
    cnt = hard.sum().double()
    X = torch.where(hard, 1 / (cnt + 1e-18) / (1 - S + 1e-18), torch.zeros_like(S))
    return num, cnt, X @ t


@pytest.mark.parametrize("tag", ["small", "mid", "oneclass", "singleton", "ragged"])
def test_pairs64_vs_reference_fixtures(tag):
    """the reference's own loss and gradient (tests/golden/fecl_*.npz), at the tolerances of test_ops_gpu.test_fecl_golden.
    'ragged' holds a different-label pair whose teacher row repeats the student row: f_i.t_j = 1 - 4.8e-8, less than one float32 ulp
    below 1, so the reference's own float32 `1 - S` is 5.96e-8 and its cross term and gradient (2.5e5) follow that value.  For that
    fixture's teacher configurations the cross branch is therefore evaluated HERE on S rounded to float32 and added to
    fecl_pairs64's student part; its cross count must still be fecl_pairs64's.  Every other fixture checks fecl_pairs64 whole."""
    g = load_golden(f"fecl_{tag}")
    feat, teach, gamb = T(g["feat"]), T(g["teacher"]), T(g["gambling"])
    mask = T(g["mask"]).reshape(feat.shape[0], -1)
    rows = feat.shape[0] * feat.shape[1]
    for i in range(int(g["n_cfg"])):
        epoch, focal, use_t, use_g = [int(v) for v in g[f"cfg{i}"]]
        thr = OL.threshold_rampup(epoch, RAMP, 0.3, 0.5)
        r = fecl_pairs64(feat, mask, teach if use_t else None, gamb if use_g else None, thr, 0.6, 2.0, bool(focal), 1.0, block=24)
        loss, grad = float(r.loss), r.grad
        if tag == "ragged" and use_t:
            stud = fecl_pairs64(feat, mask, None, gamb if use_g else None, thr, 0.6, 2.0, bool(focal), 1.0, block=24)
            num, cnt, gx = _cross_with_fp32_similarities(feat, teach, mask, thr)
            assert float(cnt) == float(r.cross_cnt) > 0 and float(stud.student_sum) == float(r.student_sum)
            loss, grad = float(stud.student_sum) / rows + float(num / (cnt + 1e-18)), stud.grad + gx
        np.testing.assert_allclose(loss, g[f"loss{i}"], rtol=1e-4, atol=1e-6, err_msg=f"loss cfg{i}")
        if np.isfinite(g[f"loss64_{i}"]):        # (the reference's float64 twin is NaN * 0 where a same-label f_i.t_j rounds above 1)
            np.testing.assert_allclose(float(r.loss), g[f"loss64_{i}"], rtol=1e-11, atol=0, err_msg=f"loss64 cfg{i}")
        ref = g[f"grad{i}"]
        err = np.abs(grad.numpy() - ref).max()
        assert err <= 1e-4 * (np.abs(ref).max() + 1e-12) + 1e-8, f"grad cfg{i}: {err}"


def test_pairs64_independent_of_block():
    fb, tb, mask = clustered(2, 130, 64, seed=5, masks=["mixed", "block_aligned"])
    u = 0.05 + 0.95 * torch.rand(2, 130, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for focal, gamb in ((True, None), (False, u)):
        ref = fecl_pairs64(fb, mask, tb, gamb, THR, 0.6, 2.0, focal, 1.0, block=512)
        for block in (1, 7, 64, 130):
            r = fecl_pairs64(fb, mask, tb, gamb, THR, 0.6, 2.0, focal, 1.0, block=block)
            assert float(r.cross_cnt) == float(ref.cross_cnt)
            for a, b in ((r.loss, ref.loss), (r.student_sum, ref.student_sum), (r.cross_num, ref.cross_num)):
                assert abs(float(a) - float(b)) <= 1e-13 * abs(float(b))
            assert bool(((r.grad - ref.grad).abs() <= 1e-13 * ref.absgrad).all())
            assert bool(((r.absgrad - ref.absgrad).abs() <= 1e-13 * ref.absgrad).all())
            if gamb is not None:
                assert bool(((r.grad_u - ref.grad_u).abs() <= 1e-13 * ref.grad_u.abs()).all())


def test_absgrad_is_the_scale_of_a_dropped_tile():
    """what the element-wise GPU bound rests on: a 64-column tile left out of the contraction moves nearly every element of the
    gradient by more than the bound 2^-8 absgrad + 2^-8 |grad| + 1e-6 absgrad allows (here at a CPU size, N = 130).  The
    contraction is rebuilt from autograd on the logits, so it also checks the pair weights W_ij + W_ji and X_ij themselves."""
    fb, tb, mask = clustered(1, 130, 64, seed=9)
    full = fecl_pairs64(fb, mask, tb, None, THR, 0.6, 2.0, True, 1.0)
    whole = _contraction_over(fb, tb, mask, torch.ones(130, dtype=torch.bool))
    assert bool(((whole - full.grad[0]).abs() <= 1e-12 * full.absgrad[0]).all())
    keep = torch.ones(130, dtype=torch.bool)
    keep[64:128] = False
    moved = (full.grad[0] - _contraction_over(fb, tb, mask, keep)).abs()
    bound = 2.0 ** -8 * full.absgrad[0] + 2.0 ** -8 * full.grad[0].abs() + 1e-6 * full.absgrad[0]
    assert float((moved > bound).double().mean()) > 0.9, "a dropped tile would pass the element-wise bound"


def _contraction_over(fb, tb, mask, keep):
    """d loss / d feat of sample 0 (focal, teacher) with the contraction index j restricted to keep: the logits L and S are the
    autograd leaves, so the pair weights are the full ones and only the final sums over j lose columns"""
    f, t = fb.double()[0], tb.double()[0]
    N = f.shape[0]
    m = mask[0].double()
    Lfull = (f @ f.t()) / 0.6
    Lleaf = Lfull.clone().requires_grad_(True)
    Sleaf = (f @ t.t()).clone().requires_grad_(True)
    eye = torch.eye(N, dtype=torch.float64)
    same = (m[:, None] == m[None, :]).double()
    L = Lleaf * (1 - eye)
    L = L - L.max(dim=0, keepdim=True)[0].detach()
    E = torch.exp(L)
    neg = (E * (1 - same)).sum(-1, keepdim=True)
    P = E / (E + neg + 1e-18)
    ell = -torch.log(P + 1e-18) * same * (1 - eye) * (1 - P) ** 2.0
    loss = (ell.sum(-1) / (same.sum(-1) - 1 + 1e-18)).mean()
    hard = ((1 - same).bool() & (Sleaf > THR)).double()
    loss = loss + (-torch.log(1 - Sleaf + 1e-18) * hard).sum() / (hard.sum() + 1e-18)
    gL, gS = torch.autograd.grad(loss, (Lleaf, Sleaf))
    W = (gL + gL.t()) * keep[None, :].double()
    return W @ f / 0.6 + (gS * keep[None, :].double()) @ t


@pytest.mark.parametrize("cid,thr", CASE_THR, ids=[f"{c}-{t}" for c, t in CASE_THR])
def test_gap_conditions_of_the_gpu_cases(cid, thr):
    """for every (shape, seed, thr) of the GPU test, in float64 on the rounded values: no different-label pair within 0.02 of thr,
    none above 0.95, at least 5 % of a mixed sample's different-label pairs above thr"""
    f, t, mask, _ = _inputs(cid)
    assert_gap(f, t, mask, thr, case(cid).masks, cid, expect_hard=cid not in CROSS_EMPTY)


_CACHE = {}


def _inputs(cid):
    if cid not in _CACHE:
        _CACHE.clear()                       # one case alive at a time
        _CACHE[cid] = case_inputs(cid)
    return _CACHE[cid]
