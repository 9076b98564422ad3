"""The FeCL kernels of the bf16 step (fecl_rows128_kernel<PASS, NQ>, fecl_rows128_grad_kernel<NQ>, and fecl_kernel<bf16> below their
dispatch floor) on CLUSTERED features, element by element against the explicit pair-weight float64 reference (tests/fecl_ref64.py).

Isotropic random unit rows (what the other FeCL tests feed) put every student logit within +-0.1 of 0 and a few dozen pairs out of
1e7 above the hard-negative threshold.  fecl_ref64.clustered gives what a trained projection head gives: same-cluster cosines near
0.83, clusters that hold both labels, about 7 % of the different-label pairs above the threshold, and no different-label pair within
0.02 of it -- so the kernel (fp32 accumulation) and the reference take the same branch for every pair, the count out[2] is
comparable exactly and nothing is excluded from any comparison.  The gap conditions are asserted on the CPU for every case
(tests/test_fecl_ref64_cpu.py) and again here before comparing.

Gradient bound, every element:   |got - ref| <= 2^-8 A + 2^-8 |ref| + 1e-6 A,   A = fecl_pairs64(...).absgrad
(the gradient's contraction over the absolute values of its terms).  Derivation: the kernels round each pair weight W_ij + W_ji
(and X_ij) to bf16 once before the gradient MFMA, <= 2^-9 relative per term, hence <= 2^-9 A; the output is stored as bf16,
<= 2^-9 |ref|; the features are bf16 already and their products exact in fp32; 1e-6 A covers the fp32 accumulation and the 1-ulp
hardware exp / log / rcp.  Both rounding terms carry a factor 2.  A 64-column tile dropped or counted twice at N = 1728 moves an
element by about A / 27, ten times the bound.  One-class samples have gradient and A exactly 0 under the focal weight (P = 1), and the
kernels return exactly 0 there.

The cases are fecl_ref64.CASES: one row per column-split count, ragged edge, mask shape and entry point the bf16 step can reach, plus
cross_empty_mixed -- a teacher, both labels and a threshold above every cosine, i.e. out[2] == 0 next to a student term that is not 0.

Every case runs with torch.empty NaN-poisoned and names the kernels it must have launched (both helpers are
test_dispatch_parity_gpu's).  Each case prints its worst |err| / bound; DESIGN.md keeps the MI355X figures.
"""
import pytest
import torch

from fecl_ref64 import CASE_THR, CROSS_EMPTY, assert_gap, case, case_inputs, fecl_pairs64
from test_dispatch_parity_gpu import launched, poisoned  # noqa: F401  (poisoned is a fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import ops

DEV = "cuda:0"
TAU, GAMMA, LAMBDA = 0.6, 2.0, 1.0
COEF = {"ddp_parts": 0.37}           # every other case: coef = 1


def _rows128_names(nq):
    return [f"fecl_rows128_kernel<{p}, {nq}, false>" for p in (1, 2, 3)] + [f"fecl_rows128_grad_kernel<{nq}>"]


def _expected(cid, Dm):
    """the kernels a case exists to cover, and the family it must NOT run on"""
    tail = ["fecl_combine_kernel<__hip_bfloat16>", "fecl_finalize_kernel"]
    if cid == "below_floor":
        return [f"fecl_kernel<__hip_bfloat16, {p}, false>" for p in (1, 2, 3, 4)] + tail, "fecl_rows128"
    names = _rows128_names(Dm // 16) + tail
    if cid == "gambling":
        names += [f"fecl_rows128_kernel<3, {Dm // 16}, true>", "fecl_gambling_finalize_kernel"]
    return names, "fecl_kernel<"


@pytest.fixture(scope="module")
def inputs():
    """a case's tensors on the GPU: one case alive at a time (the thresholds of a case share them, unchanged), none after this module"""
    cache = {}

    def get(cid):
        if cid not in cache:
            cache.clear()
            f, t, mask, u = case_inputs(cid)
            cache[cid] = (f.to(DEV), t.to(DEV), mask.to(DEV), u.to(DEV) if u is not None else None)
        return cache[cid]

    yield get
    cache.clear()


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.mark.parametrize("cid,thr", CASE_THR, ids=[f"{c}-{t}" for c, t in CASE_THR])
def test_fecl_clustered(poisoned, inputs, cid, thr):  # noqa: F811
    c = case(cid)
    B, N, Dm, focal, use_t, use_g, masks = c.B, c.N, c.Dm, c.focal, c.teacher, c.gambling, c.masks
    f, t, mask, u = inputs(cid)
    assert f.dtype == torch.bfloat16 and t.dtype == torch.bfloat16
    assert_gap(f, t, mask, thr, masks, cid, expect_hard=cid not in CROSS_EMPTY)
    ref = fecl_pairs64(f, mask, t if use_t else None, u, thr, TAU, GAMMA, focal, LAMBDA)
    cval = COEF.get(cid, 1.0)
    coef = torch.full((1,), cval, device=DEV)
    args = (f, t if use_t else None, mask, u, TAU, GAMMA, focal, thr, LAMBDA)
    names = set()
    with launched(names):
        loss, st = ops.fecl_fwd(*args)
        out = st.out.clone()
        g = ops.fecl_bwd(*args, st, coef)
        if use_g:         # d/du, and d/dfeat once more, through the entry points the step uses for a differentiable u
            st2 = ops.fecl_fwd_rows(f, t if use_t else None, mask, TAU, thr)
            _, gu = ops.fecl_gambling_finalize(f, st2, u, coef=coef)
            loss2 = ops.fecl_finalize(st2, B * N, LAMBDA, use_t).clone()
            g2 = ops.fecl_bwd(f, t if use_t else None, mask, None, TAU, GAMMA, False, thr, LAMBDA, st2, coef)
    expect, forbidden = _expected(cid, Dm)
    print(f"{cid} thr {thr}: launched {sorted(names)}")
    missing = [k for k in expect if k not in names]
    assert not missing, f"{cid}: expected kernels not launched: {missing}; launched {sorted(names)}"
    assert not [k for k in names if k.startswith(forbidden)], f"{cid}: ran on the other kernel family: {sorted(names)}"

    # ---- finiteness
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(out[:3]).all()) and bool(torch.isfinite(g).all()), cid

    # ---- cross branch
    cnt = float(ref.cross_cnt)
    if use_t:
        assert float(out[2]) == cnt, f"{cid}: cross count {float(out[2])} vs {cnt}"
        if cid in CROSS_EMPTY:
            assert cnt == 0 and float(out[1]) == 0.0
        else:
            assert cnt > 0
            r1 = abs(float(out[1]) - float(ref.cross_num)) / abs(float(ref.cross_num))
            print(f"{cid} thr {thr}: cross count {int(cnt)}, out[1] rel err {r1:.3e} (bound 1e-4)")
            assert r1 <= 1e-4, f"{cid}: cross numerator off by {r1:.3e}"
    else:
        assert float(out[1]) == 0.0 and float(out[2]) == 0.0

    # ---- loss (a one-class batch has P = 1 and loss exactly 0 in the reference: the kernels must return exactly 0 as well;
    #      cross_empty_mixed is the empty cross branch next to a student term that is not 0)
    el, e0 = abs(float(loss[0]) - float(ref.loss)), abs(float(out[0]) - float(ref.student_sum))
    print(f"{cid} thr {thr}: loss {float(loss[0]):.6f} vs {float(ref.loss):.6f}, |err| / (3e-4 |ref|) "
          f"{el / (3e-4 * abs(float(ref.loss))) if float(ref.loss) else el:.3e}; out[0] rel err {e0 / abs(float(ref.student_sum)) if float(ref.student_sum) else e0:.3e}")
    assert el <= 3e-4 * abs(float(ref.loss)), f"{cid}: loss {float(loss[0])} vs {float(ref.loss)}"
    if cid in CROSS_EMPTY:          # the student term alone
        assert abs(float(loss[0]) - float(out[0]) / (B * N)) <= 1e-6 * abs(float(loss[0]))
        assert (float(ref.loss) > 1.0) == (cid == "cross_empty_mixed")

    # ---- gradient, every element
    def check_grad(got, what):
        assert got.shape == ref.grad.shape and got.dtype == torch.bfloat16
        want = cval * ref.grad
        bound = cval * (2.0 ** -8 * ref.absgrad + 2.0 ** -8 * ref.grad.abs() + 1e-6 * ref.absgrad)
        err = (got.double() - want).abs()
        ratio = torch.where(err > 0, err / bound, torch.zeros_like(err))         # err = 0 at bound = 0 (one-class rows) is inside
        worst = float(ratio.max())
        at = [int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape)]
        small = ref.grad.abs().amax(-1) < 1e-2 * ref.grad.abs().max()
        print(f"{cid} thr {thr}: {what} worst |err| / bound {worst:.3f} at (b, row, d) = {at}; rows below 1 % of the largest "
              f"gradient: {int(small.sum())}, their worst {float(ratio[small].max()) if bool(small.any()) else 0.0:.3f}")
        assert worst <= 1.0, f"{cid}: {what} exceeds the element-wise bound {worst:.3f} x at {at}"

    check_grad(g, "d/dfeat")
    if use_g:
        assert bool(torch.isfinite(gu).all()) and bool(torch.isfinite(g2).all()) and bool(torch.isfinite(loss2).all())
        check_grad(g2, "d/dfeat (differentiable-u entry points)")
        assert abs(float(loss2[0]) - float(ref.loss)) <= 3e-4 * abs(float(ref.loss))
        ru = _rel(gu, cval * ref.grad_u)
        print(f"{cid} thr {thr}: d/du rel err {ru:.3e} (bound 2e-2)")
        assert ru <= 2e-2, f"{cid}: d/du off by {ru:.3e}"
