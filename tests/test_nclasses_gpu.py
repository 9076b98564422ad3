"""GPU: class counts other than 2 -- the fused C-class V-Net head against the launches it replaces, the skinny 16 -> C weight
gradient, UnCLoss for C classes against the reference's own outputs (tests/golden/uncl_nc.npz), the full nets at C = 3 / 1 / 8
(full_nets_nc.npz), the reference's ISLES loop body (train_DyCON_ISLES22.py:236-324) restated on this package's imports with
class_num = 3 (step_isles_nc3.npz), and the sliding-window evaluator with a 3-class model."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import _lib, ops
    from dycon_paper_replication_amd._lib import CONV_1X1
    from dycon_paper_replication_amd.engine import Engine, param_spec, projection_buffers
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.utils import dycon_losses, losses, ramps
    from dycon_paper_replication_amd.utils import test_3d_patch as T3
from oracle import nets as ON
from test_engine_gpu import within_budget

DEV = "cuda:0"
T = torch.from_numpy
HC = 16


def close(a, b, rtol=1e-4, atol=1e-6, msg=""):
    a = a.detach().float().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().float().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def _stats(t):
    t = t.detach().double().cpu()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


# ------------------------------------------------------------------------------------------------------------------- (a) head kernels
def _head_case(K, dtype, kind, with_drop, sp, B=3):
    rng = np.random.default_rng(zlib.crc32(repr((K, str(dtype), kind, with_drop, sp)).encode()))
    V = sp[0] * sp[1] * sp[2]
    f = lambda a: T(np.asarray(a, dtype=np.float32))  # noqa: E731
    x = f(rng.standard_normal((B,) + sp + (HC,)) * 1.5 + 0.3).to(DEV, dtype)
    gl = f(rng.standard_normal((B,) + sp + (K,))).to(DEV)
    W = f(rng.standard_normal((K, HC, 1, 1, 1)) * 0.4).to(DEV)
    hb = f(rng.standard_normal(K)).to(DEV)
    affine = kind != "in"
    gamma = f(rng.standard_normal(HC) * 0.5 + 1.0).to(DEV) if affine else None
    beta = f(rng.standard_normal(HC) * 0.3).to(DEV) if affine else None
    Nb, G, Vn = (1, HC, B * V) if kind == "bn" else (B, 16, V)
    cs = f((rng.random(Nb * HC) > 0.5) * 2.0).to(DEV) if with_drop else None
    return x, gl, W, hb, gamma, beta, Nb, G, Vn, cs


def _check_head(K, dtype, kind, with_drop, sp):
    x, gl, W, hb, gamma, beta, Nb, G, Vn, cs = _head_case(K, dtype, kind, with_drop, sp)
    affine = gamma is not None
    new = lambda: (torch.empty(HC, device=DEV), torch.empty(HC, device=DEV)) if affine else (None, None)  # noqa: E731
    # ---- the launches the fused kernels replace (where dycon_norm_fwd serves the size with its one-launch kernel, whose statistics
    # come from a different summation, the statistics launch + dycon_norm_apply: what Engine._vnet falls back to)
    if ops.norm_fwd_is_fused(x, Vn, HC, G):
        stats = ops.norm_stats(x, Nb, Vn, HC, G)
        y = ops.norm_apply(x, stats, Nb, Vn, HC, G, gamma, beta, True, None, None, cs)
    else:
        y, stats = ops.norm_fwd(x, Nb, Vn, HC, G, gamma, beta, True, None, cs)
    logits_ref = ops.conv_direct(y, W.reshape(K, HC).t().contiguous(), hb, CONV_1X1, K, torch.float32)
    gy = ops.conv_direct(gl, W.reshape(K, HC).contiguous(), None, CONV_1X1, HC, dtype)
    dg_ref, db_ref = new()
    gx_ref = ops.norm_bwd(x, False, gy, stats, Nb, Vn, HC, G, gamma, beta, True, dg_ref, db_ref, chan_scale=cs)
    gw_ref, gb_ref = torch.empty_like(W), torch.empty_like(hb)
    ops.conv_wgrad(y, gl, gw_ref, CONV_1X1, 0, 1, HC, dbias=gb_ref)
    # ---- fused
    stats2 = ops.norm_stats(x, Nb, Vn, HC, G)
    assert torch.equal(stats2, stats)
    logits = ops.norm_head_fwd(x, stats2, Nb, Vn, G, W, hb, gamma, beta, True, cs)
    dg, db = new()
    gx, pend = ops.norm_head_bwd(x, gl, stats2, Nb, Vn, G, W, gamma, beta, True, dg, db, cs)
    gw, gb = torch.full_like(W, float("nan")), torch.full_like(hb, float("nan"))
    ops.norm_head_dparams(pend, gw, gb)
    torch.cuda.synchronize()
    assert logits.shape == x.shape[:-1] + (K,) and logits.dtype == torch.float32
    assert torch.equal(logits, logits_ref)
    scale = float(gx_ref.float().abs().max())
    err = float((gx.float() - gx_ref.float()).abs().max())
    print(f"head K={K} {dtype} {kind} drop={with_drop} {sp}: |gx - ref| {err:.3e} of scale {scale:.3e}")
    assert err <= (1e-5 if dtype == torch.float32 else 2.0 ** -7) * scale, (err, scale)
    if dtype == torch.bfloat16:
        assert float((gx != gx_ref).float().mean()) < 1e-3
    if affine:
        close(dg, dg_ref, 1e-5, 1e-5 * float(dg_ref.abs().max()), "dgamma")
        close(db, db_ref, 1e-5, 1e-5 * float(db_ref.abs().max()), "dbeta")
    close(gw, gw_ref, 1e-4, 1e-4 * float(gw_ref.abs().max()), "head weight gradient")
    close(gb, gb_ref, 1e-4, 1e-4 * float(gb_ref.abs().max()), "head bias gradient")


@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["gn", "in", "bn"])
@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
def test_class_head_fused_equals_norm_then_head(K, dtype, kind, with_drop):
    """dycon_norm_headc_fwd / _bwd / _dparams against dycon_norm_fwd + dycon_conv_direct forward and dycon_conv_direct's data
    gradient + dycon_norm_bwd + dycon_conv_wgrad backward: logits bit for bit, gx / dgamma / dbeta to fp32 round-off (one bf16 step
    on < 1e-3 of the elements in bf16), the head's weight / bias gradient up to summation order.  B = 3 at 20 x 18 x 16: 5 760 voxels
    per sample, no multiple of the 256-thread stride, several statistics chunks."""
    _check_head(K, dtype, kind, with_drop, (20, 18, 16))


@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_class_head_fewer_voxels_than_one_stride(K, dtype):
    """5 x 7 x 9 = 315 voxels per sample: fewer than one workgroup's 256-thread stride covers twice"""
    _check_head(K, dtype, "gn", True, (5, 7, 9))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["gn", "bn"])
def test_two_classes_through_the_class_entry_points_equal_the_two_class_ones(dtype, kind):
    """classes = 2 through dycon_norm_headc_* equals dycon_norm_head_* bit for bit in every output"""
    x, gl, W, hb, gamma, beta, Nb, G, Vn, cs = _head_case(2, dtype, kind, True, (20, 18, 16))
    p, s, d = ops._p, ops._s, ops.dt(x)
    stats = ops.norm_stats(x, Nb, Vn, HC, G)
    lo_ref = ops.norm_head_fwd(x, stats, Nb, Vn, G, W, hb, gamma, beta, True, cs)
    dg_ref, db_ref = torch.empty(HC, device=DEV), torch.empty(HC, device=DEV)
    gx_ref, pend = ops.norm_head_bwd(x, gl, stats, Nb, Vn, G, W, gamma, beta, True, dg_ref, db_ref, cs)
    gw_ref, gb_ref = torch.empty_like(W), torch.empty_like(hb)
    ops.norm_head_dparams(pend, gw_ref, gb_ref)
    lo = torch.full_like(lo_ref, float("nan"))
    _lib.call("dycon_norm_headc_fwd", p(x), d, Nb, Vn, G, 2, p(stats), p(gamma), p(beta), 1, p(cs), p(W), p(hb), p(lo), s())
    nbytes = _lib.load().dycon_norm_headc_workspace(Nb, Vn, 2)
    assert nbytes == _lib.load().dycon_norm_head_workspace(Nb, Vn)
    ws = torch.empty(nbytes // 4 + 1, device=DEV)
    gx = torch.empty_like(x)
    dg, db = torch.empty(HC, device=DEV), torch.empty(HC, device=DEV)
    _lib.call("dycon_norm_headc_bwd", p(x), p(gl), p(gx), d, Nb, Vn, G, 2, p(stats), p(gamma), p(beta), 1, p(cs), p(W), p(dg), p(db),
              p(ws), ws.numel() * 4, s())
    gw, gb = torch.empty_like(W), torch.empty_like(hb)
    _lib.call("dycon_norm_headc_dparams", p(ws), Nb, Vn, 2, p(gw), p(gb), s())
    torch.cuda.synchronize()
    for name, a, b in (("logits", lo, lo_ref), ("gx", gx, gx_ref), ("dgamma", dg, dg_ref), ("dbeta", db, db_ref), ("dW", gw, gw_ref),
                       ("db", gb, gb_ref)):
        assert torch.equal(a, b), name


def test_class_head_refuses_nine_classes():
    x, gl, W, hb, gamma, beta, Nb, G, Vn, cs = _head_case(8, torch.float32, "gn", False, (5, 7, 9))
    stats = ops.norm_stats(x, Nb, Vn, HC, G)
    lo = torch.empty(x.shape[:-1] + (9,), device=DEV)
    with pytest.raises(_lib.DyconLibraryError, match="classes = 9"):
        _lib.call("dycon_norm_headc_fwd", ops._p(x), ops.dt(x), Nb, Vn, G, 9, ops._p(stats), None, None, 1, None, ops._p(W), None,
                  ops._p(lo), ops._s())


# ------------------------------------------------------------------------------------------------------------------- (b) skinny wgrad
@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("sp", [(20, 18, 16), (5, 7, 9)], ids=["m5760", "m315"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_skinny_wgrad_16_to_classes(K, sp, dtype):
    """wgrad_1x1_skinny (16 channels -> K fp32 logit gradients) against the sums in double: 1e-4 of the result's scale"""
    name = _lib.load().dycon_conv_wgrad_name(ops.dt(torch.empty(0, dtype=dtype)), _lib.F32, CONV_1X1, 1, *sp, HC, K).decode()
    assert name == "wgrad_1x1_skinny"
    rng = np.random.default_rng(zlib.crc32(repr((K, sp, str(dtype))).encode()))
    x = T(rng.standard_normal((1,) + sp + (HC,)).astype(np.float32)).to(DEV, dtype)
    gy = T(rng.standard_normal((1,) + sp + (K,)).astype(np.float32)).to(DEV)
    gw, gb = torch.full((K, HC, 1, 1, 1), float("nan"), device=DEV), torch.full((K,), float("nan"), device=DEV)
    ops.conv_wgrad(x, gy, gw, CONV_1X1, 0, 1, HC, dbias=gb)
    ref = gy.reshape(-1, K).double().t() @ x.reshape(-1, HC).double()
    refb = gy.reshape(-1, K).double().sum(0)
    close(gw.reshape(K, HC), ref, 1e-4, 1e-4 * float(ref.abs().max()), "dW")
    close(gb, refb, 1e-4, 1e-4 * float(refb.abs().max()), "db")


# ------------------------------------------------------------------------------------------------------------------- (c) UnCLoss
def _layouts(t):
    yield "ncdhw", t.contiguous()
    cl = t.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)       # the nets' channels-last view
    assert cl.shape == t.shape and (cl.shape[1] == 1 or not cl.is_contiguous())
    yield "channels_last", cl


def _either(got, ref32, ref64, rtol, atol, what):
    """within the bound of the reference's fp32 output or, where fp32 disagrees, of its fp64 twin (the arbiter)"""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    ok32 = np.abs(got - ref32) <= atol + rtol * np.abs(ref32)
    ok64 = np.abs(got - ref64) <= atol + rtol * np.abs(ref64)
    bad = ~(ok32 | ok64)
    print(f"{what}: max |got-ref32| {np.abs(got - ref32).max():.3e}, max |got-ref64| {np.abs(got - ref64).max():.3e}, "
          f"outside the fp32 bound {int((~ok32).sum())}, outside both {int(bad.sum())}")
    assert not bad.any(), f"{what}: {int(bad.sum())} values outside rtol {rtol} / atol {atol} of both the fp32 and the fp64 reference"


@pytest.mark.parametrize("C", [1, 3, 4, 8])
@pytest.mark.parametrize("big", [False, True], ids=["unit", "pm30"])
def test_uncl_classes_golden(C, big):
    g = load_golden("uncl_nc")
    tag = f"c{C}_big" if big else f"c{C}"
    crit = dycon_losses.UnCLoss()
    for (lname, s), (_, t) in zip(_layouts(T(g[f"{tag}.s"]).to(DEV)), _layouts(T(g[f"{tag}.t"]).to(DEV))):
        for i, beta in enumerate(g["betas"]):
            x = s.detach().requires_grad_(True)
            loss = crit(x, t, float(beta))
            (gx,) = torch.autograd.grad(loss, x)
            assert loss.dim() == 0 and gx.shape == x.shape
            what = f"UnCL C={C} {tag} {lname} beta={beta}"
            _either(loss, g[f"{tag}.loss{i}"], g[f"{tag}.loss{i}.f64"], 1e-5, 1e-6, what + " loss")
            _either(gx, g[f"{tag}.grad{i}"], g[f"{tag}.grad{i}.f64"], 1e-4, 1e-8, what + " grad")


def test_uncl_two_classes_keeps_the_fused_route():
    """UnCLoss with C = 2 through the public class: the bits of ops.seg_losses_* called directly"""
    g = load_golden("uncl_a")
    s, t = T(g["s"]).to(DEV), T(g["t"]).to(DEV)
    sn, tn = s.permute(0, 2, 3, 4, 1).contiguous(), t.permute(0, 2, 3, 4, 1).contiguous()
    B, V = s.shape[0], s[0, 0].numel()
    dummy = torch.empty(1, dtype=torch.uint8, device=DEV)
    for beta in (0.5, 5.0):
        sums = ops.seg_losses_fwd(sn, tn, dummy, 0, beta)
        ref = ops.seg_losses_finalize(sums, B, 0, V, beta)[5]
        coef = torch.zeros(5, device=DEV)
        coef[4] = 1.0
        gref = ops.seg_losses_bwd(sn, tn, dummy, 0, beta, sums, coef).permute(0, 4, 1, 2, 3)
        x = s.clone().requires_grad_(True)
        loss = dycon_losses.UnCLoss()(x, t, beta)
        (gx,) = torch.autograd.grad(loss, x)
        assert torch.equal(loss, ref) and torch.equal(gx, gref)


@pytest.mark.parametrize("C", [1, 3, 8])
def test_uncl_nan_in_nan_out(C):
    s = torch.randn(2, C, 4, 4, 4, device=DEV)
    t = torch.randn(2, C, 4, 4, 4, device=DEV)
    for bad_s, bad_t in ((True, False), (False, True)):
        a, b = s.clone(), t.clone()
        (a if bad_s else b)[1, C - 1, 2, 3, 1] = float("nan")
        x = a.requires_grad_(True)
        loss = dycon_losses.UnCLoss()(x, b, 2.0)
        assert torch.isnan(loss), float(loss)
        (gx,) = torch.autograd.grad(loss, x)
        assert torch.isnan(gx[1, :, 2, 3, 1]).all()          # the voxel's own gradient is not a silent zero
        assert torch.isfinite(gx[0]).all()


# ------------------------------------------------------------------------------------------------------------------- (d) full nets
FULL = [("vnet3", "vnet", 3), ("unet3", "unet", 3), ("vnet1", "vnet", 1), ("vnet8", "vnet", 8)]


def _build(kind, seed, C, dtype=torch.float32):
    net_type = "vnet" if kind == "vnet" else "unet_3D"
    p_all = (ON.make_vnet_params if kind == "vnet" else ON.make_unet_params)(seed, n_classes=C)
    spec = param_spec(net_type, 1, C)
    assert list(spec) == list(ON.trainable(p_all))
    params = {k: p_all[k].to(DEV).contiguous() for k in spec}
    grads = {k: torch.full_like(v, float("nan")) for k, v in params.items()}
    bufs = {k: p_all[k].to(DEV) for k in projection_buffers()}
    return Engine(net_type, params, grads, bufs, dtype=dtype)


def _full_inputs(g, tag):
    """x and the cotangents of `tag`, drawn in the fixture's order"""
    rng = np.random.default_rng(int(g["x_seed"]))
    draw = lambda *s: T(rng.standard_normal(s).astype(np.float32))  # noqa: E731
    x = draw(2, 1, 32, 32, 32)
    for name in g["nets"]:
        C = int(name[4:])
        r1, r2 = draw(2, C, 32, 32, 32), draw(2, 256, 4, 4, 4)
        if name == tag:
            return x, r1, r2
    raise KeyError(tag)


def _check_grad_stats(kind, eng_p, got_stats, refs64, refs32, what, skip_final_check=None):
    """tests/test_engine_gpu.py::test_full_net_fp32_vs_reference's rule: the worst relative error of the (sum, sum|.|, sum .^2)
    statistics over all parameters within 1e-4 or twice the worst relative error of the reference's own fp32 run"""
    rel = lambda st, ref: np.array([abs(st[0] - ref[0]) / (ref[1] + 1e-30), abs(st[1] - ref[1]) / (ref[1] + 1e-30),  # noqa: E731
                                    abs(st[2] - ref[2]) / (ref[2] + 1e-30)])
    worst_hip, worst_ref, at = np.zeros(3), np.zeros(3), [None] * 3
    for k, ref in refs64.items():
        if k.startswith("final."):
            assert not ref.any()
            if skip_final_check is not None:
                skip_final_check(k)
            continue
        got = got_stats[k]
        assert np.isfinite(got).all(), f"{k}: gradient statistics {got} are not finite"
        w = k[:-4] + "weight"
        one_channel_groups = kind == "unet" or eng_p[k].shape[0] == 16 or k.startswith("projection.")
        if k.endswith(".bias") and eng_p[w].dim() == 5 and not k.startswith("out_conv") and one_channel_groups:
            assert got[1] <= 1e-4 * refs64[w][1] + 2e-2, (k, got, ref)       # analytically zero: round-off noise only
            continue
        rh, rr = rel(got, ref), rel(refs32[k], ref)
        for j in range(3):
            if rh[j] > worst_hip[j]:
                worst_hip[j], at[j] = rh[j], k
        worst_ref = np.maximum(worst_ref, rr)
    print(f"{what}: worst relative gradient-statistic error: hip {worst_hip} at {at}; reference fp32 {worst_ref}")
    assert (worst_hip <= np.maximum(1e-4, 2 * worst_ref)).all(), (worst_hip, worst_ref, at)


@pytest.mark.parametrize("tag,kind,C", FULL, ids=[f[0] for f in FULL])
def test_full_net_classes_fp32_vs_reference(tag, kind, C):
    g = load_golden("full_nets_nc")
    x, r1, r2 = _full_inputs(g, tag)
    eng = _build(kind, int(g[f"{tag}.param_seed"]), C)
    xd = x.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    prof = ops.KernelProfiler()
    try:
        logits, feats, sdf = eng.forward(xd, training=True, record=True, want_sdf=True)
        torch.cuda.synchronize()
        launched = set(prof.summary())
    finally:
        prof.close()
    assert logits.shape == (2, 32, 32, 32, C) and logits.dtype == torch.float32
    if kind == "vnet":      # block_nine's normalisation and the C-class head ran as one kernel, not norm_apply + conv_direct
        fused = [n for n in launched if n.startswith("norm_apply_head")]
        assert fused and all(f"{C}>" in n for n in fused), sorted(launched)
        assert not [n for n in launched if n.startswith("head_1x1_fwd")], sorted(launched)
    else:
        assert sdf.shape == (2, 32, 32, 32, C)
        np.testing.assert_allclose(_stats(sdf), g[f"{tag}.sdf_stats.f64"], rtol=1e-4)
    lo = logits.cpu().permute(0, 4, 1, 2, 3)
    fe = feats.cpu().permute(0, 4, 1, 2, 3)
    sub = (lambda t: t[..., ::4, ::4, ::4]) if C == 8 else (lambda t: t[..., ::2, ::2, ::2])
    within_budget(sub(lo).numpy(), g[f"{tag}.logits_sub"], g[f"{tag}.logits_sub.f64"], "logits")
    within_budget(fe[..., ::2, ::2, ::2].numpy(), g[f"{tag}.feats_sub"], g[f"{tag}.feats_sub.f64"], "feats")
    np.testing.assert_allclose(_stats(lo), g[f"{tag}.logits_stats.f64"], rtol=1e-4)
    np.testing.assert_allclose(_stats(fe), g[f"{tag}.feats_stats.f64"], rtol=1e-4, atol=1e-4 * g[f"{tag}.feats_stats.f64"][1])
    eng.backward(r1.permute(0, 2, 3, 4, 1).contiguous().to(DEV), r2.permute(0, 2, 3, 4, 1).contiguous().to(DEV))
    torch.cuda.synchronize()
    names = list(g[f"{tag}.param_names"])
    refs = dict(zip(names, g[f"{tag}.grad_stats.f64"]))
    refs32 = dict(zip(names, g[f"{tag}.grad_stats"]))

    def final_untouched(k):
        assert torch.isnan(eng.g[k]).all()           # no gradient reaches the discarded sdf head
    _check_grad_stats(kind, eng.p, {k: _stats(eng.g[k]) for k in names}, refs, refs32, f"full net {tag}", final_untouched)


@pytest.mark.parametrize("tag,kind,C", FULL, ids=[f[0] for f in FULL])
def test_full_net_classes_bf16_close_to_fp32(tag, kind, C):
    """what tests/test_engine_gpu.py::test_full_net_bf16_close_to_fp32 holds bf16 to"""
    eng32, eng16 = _build(kind, 11, C), _build(kind, 11, C, torch.bfloat16)
    x = torch.randn(1, 32, 32, 32, 1, device=DEV)
    l32, f32_, _ = eng32.forward(x, record=False)
    l16, f16, _ = eng16.forward(x, record=False)
    assert l16.dtype == torch.float32 and f16.dtype == torch.bfloat16 and l16.shape[-1] == C
    rel = (l16 - l32).abs().max() / l32.abs().max()
    assert rel < 0.08, rel
    relf = (f16.float() - f32_).abs().max() / f32_.abs().max()
    assert relf < 0.15, relf


# ------------------------------------------------------------------------------------------------------------------- (e) ISLES body
def _isles_step_body(model, ema_model, optimizer, ce_loss, dice_loss, uncl_criterion, fecl_criterion, volume_batch, label_batch, noise,
                     labeled_bs, iter_num, epoch_num, beta, base_lr, max_iterations, consistency=0.1, consistency_rampup=200.0,
                     l_weight=1.0, u_weight=0.5, ema_decay=0.99):
    """train_DyCON_ISLES22.py:236-324, line for line; only the noise is an argument (the fixture's draw) instead of randn_like, and
    the parameter gradients are sampled before the clipping rescales them."""
    consistency_criterion = losses.softmax_mse_loss
    ema_inputs = volume_batch + noise
    _, stud_logits, stud_features = model(volume_batch)
    with torch.no_grad():
        _, ema_logits, ema_features = ema_model(ema_inputs)
    stud_probs = F.softmax(stud_logits, dim=1)
    ema_probs = F.softmax(ema_logits, dim=1)
    consistency_weight = consistency * ramps.sigmoid_rampup(iter_num // 150, consistency_rampup)
    loss_seg = ce_loss(stud_logits[:labeled_bs], label_batch[:labeled_bs].long())
    loss_seg_dice = dice_loss(stud_probs[:labeled_bs], label_batch[:labeled_bs].unsqueeze(1))
    B, C, H, W, D = stud_features.shape
    stud_embedding_fecl = F.normalize(stud_features.reshape(B, C, -1).transpose(1, 2), dim=-1)
    ema_embedding_fecl = F.normalize(ema_features.reshape(B, C, -1).transpose(1, 2), dim=-1)
    k = (volume_batch.shape[2] // H, volume_batch.shape[3] // W, volume_batch.shape[4] // D)
    mask_con_fecl = F.avg_pool3d(label_batch.float(), kernel_size=k, stride=k)
    mask_con_fecl = (mask_con_fecl > 0.5).float()
    mask_con_fecl = mask_con_fecl.reshape(B, -1)
    assert mask_con_fecl.shape[1] == stud_embedding_fecl.shape[1]
    mask_con_fecl = mask_con_fecl.unsqueeze(1)
    f_loss = fecl_criterion(feat=stud_embedding_fecl, mask=mask_con_fecl, teacher_feat=ema_embedding_fecl, gambling_uncertainty=None,
                            epoch=epoch_num)
    u_loss = uncl_criterion(stud_logits, ema_logits, beta)
    consistency_loss = consistency_criterion(stud_probs[labeled_bs:], ema_probs[labeled_bs:]).mean()
    loss = l_weight * (loss_seg + loss_seg_dice) + consistency_weight * consistency_loss + u_weight * (f_loss + u_loss)
    assert not (torch.isnan(loss) or torch.isinf(loss))
    optimizer.zero_grad()
    loss.backward()
    gstats = {k_: (_stats(p.grad) if p.grad is not None else None) for k_, p in model.named_parameters()}
    gnorm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=1.0)
    optimizer.step()
    alpha = min(1 - 1 / (iter_num + 1), ema_decay)
    for ema_param, param in zip(ema_model.parameters(), model.parameters()):
        ema_param.data.mul_(alpha).add_(param.data, alpha=1 - alpha)
    lr_ = base_lr * (1.0 - iter_num / max_iterations) ** 0.9
    for param_group in optimizer.param_groups:
        param_group["lr"] = lr_
    return dict(loss=loss, ce=loss_seg, dice=loss_seg_dice, cons=consistency_loss, fecl=f_loss, uncl=u_loss, cw=consistency_weight,
                gnorm=gnorm, s_logits=stud_logits, t_logits=ema_logits, s_feat=stud_features, mask=mask_con_fecl, gstats=gstats)


@pytest.mark.parametrize("kind", ["unet", "vnet"])
def test_isles_step_body_three_classes(kind):
    g = {k[len(kind) + 1:]: v for k, v in load_golden("step_isles_nc3").items() if k.startswith(kind + ".")}
    net_type = "unet_3D" if kind == "unet" else "vnet"
    mk = ON.make_unet_params if kind == "unet" else ON.make_vnet_params
    s0, s1 = [int(v) for v in g["seeds"]]
    LB, NC, B, S = int(g["LB"]), int(g["classes"]), int(g["B"]), int(g["S"])
    assert NC == 3

    def create_model(seed, ema=False):
        net = net_factory_3d(net_type=net_type, in_chns=1, class_num=NC, scaler=2)
        net.load_state_dict(mk(seed, n_classes=NC))
        net = net.to(DEV)
        net.has_dropout = False               # the fixture was drawn with dropout p = 0
        if ema:
            for p in net.parameters():
                p.detach_()
        return net

    model, ema_model = create_model(s0), create_model(s1, ema=True)
    model.train(); ema_model.train()
    base_lr, max_iterations = float(g["base_lr"]), int(g["max_iterations"])
    optimizer = torch.optim.SGD(model.parameters(), lr=base_lr, momentum=0.9, weight_decay=0.0001)
    ce_loss, dice_loss = torch.nn.CrossEntropyLoss(), losses.DiceLoss(NC)
    uncl_criterion = dycon_losses.UnCLoss()
    fecl_criterion = dycon_losses.FeCLoss(device=DEV, temperature=0.6, gamma=2.0, use_focal=True, rampup_epochs=1500)
    names = [k for k, _ in model.named_parameters()]
    assert names == list(g["param_names"])
    rng = np.random.default_rng(int(g["rng_seed"]))
    for step in range(2):
        vol = T(rng.standard_normal((B, 1, S, S, S)).astype(np.float32))
        noise = torch.clamp(T(rng.standard_normal((B, 1, S, S, S)).astype(np.float32)) * 0.1, -0.2, 0.2)
        np.testing.assert_allclose(_stats(vol), g[f"s{step}.vol_stats"], rtol=1e-12)         # the fixture's draws
        np.testing.assert_allclose(_stats(noise), g[f"s{step}.noise_stats"], rtol=1e-12)
        lab = T(g[f"s{step}.label"]).long().to(DEV)
        out = _isles_step_body(model, ema_model, optimizer, ce_loss, dice_loss, uncl_criterion, fecl_criterion, vol.to(DEV), lab,
                               noise.to(DEV), LB, step, int(g[f"s{step}.epoch"]), float(g[f"s{step}.beta"]), base_lr, max_iterations)
        ref = g[f"s{step}.scalars.f64"]   # loss, ce, dice, cons, fecl, uncl, cons_weight, grad_norm -- the trace's fp64 twin
        got = [float(out[k]) for k in ("loss", "ce", "dice", "cons", "fecl", "uncl")] + [out["cw"], float(out["gnorm"])]
        print(f"step {step} scalars: got {got}\n  fp64 {list(ref)}\n  fp32 {list(g[f's{step}.scalars'])}")
        np.testing.assert_allclose(got[:7], ref[:7], rtol=1e-4, atol=1e-6, err_msg=f"loss scalars step {step}")
        np.testing.assert_allclose(got[7], ref[7], rtol=1e-4, err_msg=f"grad norm step {step}")
        np.testing.assert_array_equal(out["mask"].cpu().numpy().reshape(g[f"s{step}.mask"].shape), g[f"s{step}.mask"])
        assert out["s_logits"].shape == (B, NC, S, S, S)
        within_budget(out["s_logits"].detach().cpu()[..., ::4, ::4, ::4].numpy(), g[f"s{step}.logits_sub"], g[f"s{step}.logits_sub.f64"],
                      f"student logits step {step}")
        for key, t in (("logits_stats", out["s_logits"]), ("t_logits_stats", out["t_logits"]), ("feat_stats", out["s_feat"])):
            r64 = g[f"s{step}.{key}.f64"]
            np.testing.assert_allclose(_stats(t), r64, rtol=1e-4, atol=1e-4 * r64[1], err_msg=f"{key} step {step}")
        sp, tp = dict(model.named_parameters()), dict(ema_model.named_parameters())
        refs = dict(zip(names, g[f"s{step}.grad_stats.f64"]))
        refs32 = dict(zip(names, g[f"s{step}.grad_stats"]))

        def final_untouched(k):
            assert out["gstats"][k] is None and sp[k].grad is None       # the discarded tanh head: SGD / clip skip it (as the reference)
        _check_grad_stats(kind, sp, out["gstats"], refs, refs32, f"{kind} step {step} gradients", final_untouched)
        for k, ref_s, ref_t in zip(names, g[f"s{step}.student_stats.f64"], g[f"s{step}.teacher_stats.f64"]):
            np.testing.assert_allclose(_stats(sp[k]), ref_s, rtol=1e-4, atol=1e-4, err_msg=f"student {k} step {step}")
            np.testing.assert_allclose(_stats(tp[k]), ref_t, rtol=1e-4, atol=1e-4, err_msg=f"teacher {k} step {step}")


# ------------------------------------------------------------------------------------------------------------------- (f) evaluator
def _single_case_restated(model, image, stride_xy, stride_z, patch_size, num_classes):
    """utils/test_3d_patch.py:293-351 of the reference: one window at a time, torch.softmax, numpy accumulation"""
    w, h, d = image.shape
    pads = [max(p - s, 0) for p, s in zip(patch_size, (w, h, d))]
    add_pad = any(pads)
    lo = [p // 2 for p in pads]
    hi = [p - p // 2 for p in pads]
    if add_pad:
        image = np.pad(image, [(lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2])], mode="constant", constant_values=0)
    ww, hh, dd = image.shape
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    score_map = np.zeros((num_classes,) + image.shape).astype(np.float32)
    cnt = np.zeros(image.shape).astype(np.float32)
    for x in range(sx):
        xs = min(stride_xy * x, ww - patch_size[0])
        for y in range(sy):
            ys = min(stride_xy * y, hh - patch_size[1])
            for z in range(sz):
                zs = min(stride_z * z, dd - patch_size[2])
                patch = image[xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]]
                patch = torch.from_numpy(np.expand_dims(np.expand_dims(patch, 0), 0).astype(np.float32)).to(DEV)
                with torch.no_grad():
                    y1 = model(patch)[1]
                    y_ = torch.softmax(y1, dim=1)
                y_ = y_.cpu().numpy()[0, 1, :, :, :]
                score_map[:, xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]] += y_
                cnt[xs:xs + patch_size[0], ys:ys + patch_size[1], zs:zs + patch_size[2]] += 1
    score_map = score_map / np.expand_dims(cnt, 0)
    label_map = (score_map[0] > 0.5).astype(np.int64)
    if add_pad:
        label_map = label_map[lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d]
        score_map = score_map[:, lo[0]:lo[0] + w, lo[1]:lo[1] + h, lo[2]:lo[2] + d]
    return label_map, score_map


@pytest.mark.parametrize("net_type", ["vnet", "unet_3D"])
@pytest.mark.parametrize("shape", [(40, 36, 24), (24, 20, 10)], ids=["overlapping", "padded"])
def test_single_case_three_classes(net_type, shape):
    """40 x 36 x 24 with windows of 32 x 32 x 16 at strides 8 / 4: the windows overlap and are clamped at the far faces;
    24 x 20 x 10: smaller than the window, the padding path"""
    torch.manual_seed(3)
    model = net_factory_3d(net_type, 1, 3, 2).to(DEV).eval()
    image = np.random.default_rng(5).standard_normal(shape).astype(np.float32)
    patch = (32, 32, 16)
    label, score = T3.test_single_case(model, image, 8, 4, patch, num_classes=3, batch_size=4)
    ref_label, ref_score = _single_case_restated(model, image, 8, 4, patch, 3)
    assert score.shape == (3,) + shape and label.shape == shape and label.dtype == np.int64
    assert (score[0] == score[1]).all() and (score[0] == score[2]).all()      # the class-1 probability in every channel (:338-339)
    err = np.abs(score - ref_score).max()
    decided = np.abs(ref_score[0] - 0.5) > 1e-5
    print(f"{net_type} {shape}: |score - restated| {err:.3e}; {int((~decided).sum())} voxels within 1e-5 of the threshold; "
          f"foreground {label.mean():.3f}")
    assert err <= 1e-5
    assert (~decided).sum() < 1e-3 * decided.size
    assert (label == ref_label)[decided].all()
    assert 0 < label.sum() < label.size           # both decisions occur


def test_single_case_refuses_a_one_class_model():
    model = net_factory_3d("vnet", 1, 1, 2).to(DEV).eval()
    image = np.zeros((32, 32, 16), np.float32)
    with pytest.raises(ValueError, match="at least 2 classes"):
        T3.test_single_case(model, image, 8, 4, (32, 32, 16), num_classes=1)
