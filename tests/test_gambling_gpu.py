"""Gambling-softmax uncertainty on the GPU: the public gambling_softmax, the fused u and its adjoint, FeCLoss with a differentiable u
against the reference (tests/golden/gambling.npz), and the step with TrainConfig(use_gambling=1) against the oracle, replayed."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_gambling_cpu import (FECL_COMBOS, GAMBLING_CASES, STRIDE_FEAT, STRIDE_LOGITS, contrast_mask, embed, entropy_ref,
                               gambling_case, gambling_softmax_ref, overflow_logits, uncertainty_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


def pancreas_u(stud_logits, k):
    """train_DyCON_Pancreas.py:242-246 as written, on this package's gambling_softmax"""
    from dycon_paper_replication_amd.utils import dycon_losses
    B = stud_logits.shape[0]
    p_gs = dycon_losses.gambling_softmax(stud_logits)
    entropy = -torch.sum(p_gs * torch.log(p_gs + 1e-6), dim=1, keepdim=True)
    entropy = F.interpolate(entropy, scale_factor=1 / k, mode="trilinear", align_corners=False).squeeze(1)
    return entropy.view(B, -1)


@pytest.mark.parametrize("C", [1, 2, 3, 8])
def test_gambling_softmax_vs_fp64(C):
    from dycon_paper_replication_amd.utils import dycon_losses
    g = torch.Generator().manual_seed(C)
    x = (4 * torch.randn(3, C, 17, 9, 6, generator=g)).float()
    w = torch.randn(3, C, 17, 9, 6, generator=g).float()
    xd = x.to(DEV).requires_grad_(True)
    y = dycon_losses.gambling_softmax(xd)
    (y * w.to(DEV)).sum().backward()
    xr = x.double().requires_grad_(True)
    yr = gambling_softmax_ref(xr)
    (yr * w.double()).sum().backward()
    assert y.shape == x.shape and y.dtype == torch.float32
    assert torch.isfinite(y).all()
    assert (y.detach().cpu().double() - yr.detach()).abs().max() <= 1e-5 * yr.detach().abs().max()
    if C == 1:       # p = e / (e + 1e-18) == 1: the gradient vanishes
        assert xd.grad.abs().max() <= 1e-6
    else:
        assert _rel(xd.grad, xr.grad) <= 1e-5


def test_gambling_softmax_unaligned_and_tail():
    """operands that are not 16-byte aligned take the scalar kernel; nvox % 4 trailing voxels are covered by both"""
    from dycon_paper_replication_amd import ops
    g = torch.Generator().manual_seed(11)
    for C, nvox in ((2, 4099), (3, 1027), (8, 4)):
        x = (3 * torch.randn(nvox, C, generator=g)).float()
        gy = torch.randn(nvox, C, generator=g).float()
        buf = torch.empty(nvox * C + 1, device=DEV)
        xa = buf[1:].view(nvox, C)
        xa.copy_(x.to(DEV))
        for xin in (x.to(DEV), xa):
            y = ops.gambling_softmax(xin)
            gx = ops.gambling_softmax_bwd(y, gy.to(DEV))
            yr = gambling_softmax_ref(x.double())
            assert (y.cpu().double() - yr).abs().max() <= 1e-6
            gr = yr * (gy.double() - (gy.double() * yr).sum(-1, keepdim=True))
            assert _rel(gx, gr) <= 1e-5
    with pytest.raises(ValueError):
        ops.gambling_softmax(torch.zeros(4, 9, device=DEV))
    with pytest.raises(ValueError):
        ops.gambling_uncertainty(torch.zeros(1, 8, 8, 8, 3, device=DEV), 4)
    with pytest.raises(ValueError):
        ops.gambling_uncertainty(torch.zeros(1, 8, 8, 8, 2, device=DEV, dtype=torch.bfloat16), 4)


def test_gambling_softmax_overflow_nan_positions():
    from dycon_paper_replication_amd.utils import dycon_losses
    x = overflow_logits()
    y = dycon_losses.gambling_softmax(x.to(DEV)).cpu()
    yr = gambling_softmax_ref(x)          # fp32, as the reference runs on fp32 logits
    assert torch.equal(torch.isnan(y), torch.isnan(yr)) and int(torch.isnan(y).sum()) == 4     # inf / inf in the overflowing channel
    ok = ~torch.isnan(yr)
    assert (y[ok] - yr[ok]).abs().max() <= 1e-6


@pytest.mark.parametrize("shape", [(96, 96, 96), (112, 112, 80)])
@pytest.mark.parametrize("k", [2, 4, 8, 16])
def test_fused_uncertainty_and_adjoint(shape, k):
    """u and g_logits += gu * du/dlogits against F.interpolate + autograd in fp64, fp32 (libm) and fast (bf16 step) forms"""
    from dycon_paper_replication_amd import ops
    B = {2: 1, 4: 2, 8: 3, 16: 4}[k]
    g = torch.Generator().manual_seed(k * 7 + shape[2])
    logits = (3 * torch.randn(B, 2, *shape, generator=g)).float()
    ld = logits.double().requires_grad_(True)
    ur = uncertainty_ref(ld, k)
    gu = torch.randn(ur.shape, generator=g).float()
    (ur * gu.double()).sum().backward()
    x = logits.permute(0, 2, 3, 4, 1).contiguous().to(DEV)
    base = torch.randn(x.shape, generator=g).float().to(DEV)
    sampled = torch.zeros(logits.shape, dtype=torch.bool)
    idx = [torch.tensor([k * i + k // 2 - 1 + o for i in range(n // k) for o in (0, 1)]) for n in shape]
    sampled[:, :, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]] = True
    for fast, tol_u, tol_g in ((False, 2e-6, 2e-5), (True, 2e-5, 1e-4)):
        u = ops.gambling_uncertainty(x, k, fast=fast)
        assert u.shape == ur.shape
        assert _rel(u, ur.detach()) <= tol_u
        gl = base.clone()
        ops.gambling_uncertainty_bwd(x, k, gu.to(DEV), gl, fast=fast)
        torch.cuda.synchronize()
        got = (gl - base).permute(0, 4, 1, 2, 3).cpu()
        assert _rel(got, ld.grad) <= tol_g
        assert float(got[~sampled].abs().sum()) == 0.0             # only the 8 voxels of each patch are touched
    with pytest.raises(ValueError):
        ops.gambling_uncertainty(x, 3)


def _fecl_on_gpu(i, focal, teacher, epoch, dtype=torch.float32):
    from dycon_paper_replication_amd.utils import dycon_losses
    logits, sf, tf, label, k = gambling_case(i, torch.float32)
    lg = logits.to(DEV).requires_grad_(True)
    f = sf.float().to(DEV).requires_grad_(True)
    crit = dycon_losses.FeCLoss(device=DEV, temperature=0.6, gamma=2.0, use_focal=bool(focal), rampup_epochs=1500)
    u = pancreas_u(lg, k)
    loss = crit(feat=embed(f).to(dtype), mask=contrast_mask(label, k).float().to(DEV),
                teacher_feat=embed(tf.float().to(DEV)).to(dtype) if teacher else None, gambling_uncertainty=u, epoch=epoch)
    loss.backward()
    return loss.detach().cpu(), f.grad.cpu(), lg.grad.cpu()


@pytest.mark.parametrize("i", range(len(GAMBLING_CASES)))
def test_fecl_differentiable_u_vs_reference(i):
    """the reference's Pancreas lines on this package, fp32 (fecl_kernel family): loss, d/dfeat and d/dlogits against the reference"""
    g = load_golden("gambling")
    for focal, teacher, epoch in FECL_COMBOS:
        key = f"c{i}_f{focal}_t{teacher}_e{epoch}"
        loss, gf, gl = _fecl_on_gpu(i, focal, teacher, epoch)
        assert abs(float(loss) - float(g[key + "_loss"])) <= 1e-4 * abs(float(g[key + "_loss"])), key
        np.testing.assert_allclose(gf.flatten()[::STRIDE_FEAT].numpy(), g[key + "_gfeat"], rtol=1e-3, atol=1e-6, err_msg=key)
        assert abs(float(gf.norm()) - float(g[key + "_gfeat_norm"])) <= 1e-4 * float(g[key + "_gfeat_norm"]), key
        np.testing.assert_allclose(gl.flatten()[::STRIDE_LOGITS].numpy(), g[key + "_glogits"], rtol=1e-3, atol=1e-6, err_msg=key)
        assert abs(float(gl.norm()) - float(g[key + "_glogits_norm"])) <= 1e-4 * float(g[key + "_glogits_norm"]), key
        assert float(gl.abs().sum()) > 0
    a = _fecl_on_gpu(i, 1, 1, 0)
    b = _fecl_on_gpu(i, 1, 1, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b))          # deterministic: no float atomics on the row terms


def test_fecl_overflow_reaches_loss():
    from dycon_paper_replication_amd.utils import dycon_losses
    _, sf, tf, label, k = gambling_case(0, torch.float32)
    u = pancreas_u(overflow_logits().to(DEV).requires_grad_(True), k)
    crit = dycon_losses.FeCLoss(device=DEV, use_focal=True, rampup_epochs=1500)
    loss = crit(feat=embed(sf.float().to(DEV)), mask=contrast_mask(label, k).float().to(DEV), teacher_feat=embed(tf.float().to(DEV)),
                gambling_uncertainty=u, epoch=0)
    assert torch.isnan(loss).item()


@pytest.mark.parametrize("N", [1728, 1100])
def test_fecl_differentiable_u_bf16_rows128(N):
    """bf16 at N >= 1024 (the 128-row kernels): loss, d/dfeat, d/du against the fp64 restatement (relclose 2e-2), same bits twice"""
    from oracle import losses as OL
    from dycon_paper_replication_amd.utils import dycon_losses
    g = torch.Generator().manual_seed(N)
    B, Dm = 2, 128
    raw = torch.randn(B, N, Dm, generator=g)
    traw = raw + 0.7 * torch.randn(B, N, Dm, generator=g)
    mask = (torch.rand(B, N, generator=g) > 0.6).float()
    u0 = torch.rand(B, N, generator=g)

    def run():
        f = F.normalize(raw.to(DEV), dim=-1).bfloat16().requires_grad_(True)
        t = F.normalize(traw.to(DEV), dim=-1).bfloat16()
        u = u0.to(DEV).requires_grad_(True)
        loss = dycon_losses.FeCLoss(device=DEV, use_focal=True, rampup_epochs=1500)(f, mask.to(DEV), t, u, epoch=700)
        loss.backward()
        return loss.detach().float().cpu(), f.grad.float().cpu(), u.grad.cpu()

    l1, gf1, gu1 = run()
    l2, gf2, gu2 = run()
    assert torch.equal(l1, l2) and torch.equal(gf1, gf2) and torch.equal(gu1, gu2)
    f = F.normalize(raw, dim=-1).bfloat16().double().requires_grad_(True)
    t = F.normalize(traw, dim=-1).bfloat16().double()
    u = u0.double().requires_grad_(True)
    lr_ = OL.fecl(f, mask.double().unsqueeze(1), t, u, 700, 0.6, 2.0, True, 1500, 1.0)
    lr_.backward()
    assert abs(float(l1) - float(lr_.detach())) <= 2e-2 * abs(float(lr_.detach()))
    assert _rel(gf1, f.grad) <= 2e-2
    assert _rel(gu1, u.grad) <= 2e-2


def _gambling_losses(monkeypatch):
    """oracle.step.losses_from_outputs with u = train_DyCON_Pancreas.py:242-246 (per-axis factor of the feature grid) into FeCL;
    state["detach"] = True cuts u's gradient (what the step would compute without the adjoint into the logits)"""
    from oracle import losses as L
    from oracle import step as OS
    orig_fecl = L.fecl
    state = {"detach": False}

    def patched(cfg, s_logits, s_feat, t_logits, t_feat, label, beta, epoch, iter_num):
        k = tuple(label.shape[1 + a] // s_feat.shape[2 + a] for a in range(3))
        u = uncertainty_ref(s_logits, k)
        state["u"] = u.detach() if state["detach"] else u
        return orig(cfg, s_logits, s_feat, t_logits, t_feat, label, beta, epoch, iter_num)

    def fecl_u(feat, mask, teacher_feat=None, gambling_uncertainty=None, *a, **kw):
        return orig_fecl(feat, mask, teacher_feat, state["u"], *a, **kw)

    orig = OS.losses_from_outputs
    monkeypatch.setattr(OS, "losses_from_outputs", patched)
    monkeypatch.setattr(L, "fecl", fecl_u)
    return state


@pytest.mark.parametrize("model", ["vnet", "unet_3D"])
def test_trainer_step_vs_oracle(model, monkeypatch):
    """one fp32 step with use_gambling=1 against oracle.step.train_step with the gambling term, run in fp64: the six scalars, and
    the step's raw (pre-clip) gradient parameter by parameter.  The FeCL gradient that reaches the logits through u is checked on
    its own: the oracle's gradient with u detached differs from the full one by D in the segmentation head, and the step's error
    there must be a small fraction of D (a dropped adjoint, a wrong scale or coefficient would leave an error of order D)."""
    from oracle import nets as ON
    from oracle import step as OS
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    state = _gambling_losses(monkeypatch)
    vol, lab, noise = make_batch(31, 2, (64, 64, 32))
    mk = ON.make_vnet_params if model == "vnet" else ON.make_unet_params
    s0, t0 = mk(41), mk(42)
    cfg = TrainConfig(model=model, labeled_bs=1, batch_size=2, dtype=torch.float32, use_gambling=1)
    tr = DyconTrainer(cfg, DEV, student_init=s0, teacher_init=t0)
    off = DropoutSpec("off")
    out = tr.step(vol.to(DEV), lab.to(DEV), noise=noise.to(DEV), s_drop=off, t_drop=off, epoch=0, beta=5.0)
    torch.cuda.synchronize()
    got_g = {k: v.double().cpu() for k, v in tr.g.items()}
    dbl = lambda p: {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in p.items()}  # noqa: E731
    refs = {}
    for detach in (False, True):
        state["detach"] = detach
        st = OS.StepState(student=dbl(s0), teacher=dbl(t0))
        refs[detach] = OS.train_step(OS.StepConfig(net_type=model, labeled_bs=1), st, vol.double(), lab, noise.double(), 5.0, 0)
    ref = refs[False]
    got = np.array([float(out[k]) for k in ("loss", "ce", "dice", "cons", "fecl", "uncl")])
    exp = np.array([float(ref[k]) for k in ("loss", "ce", "dice", "cons", "fecl", "uncl")])
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-6)
    gh = torch.cat([got_g[k].reshape(-1) for k in ref["grads"]])
    gr = torch.cat([ref["grads"][k].reshape(-1) for k in ref["grads"]])
    cos = float((gh * gr).sum() / (gh.norm() * gr.norm()))
    assert cos >= 0.9999, cos
    head = "out_conv.weight" if model == "vnet" else "out_conv2.weight"
    for k in (head, head.replace("weight", "bias")):
        g64, g64_det = ref["grads"][k], refs[True]["grads"][k]
        err, contrib = float((got_g[k] - g64).norm()), float((g64 - g64_det).norm())
        print(f"{k}: |step - oracle| {err:.3e}, |u-path contribution| {contrib:.3e}, |grad| {float(g64.norm()):.3e}")
        assert contrib > 1e-3 * float(g64.norm()), k       # the u path is really in play
        assert err <= 1e-3 * contrib, (k, err, contrib)


@pytest.mark.parametrize("model,scaler,extra", [("vnet", 2, {}), ("unet_3D", 4, {"use_aspp": True, "teacher_mode": "eval"})])
def test_replay_equals_eager(model, scaler, extra):
    """bf16, on-device dropout, the flag on: five replayed steps give the eager run's bits"""
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    patch = (96, 96, 96) if model == "vnet" else (112, 112, 80)
    batches = [make_batch(700 + i, 2, patch) for i in range(5)]
    runs = {}
    for replay in (False, True):
        tr = DyconTrainer(TrainConfig(model=model, feature_scaler=scaler, labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=3,
                                      use_gambling=1, replay=replay, **extra), DEV)
        losses = [(float(o["loss"]), float(o["fecl"])) for o in (tr.step(v.to(DEV), l.to(DEV)) for v, l, _ in batches)]
        assert (tr._rp is not None) == replay
        runs[replay] = (losses, tr.flat_p.clone(), tr.flat_t.clone())
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1]) and torch.equal(runs[True][2], runs[False][2])
    assert all(np.isfinite(runs[True][0]).ravel())
