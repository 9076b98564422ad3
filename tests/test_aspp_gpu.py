"""GPU parity of UNet3D(use_aspp=True): the dilated convolution over its live taps against F.conv3d, the engine's ASPP against the
reference's ASPP3D (tests/golden/aspp.npz), the whole net and one training step against torch restatements, replay and checkpoints."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_aspp_cpu import ASPP_CASES, aspp_case
from test_fullsize_gpu import assert_bf16_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STRIDE = 199         # tests/golden/make_golden_aspp.py


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def aspp_ref(x, p, bn_training=True, update_buffers=False, drop_mask=None):
    """ASPP3D.forward (networks/assp.py:56-73) restated on a flat parameter dict with 'aspp.' keys; drop_mask: keep-mask of the
    element-wise Dropout(0.5)."""
    def bn(z, site):
        rm, rv = p[site + ".running_mean"], p[site + ".running_var"]
        if bn_training and not update_buffers:
            rm, rv = rm.clone(), rv.clone()
        elif bn_training:
            p[site + ".num_batches_tracked"] += 1
        return F.batch_norm(z, rm, rv, p[site + ".weight"], p[site + ".bias"], bn_training, 0.1, 1e-5)

    outs = []
    for j, d in enumerate((1, 6, 12, 18)):
        w = p[f"aspp.aspp{j + 1}.atrous_conv.weight"]
        z = F.conv3d(x, w) if j == 0 else F.conv3d(x, w, padding=d, dilation=d)
        outs.append(F.relu(bn(z, f"aspp.aspp{j + 1}.bn")))
    v = F.conv3d(F.adaptive_avg_pool3d(x, 1), p["aspp.global_avg_pool.1.weight"])
    if x.shape[0] > 1:
        v = bn(v, "aspp.bn_after_pool")
    v = F.interpolate(F.relu(v), size=x.shape[2:], mode="trilinear", align_corners=True)
    y = F.relu(bn(F.conv3d(torch.cat(outs + [v], 1), p["aspp.conv1.weight"]), "aspp.bn1"))
    return y if drop_mask is None else y * (drop_mask.to(y.dtype) / 0.5)


# ------------------------------------------------------------------------------------------------ dilated convolution
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,dhw,cin,cout,d", [
    (2, (7, 9, 5), 32, 48, 1), (1, (7, 7, 5), 64, 32, 6), (2, (13, 20, 7), 32, 16, 12), (1, (19, 11, 21), 16, 32, 18),
    (2, (6, 6, 4), 32, 32, 6)])
def test_dilated_conv_vs_torch(dtype, B, dhw, cin, cout, d):
    from dycon_paper_replication_amd.aspp import (TapPlan, dilated_conv3d, dilated_conv3d_bwd_data,
                                                  dilated_conv3d_bwd_weight)
    g = torch.Generator().manual_seed(d * 100 + cin)
    x = torch.randn((B, cin) + dhw, generator=g).to(DEV).to(dtype).float()
    w = (torch.randn((cout, cin, 3, 3, 3), generator=g) * (2.0 / (cin * 27)) ** 0.5).to(DEV)
    gy = torch.randn((B, cout) + dhw, generator=g).to(DEV).to(dtype).float()
    wq = w.to(dtype).float()
    xr = x.clone().requires_grad_(True)
    wr = wq.clone().requires_grad_(True)
    yr = F.conv3d(xr, wr, padding=d, dilation=d)
    yr.backward(gy)
    y = ncdhw(dilated_conv3d(ndhwc(x).to(dtype), w, d)).float()
    gx = ncdhw(dilated_conv3d_bwd_data(ndhwc(gy).to(dtype), w, d)).float()
    gw = dilated_conv3d_bwd_weight(ndhwc(x).to(dtype), ndhwc(gy).to(dtype), d)
    live = TapPlan(dhw, [(3, d)]).live(0)
    pruned = [t for t in range(27) if t not in live]
    assert torch.all(gw.reshape(cout, cin, 27)[:, :, pruned] == 0)
    if dtype == torch.float32:
        for got, ref, what in ((y, yr, "y"), (gx, xr.grad, "gx"), (gw, wr.grad, "gw")):
            err = float((got - ref.detach()).abs().max()) / max(float(ref.abs().max()), 1e-30)
            assert err <= 1e-4, (what, err)
    else:
        assert_bf16_elementwise(y, yr.detach(), f"y d={d}")
        assert_bf16_elementwise(gx, xr.grad, f"gx d={d}")
        err = float((gw - wr.grad).abs().max()) / float(wr.grad.abs().max())
        assert err <= 1e-2, err          # fp32 accumulation of bf16 products: the weight gradient is stored in fp32


# ------------------------------------------------------------------------------------------------ engine ASPP vs the reference
def _engine_aspp(params, bufs, x, gy, dtype, training):
    from dycon_paper_replication_amd.engine import DropoutSpec, Engine
    p = {k: v.float().to(DEV).contiguous() for k, v in params.items()}
    b = {k: v.to(DEV).clone() if k.endswith("tracked") else v.float().to(DEV).clone() for k, v in bufs.items()}
    g = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    eng = Engine("unet_3D", p, g, b, dtype)
    eng.recording, eng.update_bn, eng.dropout = True, True, DropoutSpec("off")
    eng.tape, eng.G, eng.Gs = [], {}, {}
    xd = ndhwc(x.float().to(DEV)).to(dtype)
    y = eng._aspp(xd, training)
    eng._put(y, ndhwc(gy.float().to(DEV)).to(dtype))
    for f in reversed(eng.tape):
        f()
    return ncdhw(y).float(), ncdhw(eng.G[id(xd)]).float(), g, b


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", range(len(ASPP_CASES)))
def test_engine_aspp_vs_reference(case, mode):
    gold = load_golden("aspp")
    name, B, dhw = ASPP_CASES[case]
    params, bufs, x, gy = aspp_case(100 + case, B, dhw, torch.float64)
    y, gx, g, b = _engine_aspp(params, bufs, x, gy, torch.float32, mode == "train")
    pre = f"{name}_{mode}_"
    assert _rel(y.cpu().reshape(-1)[::STRIDE], gold[pre + "y"]) <= 1e-4, "y"
    assert abs(float(y.norm()) / float(gold[pre + "y_norm"]) - 1) <= 1e-5
    if mode == "eval":     # eval: the forward (running statistics); the step never differentiates an eval-mode net
        return
    assert _rel(gx.cpu().reshape(-1)[::STRIDE], gold[pre + "gx"]) <= 1e-4, "gx"
    for k, v in g.items():
        key = pre + "g." + k[len("aspp."):]
        if key not in gold:                     # bn_after_pool with one sample: no gradient in the reference either
            assert B == 1 and "bn_after_pool" in k
            continue
        got = v.cpu()
        if float(np.abs(gold[key]).max()) < 1e-9:
            # one sample: bn1 removes the pool branch's spatially constant share, so its gradients are 0 up to round-off
            assert B == 1 and float(got.abs().max()) < 1e-3, k
            continue
        if got.dim() == 5:
            assert abs(float(got.norm()) / float(gold[pre + "gnorm." + k[len("aspp."):]]) - 1) <= 1e-4, k
            got = got[:4, :4]
        else:
            got = got[::4]
        assert _rel(got, gold[key]) <= 2e-4, k
    if mode == "train":
        for k, v in b.items():
            key = pre + "buf." + k[len("aspp."):]
            if k.endswith("num_batches_tracked"):
                assert int(v) == (0 if (B == 1 and "bn_after_pool" in k) else 1), k
            else:
                assert _rel(v.cpu()[::4], gold[key]) <= 1e-4, k


def test_engine_aspp_bf16_and_two_launches_same_bits():
    params, bufs, x, gy = aspp_case(7, 2, (7, 7, 5), torch.float64)
    y1, gx1, g1, _ = _engine_aspp(params, bufs, x, gy, torch.bfloat16, True)
    y2, gx2, g2, _ = _engine_aspp(params, bufs, x, gy, torch.bfloat16, True)
    assert torch.equal(y1, y2) and torch.equal(gx1, gx2) and all(torch.equal(g1[k], g2[k]) for k in g1)
    p = {k: v.float() for k, v in params.items()}
    p.update({k: (v.clone() if k.endswith("tracked") else v.float().clone()) for k, v in bufs.items()})
    xr = x.float().to(torch.bfloat16).float().requires_grad_(True)
    yr = aspp_ref(xr, p, True, False)
    yr.backward(gy.float())
    rms = float(yr.pow(2).mean().sqrt())
    assert float((y1.cpu() - yr.detach()).abs().max()) <= 0.05 * float(yr.abs().max())
    # bf16 storage of every intermediate, and the BatchNorm backwards cancel: a loose bound (the fp32 path is held to 1e-4 above)
    assert float((gx1.cpu() - xr.grad).pow(2).mean().sqrt()) <= 0.15 * float(xr.grad.pow(2).mean().sqrt()) + 1e-3 * rms


# ------------------------------------------------------------------------------------------------ whole net, trainer
def _unet_aspp_params(seed):
    from oracle import nets as ON
    p = ON.make_unet_params(seed)
    params, bufs, _, _ = aspp_case(seed, 1, (1, 1, 1), torch.float32)
    sd = {}
    for k in p:                       # reference order: the ASPP between out_conv2 and the projection head
        if k == "projection.0.weight":
            sd.update(params)
            sd.update({b: (v if b.endswith("tracked") else torch.zeros_like(v) if b.endswith("mean") else torch.ones_like(v))
                       for b, v in bufs.items()})
        sd[k] = p[k]
    return sd


def test_unet_aspp_module_vs_torch(monkeypatch):
    """UNet3D(use_aspp=True) forward + backward (fp32, explicit dropout masks) against oracle.nets' U-Net with the ASPP
    restated in front of its projection head; 112 x 112 x 32 gives a 7 x 7 x 2 bottleneck with 9 live taps in aspp2."""
    from oracle import nets as ON
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    sd = _unet_aspp_params(3)
    net = net_factory_3d("unet_3D", scaler=2, use_aspp=True).to(DEV)
    net.load_state_dict({k: v.to(DEV) for k, v in sd.items()})
    B, dhw = 2, (112, 112, 32)
    g = torch.Generator().manual_seed(11)
    x = torch.randn((B, 1) + dhw, generator=g)
    masks = {"drop_center": (torch.rand((B,) + tuple(s // 16 for s in dhw) + (256,), generator=g) > 0.3),
             "drop_up1": (torch.rand((B,) + dhw + (16,), generator=g) > 0.3),
             "drop_aspp": (torch.rand((B,) + tuple(s // 16 for s in dhw) + (256,), generator=g) > 0.5)}
    monkeypatch.setattr(net, "_dropout_spec", lambda: DropoutSpec("mask", {k: v.to(DEV).float() for k, v in masks.items()}))
    _, logits, feats = net(x.to(DEV))
    wl = torch.randn(logits.shape, generator=g)
    wf = torch.randn(feats.shape, generator=g)
    ((logits * wl.to(DEV)).sum() + (feats * wf.to(DEV)).sum()).backward()

    orig = ON.projection_head
    cm = lambda m: m.permute(0, 4, 1, 2, 3)       # noqa: E731
    monkeypatch.setattr(ON, "projection_head", lambda c, p, s, bn_training=True, update_buffers=False: orig(
        aspp_ref(c, p, bn_training, update_buffers, cm(masks["drop_aspp"])), p, s, bn_training, update_buffers))
    # the restatement runs in fp64: the fp32 engine is compared with the exact result, not with another fp32 rounding path
    p = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k
             else v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}
    _, lr_, fr = ON.unet_forward(x.double(), p, net.scale_factor, cm(masks["drop_center"]), cm(masks["drop_up1"]), True, True)
    ((lr_ * wl.double()).sum() + (fr * wf.double()).sum()).backward()
    assert _rel(logits.detach().cpu(), lr_.detach()) <= 1e-4
    assert _rel(feats.detach().cpu(), fr.detach()) <= 2e-4
    named = dict(net.named_parameters())
    for k in ("aspp.aspp1.atrous_conv.weight", "aspp.aspp2.atrous_conv.weight", "aspp.aspp4.atrous_conv.weight",
              "aspp.global_avg_pool.1.weight", "aspp.conv1.weight", "aspp.bn1.weight", "aspp.aspp2.bn.bias",
              "aspp.bn_after_pool.weight", "center.conv2.0.weight", "conv1.conv1.0.weight", "projection.0.weight"):
        # fp32 gradients of the whole net sit at ~1% of the fp64 restatement without the ASPP already (projection.0: 0.85%,
        # the decoder's deep levels 0.4-1% at this patch); bn1 over 196 rows amplifies that on the feature branch.  The ASPP
        # alone is held to 2e-4 against the reference in test_engine_aspp_vs_reference.
        assert _rel(named[k].grad.cpu(), p[k].grad) <= 0.15, k
    sdn = net.state_dict()
    for k in ("aspp.aspp3.bn.running_var", "aspp.bn1.running_mean", "aspp.bn_after_pool.running_mean"):
        assert _rel(sdn[k].cpu(), p[k]) <= 5e-4, k      # (means of fp32 activations 15 layers deep; the ASPP alone: 1e-4 above)
    assert int(sdn["aspp.bn1.num_batches_tracked"]) == 1


def test_trainer_step_vs_oracle(monkeypatch):
    """One fp32 DyconTrainer step with use_aspp=True against oracle.step.train_step, the ASPP restated in front of the head."""
    from oracle import nets as ON
    from oracle import step as OS
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    orig = ON.projection_head
    monkeypatch.setattr(ON, "projection_head", lambda c, p, s, bn_training=True, update_buffers=False: orig(
        aspp_ref(c, p, bn_training, update_buffers), p, s, bn_training, update_buffers))
    vol, lab, noise = make_batch(21, 2, (112, 112, 32))
    s0, t0 = _unet_aspp_params(1), _unet_aspp_params(2)
    cfg = TrainConfig(model="unet_3D", use_aspp=True, labeled_bs=1, batch_size=2, dtype=torch.float32)
    tr = DyconTrainer(cfg, DEV, student_init=s0, teacher_init=t0)
    off = DropoutSpec("off")
    out = tr.step(vol.to(DEV), lab.to(DEV), noise=noise.to(DEV), s_drop=off, t_drop=off, epoch=0, beta=5.0)
    st = OS.StepState(student={k: v.clone() for k, v in s0.items()}, teacher={k: v.clone() for k, v in t0.items()})
    ref = OS.train_step(OS.StepConfig(net_type="unet_3D", labeled_bs=1), st, vol, lab, noise, 5.0, 0)
    got = np.array([float(out[k]) for k in ("loss", "ce", "dice", "cons", "fecl", "uncl")])
    exp = np.array([float(ref[k]) for k in ("loss", "ce", "dice", "cons", "fecl", "uncl")])
    np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-6)
    for k in ("aspp.aspp2.atrous_conv.weight", "aspp.conv1.weight", "aspp.global_avg_pool.1.weight", "aspp.bn1.weight",
              "aspp.aspp3.bn.bias", "projection.0.weight", "center.conv1.0.weight"):
        assert _rel(tr.p[k].cpu() - s0[k], st.student[k] - s0[k]) <= 0.15, k      # the update (gradient precision: see above)
    assert _rel(tr.s_buf["aspp.bn1.running_var"].cpu(), st.student["aspp.bn1.running_var"]) <= 1e-4
    assert _rel(tr.t_buf["aspp.aspp1.bn.running_mean"].cpu(), st.teacher["aspp.aspp1.bn.running_mean"]) <= 1e-4


def test_replay_equals_eager_and_checkpoint(tmp_path):
    """bf16, on-device dropout: five replayed steps give the eager run's bits; the checkpoint has the reference's keys and
    loads back into UNet3D(use_aspp=True) and into a fresh trainer."""
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    import json
    batches = [make_batch(600 + i, 2, (112, 112, 16)) for i in range(5)]
    runs = {}
    for replay in (False, True):
        tr = DyconTrainer(TrainConfig(model="unet_3D", use_aspp=True, labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=4,
                                      replay=replay), DEV)
        losses = [float(tr.step(v.to(DEV), l.to(DEV))["loss"]) for v, l, _ in batches]
        assert (tr._rp is not None) == replay
        runs[replay] = (losses, tr.flat_p.clone(), tr.flat_t.clone(), {k: v.clone() for k, v in tr.s_buf.items()})
    assert runs[True][0] == runs[False][0]
    assert torch.equal(runs[True][1], runs[False][1]) and torch.equal(runs[True][2], runs[False][2])
    assert all(torch.equal(runs[True][3][k], runs[False][3][k]) for k in runs[True][3])
    assert all(np.isfinite(runs[True][0]))
    path = str(tmp_path / "aspp.pth")
    tr.save_checkpoint(path)
    sd = torch.load(path, map_location="cpu")
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aspp_keys.json")) as f:
        ref = json.load(f)
    assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, list(s)) for k, s in ref]
    m = net_factory_3d("unet_3D", use_aspp=True)
    m.load_state_dict(sd)
    assert torch.equal(m.state_dict()["aspp.conv1.weight"], sd["aspp.conv1.weight"])
    tr2 = DyconTrainer(TrainConfig(model="unet_3D", use_aspp=True, labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=5), DEV)
    tr2.load_checkpoint(path)
    assert torch.equal(tr2.p["aspp.aspp2.atrous_conv.weight"].cpu(), sd["aspp.aspp2.atrous_conv.weight"])
    assert torch.equal(tr2.s_buf["aspp.bn1.running_mean"].cpu(), sd["aspp.bn1.running_mean"])


def test_module_keys_and_init():
    """UNet3D(use_aspp=True) / net_factory_3d: the reference's state-dict keys and shapes in order, 11 918 772 parameters, the ASPP's
    BatchNorm weights ~ N(1, 0.02) and biases 0 (UNet3D.__init__'s loop runs after build_aspp3d)."""
    import json
    from dycon_paper_replication_amd.networks.UNet3D_contrastive import UNet3D
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aspp_keys.json")) as f:
        ref = json.load(f)
    for m in (net_factory_3d("unet_3D", use_aspp=True), UNet3D(use_aspp=True)):
        sd = m.state_dict()
        assert [(k, list(v.shape)) for k, v in sd.items()] == [(k, list(s)) for k, s in ref]
        assert sum(p.numel() for p in m.parameters()) == 11918772
        w = sd["aspp.bn1.weight"]
        assert abs(float(w.mean()) - 1.0) < 0.01 and 0.005 < float(w.std()) < 0.04
        assert float(sd["aspp.aspp2.bn.bias"].abs().max()) == 0.0
