#!/usr/bin/env python3
"""Golden fixtures for class counts other than 2 by IMPORTING the reference on CPU (make_golden.py's stub-package recipe).

Stores data only:
  uncl_nc.npz        reference UnCLoss on (2, C, 6, 5, 7) logits, C in {1, 3, 4, 8}: per C a unit-scale pair `c{C}` and a pair `c{C}_big`
                     with logits up to +-30 (where p + 1e-6 is in force); per beta in {0.5, 2.0, 5.0} the loss and the student
                     gradient, fp32 and fp64
  full_nets_nc.npz   make_golden._full_nets' recipe (input, seeds, cotangents, statistics) for the V-Net (VNetWithHead) at C = 3, 1, 8
                     and UNet3D at C = 3; keys `{net}{C}.*`; the parameter names and shapes of every net (state-dict contract).
                     Sub-sampling: logits `_sub` (every 2nd voxel; the 8-class V-Net every 4th), features `_sub` + statistics
  step_isles_nc3.npz make_golden._ref_step_trace's recipe (B = 2, LB = 1, S = 32, two steps, dropout p = 0, fp32 + fp64 twin) driving
                     the ISLES body (train_DyCON_ISLES22.py:236-324) with 3 classes, `unet.*` and `vnet.*`.  Volumes and noise
                     are rebuilt by the test from `rng_seed` (per step: volume, then noise); the labels are stored

    python tests/golden/make_golden_nclasses.py [uncl] [full] [steps]
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/code"

for pkg in ("networks", "utils"):
    m = types.ModuleType(pkg)
    m.__path__ = [f"{REF}/{pkg}"]
    sys.modules[pkg] = m
ref_dycon = importlib.import_module("utils.dycon_losses")
ref_losses = importlib.import_module("utils.losses")
ref_ramps = importlib.import_module("utils.ramps")
ref_vnet = importlib.import_module("networks.VNet")
ref_factory = importlib.import_module("networks.net_factory_3d")

from oracle import nets as onets  # noqa: E402  (parameter builders only)

torch.set_num_threads(8)


def rng_t(rng, *shape, scale=1.0):
    return torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))


def save(name, **arrs):
    out = {}
    for k, v in arrs.items():
        if torch.is_tensor(v):
            v = v.detach().cpu().numpy()
        out[k] = np.asarray(v)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"  {name}.npz  {os.path.getsize(path) / 1024:.0f} KiB on disk")


def stats(t):
    if t is None:          # parameter unused by the loss (UNet3D.final in the training step)
        return np.zeros(3)
    t = t.detach().double()
    return np.array([t.sum().item(), t.abs().sum().item(), (t * t).sum().item()])


def _sub(t):
    return t[..., ::2, ::2, ::2]


# ----------------------------------------------------------------------------- UnCL
UNCL_CLASSES, UNCL_BETAS, UNCL_SHAPE = (1, 3, 4, 8), (0.5, 2.0, 5.0), (6, 5, 7)


def gen_uncl():
    rng = np.random.default_rng(1101)
    crit = ref_dycon.UnCLoss()
    out = {"classes": np.array(UNCL_CLASSES), "betas": np.array(UNCL_BETAS)}
    for C in UNCL_CLASSES:
        for tag, scale in ((f"c{C}", 1.0), (f"c{C}_big", 10.0)):
            s = rng_t(rng, 2, C, *UNCL_SHAPE, scale=scale).clamp(-30, 30)
            t = rng_t(rng, 2, C, *UNCL_SHAPE, scale=scale).clamp(-30, 30)
            if scale > 1:                       # the extremes themselves, in both orders
                s[0, 0, 0, 0, :2] = torch.tensor([30.0, -30.0])
                t[0, 0, 0, 0, :2] = torch.tensor([-30.0, 30.0])
                s[0, -1, 0, 0, :2] = torch.tensor([-30.0, 30.0])
            out[f"{tag}.s"], out[f"{tag}.t"] = s, t
            for i, beta in enumerate(UNCL_BETAS):
                for dt, sfx in ((torch.float32, ""), (torch.float64, ".f64")):
                    x = s.to(dt).clone().requires_grad_(True)
                    loss = crit(x, t.to(dt), beta)
                    (g,) = torch.autograd.grad(loss, x)
                    out[f"{tag}.loss{i}{sfx}"] = loss
                    out[f"{tag}.grad{i}{sfx}"] = g
    save("uncl_nc", **out)


# ----------------------------------------------------------------------------- full nets
class VNetWithHead(nn.Module):
    """make_golden.VNetWithHead with a class count: reference VNet encoder / decoder + the projection layer list of
    UNet3D_contrastive.py:261-267 on x5."""

    def __init__(self, n_classes, scale_factor=2):
        super().__init__()
        self.vnet = ref_vnet.VNet(n_channels=1, n_classes=n_classes, normalization="groupnorm", has_dropout=False)
        self.projection = nn.Sequential(nn.Conv3d(256, 512, 1), nn.BatchNorm3d(512), nn.ReLU(inplace=True),
                                        nn.Conv3d(512, 256, 1), nn.BatchNorm3d(256))
        self.scale_factor = scale_factor

    def load_flat(self, p):
        self.vnet.load_state_dict({k: v for k, v in p.items() if not k.startswith("projection.")})
        self.projection.load_state_dict({k[len("projection."):]: v for k, v in p.items() if k.startswith("projection.")})

    def flat_named_parameters(self):
        for k, v in self.vnet.named_parameters():
            yield k, v
        for k, v in self.projection.named_parameters():
            yield "projection." + k, v

    def forward(self, x):
        feats = self.vnet.encoder(x)
        out = self.vnet.decoder(feats)
        c = F.interpolate(feats[4], scale_factor=self.scale_factor, mode="trilinear", align_corners=True)
        return torch.tanh(out), out, self.projection(c)


FULL_NETS = (("vnet", 3, 11), ("unet", 3, 12), ("vnet", 1, 11), ("vnet", 8, 11))      # net, classes, parameter seed (full_nets.npz's)


def logits_sub(t, C):
    return _sub(_sub(t)) if C == 8 else _sub(t)


def _full_nets(dtype):
    rng = np.random.default_rng(606)
    c = lambda t: t.to(dtype)  # noqa: E731
    x = c(rng_t(rng, 2, 1, 32, 32, 32))
    out = {"x_seed": np.array(606),
           "draw_order": np.array("default_rng(x_seed): x (2,1,32,32,32), then per net in `nets` order r1 (logits' shape), r2 (features' shape)"),
           "nets": np.array([f"{n}{C}" for n, C, _ in FULL_NETS])}
    for kind, C, seed in FULL_NETS:
        if kind == "vnet":
            p = {k: (c(v) if v.is_floating_point() else v) for k, v in onets.make_vnet_params(seed=seed, n_classes=C).items()}
            net = VNetWithHead(C).to(dtype)
            net.load_flat(p)
            named = list(net.flat_named_parameters())
            assert torch.equal(net.train().vnet(x), net(x)[1])
        else:
            p = {k: (c(v) if v.is_floating_point() else v) for k, v in onets.make_unet_params(seed=seed, n_classes=C).items()}
            net = ref_factory.net_factory_3d("unet_3D", 1, C, 2).to(dtype)
            net.load_state_dict(p)
            net.dropout1.p = 0.0
            net.dropout2.p = 0.0
            named = list(net.named_parameters())
        net.train()
        sdf, logits, feats = net(x)
        r1 = c(rng_t(rng, *logits.shape))
        r2 = c(rng_t(rng, *feats.shape))
        # (the U-Net's sdf head is discarded by the training step and left out of the objective: final.* get no gradient)
        grads = torch.autograd.grad((logits * r1).sum() + (feats * r2).sum(), [v for _, v in named], allow_unused=True)
        tag = f"{kind}{C}"
        out.update({f"{tag}.logits_sub": logits_sub(logits, C), f"{tag}.logits_stats": stats(logits), f"{tag}.sdf_stats": stats(sdf),
                    f"{tag}.feats_sub": _sub(feats), f"{tag}.feats_stats": stats(feats), f"{tag}.param_seed": np.array(seed),
                    f"{tag}.grad_stats": np.stack([stats(g) for g in grads]),
                    f"{tag}.param_names": np.array([k for k, _ in named]),
                    f"{tag}.param_shapes": np.array([";".join(str(d) for d in v.shape) for _, v in named])})
    return out


F64_KEYS_FULL = ("logits_sub", "logits_stats", "sdf_stats", "feats_sub", "feats_stats", "grad_stats")


def gen_full_nets():
    out = _full_nets(torch.float32)
    twin = _full_nets(torch.float64)
    for kind, C, _ in FULL_NETS:
        for k in F64_KEYS_FULL:
            out[f"{kind}{C}.{k}.f64"] = twin[f"{kind}{C}.{k}"]
    save("full_nets_nc", **out)


# ----------------------------------------------------------------------------- ISLES step traces, 3 classes
def blob_labels3(rng, B, D, H, W):
    """two ellipsoids per volume: class 1, then class 2 (drawn over it); every sample holds all three labels"""
    zz, yy, xx = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    lab = np.zeros((B, D, H, W), np.int64)
    for b in range(B):
        for cls, lo, hi in ((1, 0.3, 0.5), (2, 0.5, 0.7)):
            c = rng.uniform(lo, hi, 3) * (D, H, W)
            r = rng.uniform(0.15, 0.3, 3) * (D, H, W)
            lab[b][((zz - c[0]) / r[0]) ** 2 + ((yy - c[1]) / r[1]) ** 2 + ((xx - c[2]) / r[2]) ** 2 <= 1] = cls
        assert set(np.unique(lab[b])) == {0, 1, 2}
    return torch.from_numpy(lab)


NC, BASE_LR, MAX_ITERATIONS = 3, 0.01, 20000


def _isles_step_trace(kind, n_steps=2, dtype=torch.float32):
    """The imported reference modules / losses in the order of train_DyCON_ISLES22.py:236-324."""
    seed = 707 if kind == "unet_3D" else 708
    rng, rng_lab = np.random.default_rng(seed), np.random.default_rng(seed + 100)
    B, LB, S = 2, 1, 32
    cast = lambda d: {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in d.items()}  # noqa: E731
    if kind == "unet_3D":
        model = ref_factory.net_factory_3d("unet_3D", 1, NC, 2).to(dtype)
        ema = ref_factory.net_factory_3d("unet_3D", 1, NC, 2).to(dtype)
        model.load_state_dict(cast(onets.make_unet_params(seed=21, n_classes=NC)))
        ema.load_state_dict(cast(onets.make_unet_params(seed=22, n_classes=NC)))
        for m_ in (model, ema):
            m_.dropout1.p = 0.0
            m_.dropout2.p = 0.0
        s_named = lambda: list(model.named_parameters())   # noqa: E731
        t_named = lambda: list(ema.named_parameters())     # noqa: E731
    else:
        model, ema = VNetWithHead(NC).to(dtype), VNetWithHead(NC).to(dtype)
        model.load_flat(cast(onets.make_vnet_params(seed=21, n_classes=NC)))
        ema.load_flat(cast(onets.make_vnet_params(seed=22, n_classes=NC)))
        s_named = lambda: list(model.flat_named_parameters())   # noqa: E731
        t_named = lambda: list(ema.flat_named_parameters())     # noqa: E731
    for _, p_ in t_named():
        p_.detach_()
    model.train()
    ema.train()
    opt = torch.optim.SGD([p_ for _, p_ in s_named()], lr=BASE_LR, momentum=0.9, weight_decay=0.0001)
    ce_loss, dice_loss = nn.CrossEntropyLoss(), ref_losses.DiceLoss(NC)
    uncl = ref_dycon.UnCLoss()
    fecl = ref_dycon.FeCLoss(device="cpu", temperature=0.6, gamma=2.0, use_focal=True, rampup_epochs=1500)
    out = {"B": np.array(B), "LB": np.array(LB), "S": np.array(S), "classes": np.array(NC), "seeds": np.array([21, 22]),
           "rng_seed": np.array(seed), "base_lr": np.array(BASE_LR), "max_iterations": np.array(MAX_ITERATIONS)}
    iter_num = 0
    for step in range(n_steps):
        vol = rng_t(rng, B, 1, S, S, S).to(dtype)
        noise = torch.clamp(rng_t(rng, B, 1, S, S, S) * 0.1, -0.2, 0.2).to(dtype)
        lab = blob_labels3(rng_lab, B, S, S, S)
        epoch = step * 700          # exercise the threshold ramp
        beta = ref_dycon.adaptive_beta(epoch=epoch, total_epochs=3334, max_beta=5.0, min_beta=0.5)
        _, s_logits, s_feat = model(vol)
        with torch.no_grad():
            _, t_logits, t_feat = ema(vol + noise)
        s_prob, t_prob = F.softmax(s_logits, 1), F.softmax(t_logits, 1)
        cw = 0.1 * ref_ramps.sigmoid_rampup(iter_num // 150, 200.0)
        ce = ce_loss(s_logits[:LB], lab[:LB].long())
        dice = dice_loss(s_prob[:LB], lab[:LB].unsqueeze(1))
        Bf, Cf, Hf, Wf, Df = s_feat.shape
        s_emb = F.normalize(s_feat.reshape(Bf, Cf, -1).transpose(1, 2), dim=-1)
        t_emb = F.normalize(t_feat.reshape(Bf, Cf, -1).transpose(1, 2), dim=-1)
        k = (S // Hf, S // Wf, S // Df)
        mask = (F.avg_pool3d(lab.float(), kernel_size=k, stride=k) > 0.5).float().to(dtype).reshape(Bf, -1).unsqueeze(1)
        f_loss = fecl(feat=s_emb, mask=mask, teacher_feat=t_emb, gambling_uncertainty=None, epoch=epoch)
        u_loss = uncl(s_logits, t_logits, beta)
        cons = ref_losses.softmax_mse_loss(s_prob[LB:], t_prob[LB:]).mean()
        loss = 1.0 * (ce + dice) + cw * cons + 0.5 * (f_loss + u_loss)
        opt.zero_grad()
        loss.backward()
        gstats = np.stack([stats(p_.grad) for _, p_ in s_named()])
        gnorm = torch.nn.utils.clip_grad_norm_([p_ for _, p_ in s_named()], max_norm=1.0)
        opt.step()
        alpha = min(1 - 1 / (iter_num + 1), 0.99)
        for (_, ep), (_, sp) in zip(t_named(), s_named()):
            ep.data.mul_(alpha).add_(sp.data, alpha=1 - alpha)
        lr_ = BASE_LR * (1.0 - iter_num / MAX_ITERATIONS) ** 0.9
        for group in opt.param_groups:
            group["lr"] = lr_
        iter_num += 1
        out.update({f"s{step}.label": lab.to(torch.uint8), f"s{step}.epoch": np.array(epoch), f"s{step}.beta": np.array(beta),
                    f"s{step}.vol_stats": stats(vol), f"s{step}.noise_stats": stats(noise),
                    f"s{step}.scalars": np.array([loss.item(), ce.item(), dice.item(), cons.item(), f_loss.item(),
                                                  u_loss.item(), cw, float(gnorm)]),
                    f"s{step}.logits_sub": _sub(_sub(s_logits)), f"s{step}.logits_stats": stats(s_logits),
                    f"s{step}.t_logits_stats": stats(t_logits), f"s{step}.feat_stats": stats(s_feat), f"s{step}.mask": mask,
                    f"s{step}.grad_stats": gstats,
                    f"s{step}.student_stats": np.stack([stats(p_) for _, p_ in s_named()]),
                    f"s{step}.teacher_stats": np.stack([stats(p_) for _, p_ in t_named()])})
    out["param_names"] = np.array([k for k, _ in s_named()])
    return out


F64_KEYS_STEP = ("scalars", "logits_sub", "logits_stats", "t_logits_stats", "feat_stats", "grad_stats", "student_stats", "teacher_stats")


def gen_steps():
    merged = {}
    for tag, kind in (("unet", "unet_3D"), ("vnet", "vnet")):
        out = _isles_step_trace(kind)
        twin = _isles_step_trace(kind, dtype=torch.float64)
        for step in range(2):
            for k in F64_KEYS_STEP:
                out[f"s{step}.{k}.f64"] = twin[f"s{step}.{k}"]
        merged.update({f"{tag}.{k}": v for k, v in out.items()})
    save("step_isles_nc3", **merged)


if __name__ == "__main__":
    fns = {"uncl": gen_uncl, "full": gen_full_nets, "steps": gen_steps}
    for w in sys.argv[1:] or list(fns):
        print(w)
        fns[w]()
