#!/usr/bin/env python3
"""Golden fixtures of the gambling-softmax uncertainty by IMPORTING the reference on CPU (make_golden.py's stub-package recipe).

Stores data only (gambling.npz), per case of tests/test_gambling_cpu.py GAMBLING_CASES (inputs rebuilt from gambling_case's seed), fp64:
  c{i}_p, c{i}_entropy   : the reference's gambling_softmax and the entropy of train_DyCON_Pancreas.py:243 (every 97th element)
  c{i}_u                 : u of train_DyCON_Pancreas.py:242-246 with scale 1/k (all of it)
  c{i}_f{focal}_t{teacher}_e{epoch}_{loss,gfeat,gfeat_norm,glogits,glogits_norm}
                         : the reference's FeCLoss(use_focal, rampup_epochs=1500) on the embedded features and the contrast mask, with
                           gambling_uncertainty = that u (not detached): the loss, d/d(raw student features) (every 7th element + the
                           norm) and d/d(logits) through the whole pipeline (every 97th element + the norm)
  overflow_u, overflow_loss : case 0 with test_gambling_cpu.overflow_logits (NaN where exp overflows)

    python tests/golden/make_golden_gambling.py
"""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/code"

m = types.ModuleType("utils")
m.__path__ = [f"{REF}/utils"]
sys.modules["utils"] = m
ref = importlib.import_module("utils.dycon_losses")

from test_gambling_cpu import FECL_COMBOS, GAMBLING_CASES, STRIDE_FEAT, STRIDE_LOGITS, gambling_case, overflow_logits  # noqa: E402

torch.set_num_threads(8)


def pancreas_u(stud_logits, k):
    """train_DyCON_Pancreas.py:242-246, the factor k in place of args.feature_scaler * 4"""
    B = stud_logits.shape[0]
    p_gs = ref.gambling_softmax(stud_logits)
    entropy = -torch.sum(p_gs * torch.log(p_gs + 1e-6), dim=1, keepdim=True)
    entropy = F.interpolate(entropy, scale_factor=1 / k, mode="trilinear", align_corners=False).squeeze(1)
    return entropy.view(B, -1), p_gs, -torch.sum(p_gs * torch.log(p_gs + 1e-6), dim=1, keepdim=True)


def embed(f):
    B, C = f.shape[:2]
    return F.normalize(f.reshape(B, C, -1).transpose(1, 2), dim=-1)


def mask_con(label, k):
    m = F.avg_pool3d(label.double().unsqueeze(1), kernel_size=k, stride=k)
    return (m > 0.5).double().reshape(label.shape[0], -1).unsqueeze(1)


out = {}
for i in range(len(GAMBLING_CASES)):
    logits, sf, tf, label, k = gambling_case(i)
    u, p, H = pancreas_u(logits, k)
    out[f"c{i}_p"] = p.flatten()[::STRIDE_LOGITS].numpy()
    out[f"c{i}_entropy"] = H.flatten()[::STRIDE_LOGITS].numpy()
    out[f"c{i}_u"] = u.numpy()
    for focal, teacher, epoch in FECL_COMBOS:
        lg = logits.clone().requires_grad_(True)
        f = sf.clone().requires_grad_(True)
        crit = ref.FeCLoss(device="cpu", temperature=0.6, gamma=2.0, use_focal=bool(focal), rampup_epochs=1500)
        uu, _, _ = pancreas_u(lg, k)
        loss = crit(feat=embed(f), mask=mask_con(label, k), teacher_feat=embed(tf) if teacher else None, gambling_uncertainty=uu,
                    epoch=epoch)
        loss.backward()
        key = f"c{i}_f{focal}_t{teacher}_e{epoch}"
        out[key + "_loss"] = np.array(loss.item())
        out[key + "_gfeat"] = f.grad.flatten()[::STRIDE_FEAT].numpy()
        out[key + "_gfeat_norm"] = np.array(f.grad.norm().item())
        out[key + "_glogits"] = lg.grad.flatten()[::STRIDE_LOGITS].numpy()
        out[key + "_glogits_norm"] = np.array(lg.grad.norm().item())
logits, sf, tf, label, k = gambling_case(0)
u, _, _ = pancreas_u(overflow_logits(), k)
out["overflow_u"] = u.numpy()
crit = ref.FeCLoss(device="cpu", temperature=0.6, gamma=2.0, use_focal=True, rampup_epochs=1500)
out["overflow_loss"] = np.array(crit(feat=embed(sf), mask=mask_con(label, k), teacher_feat=embed(tf), gambling_uncertainty=u, epoch=0).item())
np.savez_compressed(os.path.join(HERE, "gambling.npz"), **out)
print({k_: v.shape for k_, v in out.items() if not k_.endswith("norm")}, os.path.getsize(os.path.join(HERE, "gambling.npz")))
