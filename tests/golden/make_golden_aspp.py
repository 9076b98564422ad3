#!/usr/bin/env python3
"""Golden fixtures of UNet3D(use_aspp=True) / ASPP3D by IMPORTING the reference on CPU (make_golden.py's stub-package recipe).

Stores data only:
  aspp_keys.json : the reference UNet3D(use_aspp=True) state-dict keys and shapes, in order
  aspp.npz       : per case (tests/test_aspp_cpu.py ASPP_CASES, inputs rebuilt from aspp_case's seed) and mode (train / eval),
                   the fp64 reference's output (every 199th element + the norm); in train mode also the input gradient (the same),
                   every parameter's gradient (BatchNorm: every 4th channel; convolutions: the [:4, :4] corner + the norm) and the
                   running statistics after the forward (every 4th channel).  Dropout has p = 0, so nothing depends on torch's RNG.

    python tests/golden/make_golden_aspp.py
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/code"

for pkg in ("networks", "utils"):
    m = types.ModuleType(pkg)
    m.__path__ = [f"{REF}/{pkg}"]
    sys.modules[pkg] = m
ref_assp = importlib.import_module("networks.assp")
ref_unet = importlib.import_module("networks.UNet3D_contrastive")

from test_aspp_cpu import ASPP_CASES, aspp_case  # noqa: E402

STRIDE = 199
torch.set_num_threads(8)


def main():
    net = ref_unet.UNet3D(in_channels=1, n_classes=2, scale_factor=2, use_aspp=True)
    keys = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "aspp_keys.json"), "w") as f:
        json.dump(keys, f)
    out = {}
    for seed, (name, B, dhw) in enumerate(ASPP_CASES):
        for mode in ("train", "eval"):
            params, bufs, x, gy = aspp_case(100 + seed, B, dhw, torch.float64)
            m = ref_assp.ASPP3D(256, 256, output_stride=16).double()
            m.dropout.p = 0.0
            sd = {k[len("aspp."):]: v for k, v in {**params, **bufs}.items()}
            m.load_state_dict(sd)
            m.train(mode == "train")
            xr = x.clone().requires_grad_(True)
            y = m(xr)
            y.backward(gy)
            pre = f"{name}_{mode}_"
            out[pre + "y"] = y.detach().reshape(-1)[::STRIDE].float().numpy()
            out[pre + "y_norm"] = np.float64(y.detach().norm())
            if mode == "eval":
                continue
            out[pre + "gx"] = xr.grad.reshape(-1)[::STRIDE].float().numpy()
            out[pre + "gx_norm"] = np.float64(xr.grad.norm())
            for k, p in m.named_parameters():
                g = p.grad
                if g is None:        # bn_after_pool with one sample: no gradient, as in the reference
                    continue
                if g.dim() == 5:
                    out[pre + "g." + k] = g[:4, :4].float().numpy()
                    out[pre + "gnorm." + k] = np.float64(g.norm())
                else:
                    out[pre + "g." + k] = g[::4].float().numpy()
            for k, b in m.named_buffers():
                if not k.endswith("num_batches_tracked"):
                    out[pre + "buf." + k] = b[::4].float().numpy()
    np.savez_compressed(os.path.join(HERE, "aspp.npz"), **out)


if __name__ == "__main__":
    main()
