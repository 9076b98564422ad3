#!/usr/bin/env python3
"""Golden fixtures of the reference's remaining loss callables by IMPORTING the reference's utils/losses.py on the CPU
(make_golden.py's stub-package recipe).  Stores data only.

losses_extra.npz, per case i of tests/test_losses_extra_cpu.py EXTRA_CASES (inputs rebuilt from losses_case's seed) and per entry
`name` of its call table (dice1, dice1_soft, softmax_dice, entropy_min, entropy_map, entropy_loss, entropy_loss_map, sym_mse,
compute_kl, focal{k}):
  c{i}_{name}_v32 / _v64            : the reference's value on the fp32 inputs / on the same inputs .double() (the fp64 twin)
  c{i}_{name}_g{k}_32 / _64         : the gradient of the k-th differentiable input, every stride_of(i)-th element in natural order
  c{i}_{name}_g{k}n_32 / _64        : its 2-norm
  c{i}_entropy_map_out32 / 64, c{i}_entropy_loss_map_out32 / 64 : the maps themselves (same sampling)
  c{i}_a                            : the sampled input logits (guards the seed)
  fecl_v32 / _v64 / _g32 / _g64     : the LEGACY losses.FeCLoss(device, 0.6)(feat, mask) on fecl_case(), gradient in full

The reference's entropy_loss and entropy_loss_map build their divisor with .cuda() and cannot run here: they are NOT called.  Their
entries are entropy_minmization(p) / np.log(C) and entropy_map(p) / np.log(C), so the parity of those two names is derived, not direct.

losses_api.json: the public functions and classes the reference module defines, with parameter names and defaults (inspect).

    python tests/golden/make_golden_losses_extra.py /path/to/reference/code
"""
import importlib
import inspect
import json
import os
import sys
import types
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ["DYCON_REFERENCE"]

m = types.ModuleType("utils")
m.__path__ = [f"{REF}/utils"]
sys.modules["utils"] = m
ref = importlib.import_module("utils.losses")

from test_losses_extra_cpu import EXTRA_CASES, calls, fecl_case, losses_case, run_call, stride_of  # noqa: E402

torch.set_num_threads(8)

# the reference module with the two .cuda() callables replaced by their derived form
shim = types.SimpleNamespace(**{k: getattr(ref, k) for k in dir(ref) if not k.startswith("_")})
shim.entropy_loss = lambda p, C=2: ref.entropy_minmization(p) / np.log(C)
shim.entropy_loss_map = lambda p, C=2: ref.entropy_map(p) / np.log(C)

out = {}
for i in range(len(EXTRA_CASES)):
    t = losses_case(i)
    st = stride_of(i)
    out[f"c{i}_a"] = t["a"].flatten()[::st].numpy()
    for name, (fn, wrt) in calls(t["C"]).items():
        for tag, dtype in (("32", None), ("64", torch.float64)):
            v, gr = run_call(shim, fn, wrt, t, dtype)
            out[f"c{i}_{name}_v{tag}"] = np.array(v.item(), dtype=np.float32 if tag == "32" else np.float64)
            for k, gk in enumerate(gr):
                out[f"c{i}_{name}_g{k}_{tag}"] = gk.flatten()[::st].numpy()
                out[f"c{i}_{name}_g{k}n_{tag}"] = np.array(gk.norm().item())
    for tag, p in (("32", t["p"]), ("64", t["p"].double())):
        out[f"c{i}_entropy_map_out{tag}"] = shim.entropy_map(p).flatten()[::st].numpy()
        out[f"c{i}_entropy_loss_map_out{tag}"] = shim.entropy_loss_map(p, C=t["C"]).flatten()[::st].numpy()
feat, mask = fecl_case()
for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
    f = feat.to(dtype).requires_grad_(True)
    v = ref.FeCLoss(device="cpu", temperature=0.6)(f, mask.to(dtype))
    out[f"fecl_v{tag}"] = np.array(v.item())
    out[f"fecl_g{tag}"] = torch.autograd.grad(v, f)[0].numpy()
# np.savez_compressed stamps every member with the current time; a fixed stamp makes a rerun reproduce the file bit for bit
with zipfile.ZipFile(os.path.join(HERE, "losses_extra.npz"), "w", zipfile.ZIP_DEFLATED) as zf:
    for key, arr in out.items():
        info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        with zf.open(info, "w") as fh:
            np.lib.format.write_array(fh, np.asanyarray(arr), allow_pickle=False)

api = {}
for name, obj in sorted(vars(ref).items()):
    if name.startswith("_") or getattr(obj, "__module__", None) != ref.__name__:
        continue

    def params(fn):
        return [[p.name, None if p.default is inspect.Parameter.empty else repr(p.default)]
                for p in inspect.signature(fn).parameters.values() if p.name != "self"]
    if inspect.isclass(obj):
        api[name] = {"kind": "class", "signatures": {"__init__": params(obj.__init__), "forward": params(obj.forward)}}
    elif inspect.isfunction(obj):
        api[name] = {"kind": "function", "signatures": {"call": params(obj)}}
with open(os.path.join(HERE, "losses_api.json"), "w") as fh:
    json.dump(api, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(len(out), "arrays,", os.path.getsize(os.path.join(HERE, "losses_extra.npz")), "bytes;", sorted(api))
