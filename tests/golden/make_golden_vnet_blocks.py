#!/usr/bin/env python3
"""Golden fixtures of the V-Net's building blocks by IMPORTING the reference's networks/VNet.py on the CPU (it needs only torch).

Stores data only, in vnet_blocks.npz:
  public_names                    : the classes the reference module defines
  keys/<class>/<norm>/keys|shapes : its state_dict keys and shapes (shape rows: ndim, then the extents), four normalisations each
  <case>/keys|shapes              : the same for every case of tests/test_vnet_blocks_cpu.py CASES (inputs, parameters and the
                                    upstream gradient are rebuilt from the case's seed by case_tensors)
  <case>/<tensor>                 : the fp64 reference's tensor at sample_stride (stored as fp32), <tensor> = y | gx | g.<parameter>;
                                    batchnorm cases also buf.<buffer> after one training forward and y_eval (the .eval() forward
                                    that follows it)
  <case>/<tensor>/stat            : [scale, 2-norm] of the full fp64 tensor (scale: its max-abs; for the analytically zero bias
                                    gradient of a convolution in front of a normalisation, the weight gradient's max-abs),
                                    then the max-abs error against it, relative to that scale, of the reference run in fp32 and
                                    of the reference run with bf16 modules, parameters and inputs (the bf16 bound of the GPU test
                                    is twice the latter)
and prints the errors into profiles/vnet_blocks_bounds.txt.

    python tests/golden/make_golden_vnet_blocks.py
"""
import importlib.util
import inspect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("DYCON_REFERENCE", "/root/reference/code")
REF_FILE = os.path.join(REF, "networks", "VNet.py")


def _reference():
    spec = importlib.util.spec_from_file_location("reference_networks_VNet", REF_FILE)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _shape_rows(sd):
    rows = np.zeros((len(sd), 6), dtype=np.int64)
    for i, v in enumerate(sd.values()):
        rows[i, 0] = v.dim()
        rows[i, 1:1 + v.dim()] = list(v.shape)
    return rows


def _run(module, x, gy, dtype):
    m = module.to(dtype)
    xr = x.detach().clone().to(dtype).requires_grad_(True)
    y = m(xr)
    y.backward(gy.to(dtype))
    out = {"y": y.detach(), "gx": xr.grad}
    for k, p in m.named_parameters():
        out["g." + k] = p.grad
    return out


def main(out_dir=HERE, bounds_dir=os.path.join(ROOT, "profiles")):
    sys.path.insert(0, os.path.dirname(HERE))
    from test_vnet_blocks_cpu import CASES, KEY_ARGS, NORMS, case_tensors, sample_stride
    sys.path.pop(0)
    ref = _reference()
    torch.set_num_threads(8)
    out = {"public_names": np.array([n for n, c in inspect.getmembers(ref, inspect.isclass) if c.__module__ == ref.__name__])}
    for cls, args in KEY_ARGS.items():
        for norm in NORMS:
            sd = getattr(ref, cls)(*args, normalization=norm).state_dict()
            out[f"keys/{cls}/{norm}/keys"] = np.array(list(sd.keys()))
            out[f"keys/{cls}/{norm}/shapes"] = _shape_rows(sd)
    lines = ["# reference networks/VNet.py blocks on the CPU: max-abs error against the fp64 run, relative to the tensor's max-abs",
             "# case tensor fp32 bf16"]
    for i, (name, cls, args, dhw, norm) in enumerate(CASES):
        make = lambda: getattr(ref, cls)(*args, normalization=norm)      # noqa: E731
        sd0 = make().state_dict()
        keys, shapes = list(sd0.keys()), [tuple(v.shape) for v in sd0.values()]
        out[f"{name}/keys"] = np.array(keys)
        out[f"{name}/shapes"] = _shape_rows(sd0)
        sd, x, gy = case_tensors(i, keys, shapes)
        runs = {}
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32), ("bf16", torch.bfloat16)):
            m = make()
            m.load_state_dict(sd)
            m.train()
            runs[tag] = _run(m, x, gy, dtype)
            if norm == "batchnorm":
                for k, b in m.named_buffers():
                    runs[tag]["buf." + k] = b.detach().clone()
                m.eval()
                with torch.no_grad():
                    runs[tag]["y_eval"] = m(x.to(dtype))
        for k, t64 in runs["f64"].items():
            flat = t64.double().reshape(-1)
            s = sample_stride(flat.numel())
            out[f"{name}/{k}"] = flat[::s].float().numpy()
            amax = float(flat.abs().max())
            # The bias of a convolution that a normalisation follows has an analytically ZERO gradient (the mean is subtracted): what
            # any implementation returns is the round-off of sum_rows gz, whose size is eps x the scale of the sums the same rows
            # form for the weight gradient.  Such a tensor is measured relative to that weight gradient's max-abs.
            wk = k[:-len("bias")] + "weight"
            if k.startswith("g.") and k.endswith(".bias") and wk in runs["f64"]:
                wmax = float(runs["f64"][wk].abs().max())
                if amax < 1e-6 * wmax:
                    amax = wmax
            errs = []
            for tag in ("f32", "bf16"):
                if k in runs[tag] and amax > 0:
                    errs.append(float((runs[tag][k].double().reshape(-1) - flat).abs().max()) / amax)
                else:
                    errs.append(0.0)
            out[f"{name}/{k}/stat"] = np.array([amax, float(flat.norm())] + errs, dtype=np.float64)
            if k in runs["bf16"]:
                lines.append(f"{name} {k} {errs[0]:.3e} {errs[1]:.3e}")
    np.savez_compressed(os.path.join(out_dir, "vnet_blocks.npz"), **out)
    with open(os.path.join(bounds_dir, "vnet_blocks_bounds.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
