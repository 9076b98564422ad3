#!/usr/bin/env python3
"""Fixtures of the `_plus` evaluator family, the LA data path and the LA draw order (tests/test_ensemble_cpu.py, test_la_heart_cpu.py).

The reference's code/utils/test_3d_patch.py and code/dataloaders/la_heart.py cannot be imported here (cv2, h5py, natsort, nibabel,
medpy, skimage), so they are READ with `ast`, not imported.  Stores data only:

  test_3d_patch_api.json
    "test_3d_patch": {name: {"params": [...], "defaults": {param: value}}} of the six names utils/ensemble_eval.py binds
    "la_heart":      the same for every public top-level function and class (a class: the parameters of its __init__ without self;
                     "params": null when it defines none)
  ensemble.npz
    normalize.<i>.in / .out    inputs (seeded) and the outputs of the reference's normalize_image (:14-17), whose definition is
                               compiled from the parsed source on its own (it needs numpy only)
    plan.*                     draw_plan(PLAN_SHAPES, PLAN_INDICES, PLAN_PATCH) in its default order after np.random.seed(PLAN_SEED):
                               the records the crop-first order drew before the `order` keyword existed

    python tests/golden/make_golden_ensemble.py
"""
import ast
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/code"

T3_NAMES = ("test_single_case_plus", "test_all_case_plus", "var_all_case_LA", "var_all_case_LA_plus", "calculate_metric_percase1",
            "normalize_image")
PLAN_SHAPES, PLAN_INDICES, PLAN_PATCH, PLAN_SEED = [(13, 11, 9), (20, 17, 16), (6, 11, 9), (8, 12, 10)], [0, 1, 2, 3, 1, 0, 2], (8, 8, 6), 2024


def signature(fn, drop_self=False):
    a = fn.args
    assert not a.posonlyargs and not a.kwonlyargs and a.vararg is None and a.kwarg is None
    params = [p.arg for p in a.args]
    defaults = {p: ast.literal_eval(d) for p, d in zip(params[len(params) - len(a.defaults):], a.defaults)}
    if drop_self:
        assert params[0] == "self"
        params = params[1:]
    return {"params": params, "defaults": defaults}


def parse(rel):
    with open(os.path.join(REF, rel)) as f:
        return ast.parse(f.read())


def main():
    t3 = parse("utils/test_3d_patch.py")
    fns = {n.name: n for n in t3.body if isinstance(n, ast.FunctionDef)}
    api = {"test_3d_patch": {name: signature(fns[name]) for name in T3_NAMES}, "la_heart": {}}
    for node in parse("dataloaders/la_heart.py").body:
        if isinstance(node, ast.FunctionDef) and not node.name.startswith("_"):
            api["la_heart"][node.name] = dict(signature(node), kind="function")
        elif isinstance(node, ast.ClassDef) and not node.name.startswith("_"):
            init = [n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "__init__"]
            sig = signature(init[0], drop_self=True) if init else {"params": None, "defaults": {}}
            api["la_heart"][node.name] = dict(sig, kind="class")
    with open(os.path.join(HERE, "test_3d_patch_api.json"), "w") as f:
        json.dump(api, f, indent=1, sort_keys=True)
        f.write("\n")

    ns = {"np": np}
    exec(compile(ast.Module(body=[fns["normalize_image"]], type_ignores=[]), "normalize_image", "exec"), ns)
    out = {}
    rng = np.random.default_rng(7)
    inputs = [rng.standard_normal((5, 4, 3)), (rng.random((6, 7)) * 300 - 100).astype(np.float32), rng.integers(-5, 90, (4, 4, 4)),
              rng.integers(0, 256, (3, 9)).astype(np.uint8)]
    for i, x in enumerate(inputs):
        out[f"normalize.{i}.in"], out[f"normalize.{i}.out"] = x, ns["normalize_image"](x)

    from dycon_paper_replication_amd.dataloaders import draw_plan
    np.random.seed(PLAN_SEED)
    plan = draw_plan(PLAN_SHAPES, PLAN_INDICES, PLAN_PATCH)
    out["plan.shapes"], out["plan.indices"] = np.asarray(PLAN_SHAPES), np.asarray(PLAN_INDICES)
    out["plan.patch_size"], out["plan.seed"] = np.asarray(PLAN_PATCH), np.asarray(PLAN_SEED)
    for field in ("case", "origin", "k", "flip_axis", "patch"):
        out[f"plan.{field}"] = np.ascontiguousarray(plan[field])
    out["plan.next_draw"] = np.asarray(np.random.randint(0, 1 << 30))      # the generator's position after the plan
    path = os.path.join(HERE, "ensemble.npz")
    np.savez_compressed(path, **out)
    print(sorted(api["test_3d_patch"]), sorted(api["la_heart"]), {k: v.shape for k, v in out.items()}, os.path.getsize(path))


if __name__ == "__main__":
    main()
