#!/usr/bin/env python3
"""What the uncertainty maps cost, at the BraTS geometry: one bf16 V-Net, a 192 x 192 x 64 volume, windows 96 x 96 x 64, stride
16 / 4 (49 windows), chunks of 4.  Three configurations of `uncertainty.single_case_uncertainty_device`:

    gaussian            Blend("gaussian")
    gaussian, mirror    Blend("gaussian", mirror_axes=(0, 1, 2)): 8 forwards per window
    gaussian, mc 4      Blend("gaussian"), mc_passes=4: 4 dropout forwards per chunk

each against `eval_classes.single_case_classes_device` with the same blend on the PARENT commit (`--parent DIR`: a checkout of the
parent with its library built).  Every run is a fresh process that imports ONE of the two trees, parent and this tree alternating;
the figure of a run is the median of its regions, and "range" is the parent's own min .. max over its runs, the spread repeated
runs of the same code show here.  The baseline of "mc 4" is one deterministic forward per chunk, so its ratio includes the three
extra forwards.  In this tree the same processes also take, per configuration: the case with every forward replaced by a cached
logits tensor (upload, gathers, layout conversion, accumulates, finalize and the host's work between them: the share of the case
spent outside the model), and `uncertainty.calibration` on the case's maps (15 bins, entropy as the uncertainty).
Times are synchronised wall clock over --cases cases per region (a fifth of them for the mirrored configuration).

    python tools/uncertainty_micro.py --parent ../parent --out profiles/uncertainty_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE, PATCH, STRIDE_XY, STRIDE_Z, BATCH = (192, 192, 64), (96, 96, 64), 16, 4, 4
CONFIGS = [("gaussian", (), 1), ("gaussian, mirror (0, 1, 2)", (0, 1, 2), 1), ("gaussian, mc_passes=4", (), 4)]


def _region(fn, cases):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(cases):
        r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / cases, r


def worker(a):
    """one tree, every configuration, the variants of a configuration alternating region by region"""
    import torch
    sys.path.insert(0, a.root)
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.utils import eval_classes as EC
    from dycon_paper_replication_amd.utils.sliding_window import Blend
    assert os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(EC.__file__)))) == os.path.abspath(a.root)
    shape, patch = tuple(a.shape), tuple(a.patch)
    torch.manual_seed(0)
    net = net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).to("cuda:0")
    image = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
    label = (np.random.default_rng(1).random(shape) < 0.3).astype(np.uint8)
    args = (image, STRIDE_XY, STRIDE_Z, patch)
    out = {}
    for name, axes, passes in CONFIGS:
        blend = Blend("gaussian", mirror_axes=axes)
        variants = {"classes": lambda: EC.single_case_classes_device(net, *args, batch_size=BATCH, blend=blend)}
        if a.tree == "branch":
            from dycon_paper_replication_amd.utils import uncertainty as U

            class Cached(torch.nn.Module):
                """the net's logits of one chunk, computed once: the case without its forwards"""
                has_dropout = True

                def __init__(self):
                    super().__init__()
                    net.eval()
                    with torch.no_grad():
                        self.logits = net(torch.zeros((BATCH, 1) + patch, dtype=torch.float32, device="cuda:0"))[1]

                def forward(self, x):
                    return None, self.logits[:x.shape[0]], None

                def forward_mc(self, x, seed, offset):
                    return self.forward(x)

            cached = Cached()
            kw = dict(batch_size=BATCH, blend=blend, mc_passes=passes, seed=0)
            variants["uncertainty"] = lambda: U.single_case_uncertainty_device(net, *args, **kw)
            variants["uncertainty, cached logits"] = lambda: U.single_case_uncertainty_device(cached, *args, device="cuda:0", **kw)
            maps = variants["uncertainty"]()
            variants["calibration"] = lambda: U.calibration(maps.prob, label, bins=15, uncertainty=maps.entropy)
        cases = max(a.cases // 5, 1) if axes else a.cases
        ms, last = {k: [] for k in variants}, {}
        for fn in variants.values():
            fn()
            fn()
        for _ in range(a.regions):
            for k, fn in variants.items():
                t, last[k] = _region(fn, cases)
                ms[k].append(t)
        res = {k: statistics.median(v) for k, v in ms.items()}
        res["sha"] = hashlib.sha1(last["classes"][1].cpu().numpy().tobytes()).hexdigest()
        if a.tree == "branch":
            same = passes == 1 and bool(torch.equal(last["uncertainty"].prob, last["classes"][1]))
            res["prob equals the classes evaluator"] = same
            res["ece"] = last["calibration"]["ece"]
        out[name] = res
    print("RESULT " + json.dumps(out), flush=True)


def _spread(v):
    return f"median {statistics.median(v):8.3f} (min {min(v):.3f} .. max {max(v):.3f}; runs {', '.join(f'{x:.3f}' for x in v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libdycon_hip.so built")
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per tree")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--cases", type=int, default=10, help="cases per region")
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPE)
    ap.add_argument("--patch", type=int, nargs=3, default=PATCH)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="branch", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    shape, patch = tuple(a.shape), tuple(a.patch)
    if a.parent is None or a.runs < 3 or a.regions < 3 or shape != SHAPE or patch != PATCH:
        print("note: without --parent, with fewer than 3 runs or regions, or at another geometry, this is a rehearsal, not a measurement",
              flush=True)
    trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("branch", HERE)]
    runs = {name: [] for name, _ in trees}
    for _ in range(a.runs):
        for name, root in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--tree", name, "--regions", str(a.regions),
                   "--cases", str(a.cases), "--shape", *map(str, shape), "--patch", *map(str, patch)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
            runs[name].append(json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:]))
            print(f"  {name}: " + ", ".join(f"{k} {v['classes']:.2f}" for k, v in runs[name][-1].items()), flush=True)
    import torch
    lines = [f"# uncertainty_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one bf16 V-Net (2 classes), volume {shape}, windows {patch}, "
             f"stride {STRIDE_XY} / {STRIDE_Z}, chunks of {BATCH}",
             f"# ms/case, synchronised wall clock; {a.runs} fresh processes per tree, alternating; a run = the median of its {a.regions} "
             f"regions of {a.cases} cases ({max(a.cases // 5, 1)} for the mirrored configuration)"]
    for name, _, _ in CONFIGS:
        col = lambda tree, key: [r[name][key] for r in runs[tree]]   # noqa: E731
        lines.append(f"{name}")
        if a.parent:
            lines.append(f"    parent  single_case_classes_device       {_spread(col('parent', 'classes'))}")
        lines.append(f"    branch  single_case_classes_device       {_spread(col('branch', 'classes'))}")
        lines.append(f"    branch  single_case_uncertainty_device   {_spread(col('branch', 'uncertainty'))}")
        lines.append(f"    branch  the line above, cached logits    {_spread(col('branch', 'uncertainty, cached logits'))}")
        lines.append(f"    branch  calibration (15 bins, entropy)   {_spread(col('branch', 'calibration'))}")
        unc = statistics.median(col("branch", "uncertainty"))
        outside = statistics.median(col("branch", "uncertainty, cached logits")) / unc
        note = f"    outside the model: {outside:.3f} of the uncertainty case"
        if a.parent:
            base = col("parent", "classes")
            same = len({r[name]["sha"] for t, _ in trees for r in runs[t]}) == 1
            ratio = statistics.median(col("branch", "classes")) / statistics.median(base)
            note = (f"    uncertainty / parent's classes evaluator {unc / statistics.median(base):.3f} (parent's own range "
                    f"{min(base) / statistics.median(base):.3f} .. {max(base) / statistics.median(base):.3f}); classes evaluator branch / "
                    f"parent {ratio:.3f}, probability maps equal as bytes: {same}\n" + note)
        eq = all(r[name]["prob equals the classes evaluator"] for r in runs["branch"])
        lines.append(note + (f"; prob equals the classes evaluator's as bits: {eq}" if "mc_passes" not in name else ""))
    for l in lines:
        print(l, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
