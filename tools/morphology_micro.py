#!/usr/bin/env python3
"""Time of the device mask post-processing (utils/morphology.py, csrc/morphology.hip) next to the host path it replaces, in the same
process on the same box, for one smoothed-noise blob mask (tests/morphology_ref.smooth_mask, density 0.7) at 192 x 192 x 64 and one
at 112 x 112 x 80:

  (a) a sliding-window case through `surface_eval.test_all_case(..., device_surface=True, blend=Blend("constant"))` with
      postprocess=None against the PARENT commit (`--parent DIR`: a checkout of the parent with its library built).  Every run is a
      fresh process that imports ONE of the two trees, parent and this tree alternating; the figure of a run is the median of its
      regions, "range" the parent's own min .. max over its runs.  The call is the one both trees have: the keyword is not passed.
  (b) the stencil: GPU time per iteration of dycon_morph_stencil on the packed mask (HIP events around 200 calls of n iterations,
      divided by 200 n) at 6 and 26 neighbours, erosion and dilation, next to the time a device-to-device copy of the packed mask
      would take at the copy rate measured here on a 256 MiB buffer; and whole calls of 1, 3 and 7 iterations.
  (c) binary_erosion(3 iterations), binary_fill_holes, remove_small_components(30) and a 4-step chain on a uint8 device mask: GPU time
      by HIP events around the call, host time to issue it (wall clock, device idle before, nothing waited for), the mean time of
      each kernel of one call (the library's per-launch events, which cost the launches their overlap) with the share of the
      dycon_cc_roots kernels, and the host path: mask copied to the host, scipy.ndimage, result copied back, synchronised wall clock.
Before anything is timed every device result is compared with scipy's, bit for bit.

    python tools/morphology_micro.py --parent ../parent --out profiles/morphology_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import datetime
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(192, 192, 64), (112, 112, 80)]
SW_SHAPE, SW_PATCH, STRIDE_XY, STRIDE_Z, BATCH = (192, 192, 64), (96, 96, 64), 16, 4, 4


def worker(a):
    """(a) in the tree `a.root`, through nothing but what both trees have"""
    sys.path.insert(0, a.root)
    import torch
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    from dycon_paper_replication_amd.utils import surface_eval as SE
    from dycon_paper_replication_amd.utils.sliding_window import Blend
    assert os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(SE.__file__)))) == os.path.abspath(a.root)
    torch.manual_seed(0)
    net = net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).to("cuda:0")
    image = np.random.default_rng(0).standard_normal(SW_SHAPE).astype(np.float32)
    x, y, z = np.ogrid[:SW_SHAPE[0], :SW_SHAPE[1], :SW_SHAPE[2]]
    label = ((x - 96) ** 2 + (y - 96) ** 2 + (2 * (z - 32)) ** 2 <= 50 ** 2).astype(np.uint8)
    cases = [(image, label)] * a.cases

    def run():
        return SE.test_all_case(net, cases, 2, SW_PATCH, STRIDE_XY, STRIDE_Z, batch_size=BATCH, device_surface=True, blend=Blend("constant"))

    run()
    ms = []
    for _ in range(a.regions):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = run()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / a.cases)
    print("RESULT " + json.dumps({"ms": ms, "metrics": [float(v) for v in r]}), flush=True)


def _spread(v):
    return f"median {statistics.median(v):.3f} (min {min(v):.3f} .. max {max(v):.3f}; runs {', '.join(f'{x:.3f}' for x in v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libdycon_hip.so built")
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per tree for (a)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--cases", type=int, default=5, help="cases per region of (a)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    # ---- (a): fresh processes, before this process touches the GPU
    trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("branch", HERE)]
    runs, metrics = {name: [] for name, _ in trees}, {name: set() for name, _ in trees}
    for _ in range(a.runs):
        for name, root in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--regions", str(a.regions), "--cases", str(a.cases)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs[name].append(statistics.median(res["ms"]))
            metrics[name].add(tuple(res["metrics"]))
            print(f"  {name}: {runs[name][-1]:.3f} ms/case", flush=True)

    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import morphology_ref as MR
    from components_micro import kernel_breakdown, timed_events, timed_wall
    from lesions_micro import timed_issue
    from dycon_paper_replication_amd import _lib
    from dycon_paper_replication_amd.utils import morphology as M

    dev = "cuda:0"
    emit(f"# morphology_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}")
    emit(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; median (min)")
    emit(f"(a) test_all_case, postprocess=None: one bf16 V-Net, volume {SW_SHAPE}, windows {SW_PATCH}, stride {STRIDE_XY} / {STRIDE_Z}, "
         f"ms/case; {a.runs} fresh processes per tree, alternating; a run = the median of its {a.regions} regions of {a.cases} cases")
    for name, _ in trees:
        emit(f"    {name:6s}  {_spread(runs[name])}")
    if a.parent:
        med = statistics.median(runs["branch"])
        where = "inside" if min(runs["parent"]) <= med <= max(runs["parent"]) else "below" if med < min(runs["parent"]) else "ABOVE"
        emit(f"    branch / parent {med / statistics.median(runs['parent']):.3f}: {where} the parent's range; metrics equal: "
             f"{len(metrics['parent'] | metrics['branch']) == 1}")

    big = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(big)
    copy_ms = timed_events(lambda: dst.copy_(big), 3, 10)[1]
    rate = big.numel() / (copy_ms * 1e-3)                                               # bytes copied per second
    del big, dst
    emit(f"device copy rate (256 MiB, device to device, best of 10): {rate / 1e12:.2f} TB/s copied")

    for shape in SHAPES:
        X, Y, Z = shape
        mask = MR.smooth_mask(shape, 0.7, 0)
        t = torch.from_numpy(mask).to(dev)
        words = M._Mask((1,) + shape, source=t[None]).packed()
        out, scratch = torch.empty_like(words), torch.empty_like(words)
        nbytes = words.numel() * 8
        emit(f"--- {X} x {Y} x {Z}, density {mask.mean():.3f}; packed {nbytes} bytes, a copy of it at the rate above {1e6 * nbytes / rate:.3f} us")

        # ---- (b)
        def stencil(conn, op, n):
            return lambda: _lib.call("dycon_morph_stencil", words.data_ptr(), out.data_ptr(), scratch.data_ptr(), 1, X, Y, Z, conn, op, n,
                                     torch.cuda.current_stream().cuda_stream)

        def many(fn, k=200):
            def run():
                for _ in range(k):
                    fn()
            return run

        emit("(b) dycon_morph_stencil on the packed mask, GPU us per iteration (200 calls of n iterations between two events); a call of n <= 4 iterations is one launch, so at n = 1 the figure is the rate at which the host issues calls")
        for conn in (1, 3):
            for op, name in ((M.ERODE, "erosion"), (M.DILATE, "dilation")):
                row = []
                for n in (1, 3, 7):
                    med, best = timed_events(many(stencil(conn, op, n)), 2, 7)
                    row.append(f"n = {n}: {1e3 * med / (200 * n):.2f} ({1e3 * best / (200 * n):.2f})")
                    if n == 7:
                        frac = (1e6 * nbytes / rate) / (1e3 * med / (200 * n))
                emit(f"    connectivity {conn} {name:8s} " + "; ".join(row) + f"; the copy bound is {frac:.3f} of an iteration")

        # ---- (c)
        pp = M.PostProcess(M.Opening(1, 2), M.FillHoles(), M.MinSize(30), M.Largest())
        rows = [("binary_erosion(c=1, n=3)", lambda: M.binary_erosion(t, 1, 3), lambda m: MR.erosion(m, 1, 3)),
                ("binary_fill_holes()", lambda: M.binary_fill_holes(t), lambda m: MR.fill_holes(m, 1)),
                ("remove_small_components(30)", lambda: M.remove_small_components(t, 30), lambda m: MR.min_size(m, 30, 3)),
                ("PostProcess(Opening(1, 2), FillHoles(), MinSize(30), Largest())", lambda: pp(t),
                 lambda m: MR.chain(m, [("opening", (1, 2)), ("fill_holes", (1,)), ("min_size", (30, 3)), ("largest", (3,))]))]
        emit(f"(c) uint8 device mask in, uint8 device mask out; ms; device: {a.reps} after {a.warmup} warm-up; host path: {a.host_reps} repeats")
        for name, device, ref in rows:
            def host():
                return torch.from_numpy(ref(t.cpu().numpy())).to(dev)

            assert torch.equal(device(), host()), name
            gpu, issue, h = timed_events(device, a.warmup, a.reps), timed_issue(device, a.warmup, a.reps), timed_wall(host, 1, a.host_reps)
            kernels = kernel_breakdown(device)
            cc = sum(v for k, v in kernels.items() if k.startswith(("cc_tile", "cc_merge", "cc_flatten")))
            emit(f"    {name}")
            emit(f"        GPU time {gpu[0]:.3f} ({gpu[1]:.3f}); host time to issue {issue[0]:.3f} ({issue[1]:.3f}); host path (copy, scipy, "
                 f"copy back) {h[0]:.3f} ({h[1]:.3f}): {h[0] / gpu[0]:.0f}x the GPU time, {h[0] / issue[0]:.0f}x the time to issue")
            emit("        kernels, ms: " + ", ".join(f"{k.replace('_kernel', '')} {v:.4f}" for k, v in kernels.items()) +
                 f"; dycon_cc_roots' share of the kernel time {cc / max(sum(kernels.values()), 1e-9):.2f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
