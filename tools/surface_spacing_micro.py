#!/usr/bin/env python3
"""Time of the weighted surface-distance path (utils/surface.py, csrc/surface_spacing.hip) next to the unit histogram path and the host
scipy path, in the same process on the same box, at the configurations of tools/surface_micro.py:

  * metrics.compute_hd95_device against metrics.compute_hd95-with-a-spacing at (4, 96, 96, 96), the training batch;
  * eval_classes.calculate_metric_perclass(device_surface=True) against its host form on one 240 x 240 x 155 case, 2 and 4 classes.

Per configuration four rows: the weighted path at (0.7, 0.7, 5.0), the weighted path at (1, 1, 1), the unit histogram path
(voxelspacing=None: the kernels of csrc/surface.hip, comparable with profiles/surface_micro.txt) and the host path at
(0.7, 0.7, 5.0), which is what the speed-up is stated against.  The three device variants alternate inside one loop, one call each
per repeat, so drift on a shared box hits them alike.  Device, batch rows: HIP events around the call; perclass rows: wall-clock
around the whole call, its host syncs and confusion counts included.  Median of the repeats, min in brackets.  Below the table: the
mean time per call of every kernel of the weighted path (the library's per-launch events), grouped into transform, sums and select.

    python tools/surface_spacing_micro.py --out profiles/surface_spacing_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dycon_paper_replication_amd import _lib  # noqa: E402
from dycon_paper_replication_amd.utils import eval_classes, metrics  # noqa: E402
from dycon_paper_replication_amd.utils.test_3d_patch import _surface_distances  # noqa: E402
from surface_micro import label_maps  # noqa: E402

ANISO = (0.7, 0.7, 5.0)
GROUPS = (("transform", ("spaced_border_z_kernel", "spaced_axis_pass_kernel")), ("sums", ("spaced_sums_kernel", "spaced_begin_kernel")),
          ("select", ("spaced_digit_kernel", "spaced_pick_kernel")))


def one_events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def one_wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def alternate(fns, one, warmup, reps):
    """[(median, min)] of each fn, one call of each per repeat in turn"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            ms[i].append(one(fn))
    return [(statistics.median(m), min(m)) for m in ms]


def kernel_breakdown(fn, reps=5):
    """mean ms per call of every kernel `fn` launches (the library's per-launch HIP events: dycon_kernel_timing)"""
    import ctypes as C
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    _lib.call("dycon_kernel_timing", 1)
    try:
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        n = lib.dycon_kernel_timing_count()
        ms, st, nm = (C.c_float * n)(), (C.c_ulonglong * n)(), (C.c_int * n)()
        if lib.dycon_kernel_timing_fetch(0, n, ms, st, nm):
            raise _lib.DyconLibraryError(lib.dycon_last_error().decode())
    finally:
        _lib.call("dycon_kernel_timing", 0)
    out = {}
    for i in range(n):
        name = lib.dycon_kernel_timing_name(nm[i]).decode().split("(")[0].split("<")[0].split()[-1]
        out[name] = out.get(name, 0.0) + ms[i] / reps
    return out


def host_hd95(pred, gt, max_dist, spacing):
    """metrics.compute_hd95 with a spacing: the host path a user who reports millimetres runs today"""
    out = []
    for p, t in zip(pred, gt):
        if p.sum() == 0 or t.sum() == 0:
            out.append(max_dist)
        else:
            out.append(float(np.percentile(np.hstack((_surface_distances(p != 0, t != 0, spacing),
                                                      _surface_distances(t != 0, p != 0, spacing))), 95)))
    return out


def timed_host(fn, reps):
    ms, val = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        val = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return (statistics.median(ms), min(ms)), val


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# surface_spacing_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device: median of {a.reps} alternating repeats after "
             f"{a.warmup} warm-up (min in brackets); host: wall-clock median of {a.host_reps}; speed-up against the host row",
             f"{'configuration':<58}{'ms':>20}{'speed-up':>10}"]
    breakdowns = []

    def block(name, dev_rows, host):
        lines.append(name)
        for label, d in dev_rows:
            lines.append(f"{'  ' + label:<58}{d[0]:>11.3f} ({d[1]:.3f}){host[0] / d[0]:>9.1f}x")
        lines.append(f"{'  host scipy, spacing (0.7, 0.7, 5.0)':<58}{host[0]:>11.1f} ({host[1]:.1f})")

    labels = ("weighted path, spacing (0.7, 0.7, 5.0)", "weighted path, spacing (1, 1, 1)", "unit histogram path (voxelspacing=None)")
    spacings = (ANISO, (1.0, 1.0, 1.0), None)

    # the training batch: HD95 of 4 binary pairs at 96^3
    shape = (96, 96, 96)
    pairs = [label_maps(shape, 2, 10 * i, 4.0) for i in range(4)]
    pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    max_dist = float(np.linalg.norm(shape))
    fns = [lambda s=s: metrics.compute_hd95_device(tp, tg, max_dist, voxelspacing=s) for s in spacings]
    host, ref = timed_host(lambda: host_hd95(pred, gt, max_dist, ANISO), a.host_reps)
    np.testing.assert_allclose(fns[0]().cpu().numpy(), ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(fns[1]().cpu().numpy(), fns[2]().cpu().numpy(), rtol=1e-12, atol=0)
    block("compute_hd95 (4, 96, 96, 96)", list(zip(labels, alternate(fns, one_events, a.warmup, a.reps))), host)
    breakdowns.append(("(4, 96, 96, 96), spacing (0.7, 0.7, 5.0)", kernel_breakdown(fns[0])))
    breakdowns.append(("(4, 96, 96, 96), spacing (1, 1, 1)", kernel_breakdown(fns[1])))

    # one evaluated case at the BraTS volume size
    shape = (240, 240, 155)
    for classes in (2, 4):
        pred, gt = label_maps(shape, classes, 100 + classes, 8.0)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        fns = [lambda s=s: eval_classes.calculate_metric_perclass(tp, tg, classes, device_surface=True, voxelspacing=s) for s in spacings]
        host, ref = timed_host(lambda: eval_classes.calculate_metric_perclass(tp, tg, classes, voxelspacing=ANISO), a.host_reps)
        np.testing.assert_allclose(fns[0](), ref, rtol=1e-12, atol=0)
        np.testing.assert_allclose(fns[1](), fns[2](), rtol=1e-12, atol=0)
        block(f"calculate_metric_perclass 240x240x155, C = {classes}", list(zip(labels, alternate(fns, one_wall, a.warmup, a.reps))), host)
        breakdowns.append((f"240x240x155, C = {classes}, spacing (0.7, 0.7, 5.0)", kernel_breakdown(fns[0])))
        breakdowns.append((f"240x240x155, C = {classes}, spacing (1, 1, 1)", kernel_breakdown(fns[1])))

    lines.append("")
    lines.append("# kernels of the weighted path, mean ms per call over 5 calls (per-launch events, each launch timed alone)")
    lines.append(f"{'configuration':<48}" + "".join(f"{g:>12}" for g, _ in GROUPS) + f"{'  of which y/x passes':>22}")
    for name, k in breakdowns:
        cells = "".join(f"{sum(k.get(n, 0.0) for n in names):>12.3f}" for _, names in GROUPS)
        lines.append(f"{name:<48}{cells}{k.get('spaced_axis_pass_kernel', 0.0):>22.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
