#!/usr/bin/env python3
"""Time of the device surface-distance path (utils/surface.py, csrc/surface.hip) next to the host path it can replace, in the same
process on the same box:

  * metrics.compute_hd95_device against metrics.compute_hd95 at (4, 96, 96, 96), the training batch;
  * eval_classes.calculate_metric_perclass(device_surface=True) against its host form on one 240 x 240 x 155 case, 2 and 4 classes.

Device: HIP events around the call, warm-up, then the median of the timed repeats (min in brackets); the perclass rows are wall-clock
around the whole call, its host syncs and confusion counts included, since that is what an evaluation loop pays.  Host: wall-clock,
median of --host-reps.  The masks are thresholded smoothed noise (a few blobs with ragged borders), prediction and ground truth drawn
from correlated fields.

    python tools/surface_micro.py --out profiles/surface_micro.txt --commit $(git rev-parse --short HEAD)
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

from dycon_paper_replication_amd.utils import eval_classes, metrics, surface  # noqa: E402


def timed_events(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def timed_wall(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms)


def field(shape, seed, sigma):
    from scipy import ndimage
    return ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape).astype(np.float32), sigma, mode="nearest")


def label_maps(shape, classes, seed, sigma):
    """(pred, gt) label maps with `classes` classes: quantile bands of two correlated smoothed-noise fields, foreground about 15 %"""
    base, other = field(shape, seed, sigma), field(shape, seed + 1, sigma)
    out = []
    for f in (base, 0.8 * base + 0.2 * other):
        edges = np.quantile(f, np.linspace(0.85, 1.0, classes)[:-1])
        out.append(np.digitize(f, edges).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# surface_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device: median of {a.reps} after {a.warmup} warm-up (min in "
             f"brackets); host: wall-clock median of {a.host_reps}",
             f"{'configuration':<44}{'device ms':>20}{'host ms':>22}{'speed-up':>10}"]

    def row(name, d, h=None):
        host = f"{h[0]:>13.1f} ({h[1]:.1f}){h[0] / d[0]:>9.1f}x" if h else ""
        lines.append(f"{name:<44}{d[0]:>11.3f} ({d[1]:.3f}){host}")

    # the training batch: HD95 of 4 binary pairs at 96^3
    shape = (96, 96, 96)
    pairs = [label_maps(shape, 2, 10 * i, 4.0) for i in range(4)]
    pred, gt = np.stack([p for p, _ in pairs]), np.stack([g for _, g in pairs])
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    max_dist = float(np.linalg.norm(shape))
    got, ref = metrics.compute_hd95_device(tp, tg, max_dist).cpu().numpy(), metrics.compute_hd95(pred, gt, max_dist)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
    row("compute_hd95 (4, 96, 96, 96)", timed_events(lambda: metrics.compute_hd95_device(tp, tg, max_dist), a.warmup, a.reps),
        timed_wall(lambda: metrics.compute_hd95(tp, tg, max_dist), 0, a.host_reps))
    row("  histograms only (surface_hists)", timed_events(lambda: surface.surface_hists(tp, tg), a.warmup, a.reps))

    # one evaluated case at the BraTS volume size
    shape = (240, 240, 155)
    for classes in (2, 4):
        pred, gt = label_maps(shape, classes, 100 + classes, 8.0)
        tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
        got = eval_classes.calculate_metric_perclass(tp, tg, classes, device_surface=True)
        ref = eval_classes.calculate_metric_perclass(tp, tg, classes)
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=0)
        row(f"calculate_metric_perclass 240x240x155, C = {classes}",
            timed_wall(lambda: eval_classes.calculate_metric_perclass(tp, tg, classes, device_surface=True), a.warmup, a.reps),
            timed_wall(lambda: eval_classes.calculate_metric_perclass(tp, tg, classes), 0, a.host_reps))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
