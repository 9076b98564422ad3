#!/usr/bin/env python3
"""Time of the device signed-distance path (utils/util.py, csrc/sdf.hip) next to the scipy path of the reference's compute_sdf
(code/utils/util.py:205-236, restated in tests/sdf_ref.py), in the same process on the same box, for a training batch of B = 4 at
96^3 and at 112 x 112 x 80.

Device: compute_sdf_device on labels that live on the GPU, fp32 output.  "GPU ms" is HIP events around the call, "host ms" the
wall-clock the call keeps the Python thread (no synchronisation inside); warm-up, then the median of the timed repeats (min in
brackets).  scipy: wall-clock of the restatement on the same masks, median of --host-reps.  The masks are thresholded smoothed noise
(a few blobs with ragged borders), foreground about 15 %.  The two results are compared bit for bit before anything is timed.

    python tools/sdf_micro.py --out profiles/sdf_micro.txt --commit $(git rev-parse --short HEAD)
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import sdf_ref  # noqa: E402
from dycon_paper_replication_amd.utils import util  # noqa: E402


def timed_device(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    gpu, host = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t0 = time.perf_counter()
        fn()
        host.append(1e3 * (time.perf_counter() - t0))
        e1.record()
        e1.synchronize()
        gpu.append(e0.elapsed_time(e1))
    return (statistics.median(gpu), min(gpu)), (statistics.median(host), min(host))


def timed_wall(fn, reps):
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), min(ms)


def blobs(shape, seed):
    from scipy import ndimage
    x = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape).astype(np.float32), 4.0, mode="nearest")
    return (x >= np.quantile(x, 0.85)).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# sdf_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; device: median of {a.reps} after {a.warmup} warm-up (min in "
             f"brackets); scipy: wall-clock median of {a.host_reps}",
             f"{'configuration':<40}{'GPU ms':>18}{'host ms':>18}{'scipy ms':>22}{'scipy / GPU':>13}"]
    for shape in ((96, 96, 96), (112, 112, 80)):
        masks = np.stack([blobs(shape, 10 * i + shape[2]) for i in range(4)])
        labels = torch.from_numpy(masks).to(dev)
        out_shape = (4, 1) + shape
        got = util.compute_sdf_device(labels, out_shape, dtype=torch.float64).cpu().numpy()
        assert np.array_equal(got, sdf_ref.compute_sdf(masks, out_shape), equal_nan=True)
        g, h = timed_device(lambda: util.compute_sdf_device(labels, out_shape), a.warmup, a.reps)
        s = timed_wall(lambda: sdf_ref.compute_sdf(masks, out_shape), a.host_reps)
        name = f"compute_sdf (4, {shape[0]}, {shape[1]}, {shape[2]})"
        lines.append(f"{name:<40}{g[0]:>9.3f} ({g[1]:.3f}){h[0]:>9.3f} ({h[1]:.3f}){s[0]:>13.1f} ({s[1]:.1f}){s[0] / g[0]:>12.0f}x")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
