#!/usr/bin/env python3
"""Preprocessing on the device (preprocessing.py, csrc/resample.hip) next to numpy / scipy on the same box, at the two geometries the
reference's scripts meet: BraTS 240 x 240 x 155 -> 192 x 192 x 64 and ISLES 112 x 112 x 73 -> 112 x 112 x 64, one case at a time.

  per launch group   (s) dycon_volume_stats, (z1) dycon_zoom order 1 with the normalisation applied on load, (z0) dycon_zoom order 0
                     that binarises on load, (c) a device-to-device copy of the image (torch's copy kernel: 16-byte loads and stores),
                     the yardstick.  (s), (z1), (z0) and (c) alternate.  host ms: wall clock of the enqueue loop, no synchronisation
                     inside a region.  GPU ms: HIP events around groups of calls enqueued behind a blocker kernel (back-to-back).
                     "share of the copy rate": (algorithmic bytes / GPU time) / (copy bytes / copy time); algorithmic bytes are
                     the input read once per pass that has to read it (twice for the statistics) plus the output written once.
  per case           (p) preprocess_*_volume from device-resident inputs, synchronised wall clock, next to (n) the reference's
                     arithmetic in numpy / scipy on this box's CPU (normalize_image's expressions, zoom order 1, zoom order 0).
The figure is the median over --regions regions (min .. max: the spread on this box).

    python tools/preprocess_micro.py --out profiles/preprocess_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import resample_ref as R  # noqa: E402
from datapath_micro import fmt, gpu_region, host_region  # noqa: E402
from dycon_paper_replication_amd import preprocessing as P  # noqa: E402

GEOMETRIES = (("BraTS", (240, 240, 155), (192, 192, 64), 0.0), ("ISLES", (112, 112, 73), (112, 112, 64), 0.5))


def synthetic_case(shape, seed):
    """a positive head in a zero background with integer intensities, and a blob of labels 1, 2, 4"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*(np.linspace(-1, 1, n, dtype=np.float32) for n in shape), indexing="ij"))
    image = np.where((g ** 2).sum(0) < 0.8, np.round(400 + 150 * rng.standard_normal(shape, dtype=np.float32)).clip(1, None), 0)
    seg = np.where(((g - 0.2) ** 2).sum(0) < 0.15, rng.choice(np.array([1, 2, 4], np.float32), size=shape), 0)
    return image.astype(np.float32), seg.astype(np.float32)


def host_case(image, seg, target, thr):
    x = R.normalize_image(image)
    f = [t / s for t, s in zip(target, image.shape)]
    return ndimage.zoom(x, f, order=1), ndimage.zoom((seg > thr).astype(np.uint8), f, order=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per region of the per-launch comparison")
    ap.add_argument("--cases", type=int, default=20, help="cases per region of the per-case comparison")
    ap.add_argument("--host-cases", type=int, default=3, help="numpy / scipy cases per region")
    a = ap.parse_args()
    if a.regions < 3 or a.calls < 100:
        print("note: fewer than 3 regions of 100 calls is a rehearsal, not a measurement", flush=True)
    dev = "cuda:0"
    lines = [f"# preprocess_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}, numpy {np.__version__}; one case per call; alternating, "
             f"median of {a.regions} regions (min .. max); {a.calls} calls per region per launch group, {a.cases} cases per region",
             "# the zoom kernels are as first written, nothing in them was tuned; the statistics launches were changed once after their "
             "first measurement (DESIGN.md section 7: one conditional set of atomics per workgroup, partials folded in parallel)"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    for name, shape, target, thr in GEOMETRIES:
        image, seg = synthetic_case(shape, 7)
        want_i, want_l = host_case(image, seg, target, thr)
        img, lab = torch.from_numpy(image).to(dev), torch.from_numpy(seg).to(dev)
        got_i, got_l = P._preprocess(img, lab, target, thr, name)
        err = float(np.abs(got_i.cpu().numpy() - want_i).max())
        assert np.array_equal(got_l.cpu().numpy(), want_l) and err < 1e-6, err           # equal before anything is timed
        V, Vo = int(np.prod(shape)), int(np.prod(target))
        vol = img.reshape((1,) + shape)
        labv = lab.reshape((1,) + shape)
        st = P._stats(vol, want_stats=False)
        dst = torch.empty_like(vol)
        groups = {"s": (lambda _: P._stats(vol, want_stats=False), 2 * 4 * V),
                  "z1": (lambda _: P._zoom(vol, target, 1, st.record, torch.float32, None), 4 * V + 4 * Vo),
                  "z0": (lambda _: P._zoom(labv, target, 0, None, torch.uint8, thr), 4 * V + Vo),
                  "c": (lambda _: dst.copy_(vol), 2 * 4 * V)}
        for fn, _ in groups.values():
            fn(0)
        host, gpu, retaken, blocker = {k: [] for k in groups}, {k: [] for k in groups}, [0], [2_000_000]
        for _ in range(a.regions):
            for k, (fn, _) in groups.items():
                host[k].append(host_region(fn, [0], a.calls))
        for _ in range(a.regions):
            for k, (fn, _) in groups.items():
                gpu[k].append(gpu_region(fn, [0], a.calls, blocker, retaken))
        copy_rate = groups["c"][1] / statistics.median(gpu["c"])
        emit(f"{name}: {shape} -> {target}, {4 * V / 1e6:.1f} MB image; label equal to scipy's, image within {err:.1e} of numpy / scipy")
        for k, label in (("s", "dycon_volume_stats (memset + 3 launches)     "), ("z1", "dycon_zoom order 1, normalise on load         "),
                         ("z0", "dycon_zoom order 0, binarise on load          "), ("c", "device-to-device copy of the image            ")):
            rate = groups[k][1] / statistics.median(gpu[k])
            emit(f"  ({k:>2}) {label} host ms {fmt(host[k])}   GPU ms {fmt(gpu[k])}   {groups[k][1] / 1e6:6.1f} MB, "
                 f"{rate / 1e9:5.2f} TB/s, {100 * rate / copy_rate:5.1f}% of the copy rate")
        emit(f"       blocker groups re-taken: {retaken[0]}")

        def device_case():
            return P._preprocess(img, lab, target, thr, name)

        def region(fn, n):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / n

        device_case()
        res = {"p": [], "n": []}
        for _ in range(a.regions):
            res["p"].append(region(device_case, a.cases))
            res["n"].append(region(lambda: host_case(image, seg, target, thr), a.host_cases))
        emit(f"  ( p) preprocess_*_volume, inputs on the device      ms/case {fmt(res['p'])}")
        emit(f"  ( n) numpy normalise + scipy zoom order 1 + order 0 ms/case {fmt(res['n'])}   (n) / (p) "
             f"{statistics.median(res['n']) / statistics.median(res['p']):.0f}x")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
