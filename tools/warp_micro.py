#!/usr/bin/env python3
"""The interpolating augmentations of the device batch loader (dataloaders/device_warp.py, utils/filters.py; csrc/warp.hip,
csrc/filters.hip) next to the plain assembly they extend ON THE SAME CROPS, next to the scipy / numpy chain they restate on the same
box, each Gaussian pass next to a device-to-device copy of the same bytes, a trainer fed by the augmenting loader next to a trainer
fed one resident batch, and the default loader next to the parent commit's.

  (p) assemble_batch                          the plain kernel on the same crops: the yardstick
  (0) assemble_batch_warp, warp = 0           the same crops through the new entry point
  (a) assemble_batch_warp, affine             scale 0.8..1.25, rotations up to 15 degrees about the three axes, order 1 / order 0
  (e) assemble_batch_warp, affine + elastic   the same with a displacement field (made beforehand: (f) is its own row)
  (f) elastic_field                           Philox noise + three Gaussian passes (sigma 9..13, mode constant) x alpha, B x 3 volumes
  (b) blur                                    gaussian_filter in place, sigma 0.5..1.0, every sample of the batch
  (i) intensity                               gain, bias and gamma on every sample of the batch
  host chain                                  scipy.ndimage.affine_transform / map_coordinates (order 1 image, order 0 label),
                                              gaussian_filter, numpy gain / bias / gamma on host arrays, wall clock

Data, sizes and the timing method are those of tools/datapath_micro.py (whose helpers are imported): synthetic BraTS-like cases,
B = 4 at 96^3, labels int64; the plans are drawn once (64, seeded) and every variant assembles the same ones.  The variants
ALTERNATE region by region; median over --regions regions of --batches batches (min .. max).  host ms: the enqueue loop alone;
GPU ms: HIP events around groups enqueued behind a blocker kernel (back-to-back execution).  Before anything is timed (a) and (e)
are compared bit for bit with scipy on one batch, and (0) with (p).

--parent-device-cache FILE: dataloaders/device_cache.py of the parent commit (``git show HEAD~1:...``), loaded next to this
commit's; the two default loaders (warp=None, intensity=None) then alternate in this process.

    python tools/warp_micro.py --out profiles/warp_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import datetime
import importlib.util
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from datapath_micro import GROUP, fmt, gpu_region, host_region, make_cases  # noqa: E402
from dycon_paper_replication_amd.dataloaders import (PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, assemble_batch)  # noqa: E402
from dycon_paper_replication_amd.dataloaders import device_warp as W  # noqa: E402
from dycon_paper_replication_amd.dataloaders.brats19 import TwoStreamBatchSampler  # noqa: E402
from dycon_paper_replication_amd.utils import filters as F  # noqa: E402


def plain_of(plan):
    q = np.zeros(len(plan), dtype=PLAN_DTYPE)
    for f in PLAN_DTYPE.names:
        q[f] = plan[f]
    return q


def host_chain(cases, plan, rng, elastic):
    """the scipy / numpy chain of one batch (k = 0, no flip: a rot90 and a flip cost the host next to nothing) -> seconds per part"""
    from scipy import ndimage
    patch = tuple(int(v) for v in plan["patch"][0])
    t = {"warp": 0.0, "field": 0.0, "blur": 0.0, "intensity": 0.0}
    outs = []
    for rec in plan:
        img, lab, m = cases[rec["case"]]["image"], cases[rec["case"]]["label"], rec["m"].reshape(3, 3)
        if elastic:
            t0 = time.perf_counter()
            noise = rng.standard_normal((3,) + patch).astype(np.float32)
            field = np.float32(rec["alpha"]) * np.stack([ndimage.gaussian_filter(v, rec["sigma"], mode="constant") for v in noise])
            t["field"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        if elastic:
            c = W.source_coordinates(m, rec["off"], patch, field)
            oi = ndimage.map_coordinates(img, c, order=1, mode="constant")
            ol = ndimage.map_coordinates(lab, c, order=0, mode="constant")
        else:
            oi = ndimage.affine_transform(img, m, rec["off"], output_shape=patch, order=1, mode="constant")
            ol = ndimage.affine_transform(lab, m, rec["off"], output_shape=patch, order=0, mode="constant")
        t["warp"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        ob = ndimage.gaussian_filter(oi, 0.75)
        t["blur"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        W.intensity_host(ob, 1.1, 0.05, 0.8, -3.0, 3.0)
        t["intensity"] += time.perf_counter() - t0
        outs.append((oi, ol, field if elastic else None))
    return t, outs


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def load_parent(path):
    """the parent commit's dataloaders/device_cache.py as a module of this package (its relative imports resolve here)"""
    name = "dycon_paper_replication_amd.dataloaders._parent_device_cache"
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cases", type=int, default=12)
    ap.add_argument("--host-batches", type=int, default=2)
    ap.add_argument("--parent-device-cache", default=None)
    a = ap.parse_args()
    if a.regions < 3 or a.batches < 200:
        print("note: fewer than 3 regions of 200 batches is a rehearsal, not a measurement", flush=True)
    dev = "cuda:0"
    B, patch = 4, (96, 96, 96)
    vox = B * patch[0] * patch[1] * patch[2]
    lines = [f"# warp_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {a.cases} synthetic cases, B = {B} at 96^3, labels int64; the "
             f"variants alternate, median of {a.regions} regions of {a.batches} batches (min .. max); host ms = enqueue loop, no "
             f"synchronisation; GPU ms = HIP events around groups of {GROUP} batches enqueued behind a blocker kernel (back-to-back "
             f"execution); every variant works on the same 64 pre-drawn plans.  The kernels are first versions, correct and not tuned."]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    cases = make_cases(a.cases, 0)
    cache = DeviceVolumeCache(cases, device=dev)
    emit(f"cache: {len(cache)} cases, {cache.nbytes / 2**20:.1f} MiB, stored shapes {cache.shapes[0]} .. {cache.shapes[-1]}")
    rng = np.random.default_rng(1)
    batches = [[int(i) for i in rng.integers(0, len(cache), B)] for _ in range(64)]
    warp = W.Warp(p_affine=1.0, p_elastic=1.0, alpha=(50.0, 200.0), sigma=(9.0, 13.0))
    np.random.seed(11)
    t0 = time.perf_counter()
    plans_e = [W.draw_plan_warp(cache.shapes, idx, patch, warp, W.Intensity()) for idx in batches]
    draw_ms = 1e3 * (time.perf_counter() - t0) / len(plans_e)
    plans_a = [p.copy() for p in plans_e]
    for p in plans_a:
        p["elastic"] = 0
    plain = [plain_of(p) for p in plans_e]
    idle = [p.copy() for p in plans_a]
    for p in idle:
        p["warp"] = 0

    # ------------------------------------------------------------------ the host chain; its first batch is the check of (a) and (e)
    host_t = {"affine": [], "elastic": []}
    for n in range(a.host_batches):
        for name, plans, el in (("affine", plans_a, False), ("elastic", plans_e, True)):
            q = plans[n].copy()
            q["k"], q["flip_axis"] = 0, -1
            t, outs = host_chain(cases, q, np.random.default_rng(n), el)
            host_t[name].append(t)
            if n == 0:
                disp = torch.from_numpy(np.stack([o[2] for o in outs])).to(dev) if el else None
                got = W.assemble_batch_warp(cache, q, displacement=disp, label_dtype=torch.int64)
                assert np.array_equal(got["image"][:, 0].cpu().numpy().view(np.uint32), np.stack([o[0] for o in outs]).view(np.uint32)), name
                assert np.array_equal(got["label"].cpu().numpy(), np.stack([o[1] for o in outs]).astype(np.int64)), name
    emit("before anything is timed: (a) and (e) equal scipy's affine_transform / map_coordinates bit for bit on one batch")

    # ------------------------------------------------------------------ the assembly variants
    field = W.elastic_field(B, patch, plans_e[0]["alpha"], plans_e[0]["sigma"], 3, 0, device=dev)
    out = {k: assemble_batch(cache, plain[0], label_dtype=torch.int64) for k in ("p", "0", "a", "e")}
    aug = W.LoaderAugment(3, torch.device(dev))
    blur_plan, int_plan = plans_a[0].copy(), plans_a[0].copy()
    blur_plan["blur_sigma"] = np.linspace(0.5, 1.0, B)
    int_plan["gain"], int_plan["bias"], int_plan["gamma"] = 1.1, 0.05, 0.8
    image = out["a"]["image"].clone()
    fns = {"p": lambda n: assemble_batch(cache, plain[n], out=out["p"], label_dtype=torch.int64),
           "0": lambda n: W.assemble_batch_warp(cache, idle[n], out=out["0"], label_dtype=torch.int64),
           "a": lambda n: W.assemble_batch_warp(cache, plans_a[n], out=out["a"], label_dtype=torch.int64),
           "e": lambda n: W.assemble_batch_warp(cache, plans_e[n], out=out["e"], displacement=field, label_dtype=torch.int64),
           "f": lambda n: aug.field(plans_e[n], n),
           "b": lambda n: aug.values(blur_plan, image, -3.0, 3.0),
           "i": lambda n: aug.values(int_plan, image, -3.0, 3.0)}
    for n in range(4):                                                 # equal before timed; also the warm-up of every variant
        res = {k: f(n) for k, f in fns.items()}
        assert torch.equal(res["0"]["image"], res["p"]["image"]) and torch.equal(res["0"]["label"], res["p"]["label"])
    emit("before anything is timed: (0) equals (p) bit for bit on four batches")
    order = list(range(len(plans_e)))
    host, gpu, retaken, blocker = {k: [] for k in fns}, {k: [] for k in fns}, [0], [2_000_000]
    for _ in range(a.regions):
        for k, f in fns.items():
            host[k].append(host_region(f, order, a.batches))
    for _ in range(a.regions):
        for k, f in fns.items():
            gpu[k].append(gpu_region(f, order, a.batches, blocker, retaken))
    names = {"p": "(p) assemble_batch (plain kernel)       ", "0": "(0) assemble_batch_warp, warp = 0       ",
             "a": "(a) assemble_batch_warp, affine         ", "e": "(e) assemble_batch_warp, affine+elastic ",
             "f": "(f) elastic_field (noise, 3 passes x 4) ", "b": "(b) blur in place, 4 samples            ",
             "i": "(i) gain / bias / gamma, 4 samples      "}
    emit(f"patch 96^3, B = {B}: {vox * 17 / 1e6:.1f} MB per assembled batch (read 5 + written 12 per voxel); a field is {vox * 12 / 1e6:.1f} MB")
    gp = statistics.median(gpu["p"])
    for k in fns:
        emit(f"  {names[k]} host ms/batch {fmt(host[k])}   GPU ms/batch {fmt(gpu[k])}   {statistics.median(gpu[k]) / gp:6.2f} x (p)")
    emit(f"      blocker groups re-taken: {retaken[0]}; draw_plan_warp {draw_ms:.3f} ms/batch on the host (not in the rows above)")
    for name, key in (("affine", "a"), ("elastic", "e")):
        parts = {k: 1e3 * statistics.median([t[k] for t in host_t[name]]) for k in ("warp", "field", "blur", "intensity")}
        emit(f"  host chain, {name}: scipy warp (image order 1 + label order 0) {parts['warp']:.0f} ms, field {parts['field']:.0f} ms, "
             f"gaussian_filter blur {parts['blur']:.0f} ms, numpy gain / bias / gamma {parts['intensity']:.0f} ms per batch of {B} "
             f"(wall clock, median of {a.host_batches}); warp alone = {parts['warp'] / statistics.median(gpu[key]):.0f} x GPU ms of ({key})")

    # ------------------------------------------------------------------ each Gaussian pass next to a copy of the same bytes
    N = 3 * B
    x = torch.randn((N,) + patch, device=dev)
    y, z = torch.empty_like(x), torch.empty_like(x)
    nbytes = 2 * x.numel() * 4
    emit(f"Gaussian passes, {N} volumes of 96^3 ({x.numel() * 4 / 1e6:.1f} MB read + as much written per pass), HIP events around 50 "
         f"back-to-back calls, alternating with a device-to-device copy of the same bytes, median of {a.regions} (min .. max)")
    rows = {"copy": lambda: z.copy_(x)}
    for sigma, r in ((2.0, 8), (11.0, 44)):
        for axis, nm in enumerate("xyz"):
            s = [0.0, 0.0, 0.0]
            s[axis] = sigma
            rows[f"{nm} pass, sigma {sigma:4.1f} (r = {r:2d})"] = (lambda s=tuple(s): F.gaussian_filter(x, s, out=y))
    ms = {k: [] for k in rows}
    for f in rows.values():
        f()
    for _ in range(a.regions):
        for k, f in rows.items():
            ms[k].append(event_ms(f, 50))
    cp = statistics.median(ms["copy"])
    for k in rows:
        m = statistics.median(ms[k])
        emit(f"  {k:28s} ms {fmt(ms[k])}   {nbytes / m / 1e9:6.3f} TB/s   copy / pass = {cp / m:5.2f}")

    # ------------------------------------------------------------------ the default loader next to the parent commit's
    sampler = TwoStreamBatchSampler(list(range(4)), list(range(4, len(cache))), 4, 2)

    def forever(loader):
        while True:
            yield from loader
    if a.parent_device_cache:
        parent = load_parent(a.parent_device_cache)
        feeds = {"parent": forever(parent.DeviceBatchLoader(cache, sampler, patch)), "this": forever(DeviceBatchLoader(cache, sampler, patch))}
        np.random.seed(17)
        res_h, res_w = {k: [] for k in feeds}, {k: [] for k in feeds}
        for k in feeds:
            for _ in range(8):
                next(feeds[k])
        for _ in range(a.regions):
            for k, feed in feeds.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.batches):
                    next(feed)
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                res_h[k].append(1e3 * (t1 - t0) / a.batches)
                res_w[k].append(1e3 * (time.perf_counter() - t0) / a.batches)
        emit(f"default DeviceBatchLoader (warp=None, intensity=None) next to the parent commit's, alternating in this process; "
             f"{a.regions} regions of {a.batches} batches, draw + assemble")
        for k in feeds:
            emit(f"  {k:7s} host ms/batch {fmt(res_h[k])}   synchronised wall clock ms/batch {fmt(res_w[k])}")
        lo, hi, v = min(res_w["parent"]), max(res_w["parent"]), statistics.median(res_w["this"])
        emit(f"      this commit's median {v:.4f} ms lies {'inside' if lo <= v <= hi else 'OUTSIDE'} the parent's run-to-run range "
             f"{lo:.4f} .. {hi:.4f} ms")

    # ------------------------------------------------------------------ a loader-fed step next to a resident-batch step
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    tr = DyconTrainer(TrainConfig(model="vnet", batch_size=4, labeled_bs=2, dtype=torch.bfloat16, seed=1337), dev)
    full = W.Warp(p_affine=0.8, p_elastic=0.5, alpha=(50.0, 200.0), sigma=(9.0, 13.0))
    inten = W.Intensity(p_gain=0.5, p_bias=0.5, p_gamma=0.5, p_blur=0.5, range=(-3.0, 3.0))
    np.random.seed(13)
    feeds = {"plain": forever(DeviceBatchLoader(cache, sampler, patch)),
             "affine": forever(DeviceBatchLoader(cache, sampler, patch, warp=W.Warp(p_affine=0.8))),
             "full": forever(DeviceBatchLoader(cache, sampler, patch, warp=full, intensity=inten))}
    fixed = {k: v.clone() for k, v in next(feeds["full"]).items()}
    gets = {"fixed": lambda: fixed, **{k: (lambda k=k: next(feeds[k])) for k in feeds}}

    def region(get):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = get()
            o = tr.step(b["image"], b["label"])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps, o

    for get in gets.values():                                          # eager, eager, record, first replays
        for _ in range(6):
            b = get()
            tr.step(b["image"], b["label"])
    res = {k: [] for k in gets}
    for _ in range(a.regions):
        for k, get in gets.items():
            t, o = region(get)
            res[k].append(t)
    emit(f"DyconTrainer.step, V-Net bf16, B = 4 (2 + 2) at 96^3, uint8 labels, replay on; median of {a.regions} regions of {a.steps} "
         f"steps, synchronised wall clock, alternating; skipped steps {tr.skipped_steps}, last loss {float(o['loss']):.4f}")
    label = {"fixed": "fed one resident batch", "plain": "fed by DeviceBatchLoader", "affine": "fed by DeviceBatchLoader(warp=Warp(p_affine=0.8))",
             "full": "fed by DeviceBatchLoader(warp: affine 0.8 + elastic 0.5, intensity: all 0.5)"}
    fx = statistics.median(res["fixed"])
    for k in gets:
        emit(f"  {label[k]:78s} ms/step {fmt(res[k])}   {statistics.median(res[k]) - fx:+.4f} vs resident")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
