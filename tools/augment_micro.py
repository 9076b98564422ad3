#!/usr/bin/env python3
"""Batch assembly with RandomRot / CreateOnehotLabel on the device (dataloaders/device_augment.py, csrc/augment.hip) next to the plain
assembly it extends (dycon_assemble_batch, csrc/datapath.hip) ON THE SAME CROPS, next to the host chain it replaces (scipy) on the same
box, and a trainer fed by the rotating loader next to a trainer fed one resident batch.

  (p) assemble_batch                          the parent's kernel: the yardstick
  (0) assemble_batch_rot, rotate = 0          the same PLAN_DTYPE plans through the new entry point
  (r) assemble_batch_rot                      rotation
  (h) assemble_batch_rot, onehot=2 int64      rotation + one-hot planes as ToTensor leaves them
  (u) assemble_batch_rot, onehot=2 uint8      rotation + one-hot planes, one byte each
  host chain                                  RandomRot -> RandomCrop -> RandomRotFlip -> ToTensor of dataloaders/isles22.py on host
                                              arrays (scipy.ndimage.rotate of the whole stored volume, image and label), wall clock

Data, sizes and the timing method are those of tools/datapath_micro.py (whose helpers are imported): synthetic BraTS-like cases, B = 4
at 96^3 and at 112 x 112 x 80, labels int64; the plans are drawn once (64 per size, seeded) and every variant assembles the same ones,
(p) and (0) from their PLAN_DTYPE fields.  The variants ALTERNATE region by region; median over --regions regions of --batches batches
(min .. max).  host ms: the enqueue loop alone; GPU ms: HIP events around groups enqueued behind a blocker kernel (back-to-back
execution).  Before anything is timed, (r) is compared bit for bit with the host chain of the same seed, and (0) with (p).

    python tools/augment_micro.py --out profiles/augment_micro.txt --commit $(git rev-parse --short HEAD)
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from datapath_micro import GROUP, fmt, gpu_region, host_region, make_cases  # noqa: E402
from dycon_paper_replication_amd.dataloaders import (PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, assemble_batch,  # noqa: E402
                                                     assemble_batch_rot, draw_plan_rot)
from dycon_paper_replication_amd.dataloaders.isles22 import (RandomCrop, RandomRot, RandomRotFlip, ToTensor,  # noqa: E402
                                                             TwoStreamBatchSampler)


def host_chain(cases, indices, patch):
    outs = []
    for i in indices:
        s = dict(cases[i])
        for t in (RandomRot(), RandomCrop(patch), RandomRotFlip(), ToTensor()):
            s = t(s)
        outs.append(s)
    return torch.stack([o["image"] for o in outs]), torch.stack([o["label"] for o in outs])


def plain_of(plan):
    """the PLAN_DTYPE fields of a ROT_PLAN_DTYPE plan: the same crops without the rotation"""
    q = np.zeros(len(plan), dtype=PLAN_DTYPE)
    for f in PLAN_DTYPE.names:
        q[f] = plan[f]
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cases", type=int, default=12)
    ap.add_argument("--host-batches", type=int, default=3)
    a = ap.parse_args()
    if a.regions < 3 or a.batches < 200:
        print("note: fewer than 3 regions of 200 batches is a rehearsal, not a measurement", flush=True)
    dev = "cuda:0"
    B = 4
    lines = [f"# augment_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {a.cases} synthetic cases, B = {B}, labels int64; the variants "
             f"alternate, median of {a.regions} regions of {a.batches} batches (min .. max); host ms = enqueue loop, no synchronisation; "
             f"GPU ms = HIP events around groups of {GROUP} batches enqueued behind a blocker kernel (back-to-back execution); every "
             f"variant assembles the same 64 pre-drawn plans"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    cases = make_cases(a.cases, 0)
    cache = DeviceVolumeCache(cases, device=dev)
    emit(f"cache: {len(cache)} cases, {cache.nbytes / 2**20:.1f} MiB, stored shapes {cache.shapes[0]} .. {cache.shapes[-1]}")
    rng = np.random.default_rng(1)
    batches = [[int(i) for i in rng.integers(0, len(cache), B)] for _ in range(64)]
    blocker = [2_000_000]
    for patch in ((96, 96, 96), (112, 112, 80)):
        # the host chain first: its batches are the check of (r), its wall clock the figure to put next to the kernels
        host_ms = []
        for n in range(a.host_batches):
            np.random.seed(100 + n)
            t0 = time.perf_counter()
            ref_i, ref_l = host_chain(cases, batches[n], patch)
            host_ms.append(1e3 * (time.perf_counter() - t0))
            np.random.seed(100 + n)
            got = assemble_batch_rot(cache, draw_plan_rot(cache.shapes, batches[n], patch), label_dtype=torch.int64)
            assert torch.equal(got["image"].cpu(), ref_i) and torch.equal(got["label"].cpu(), ref_l), patch
        np.random.seed(11)
        t0 = time.perf_counter()
        plans = [draw_plan_rot(cache.shapes, idx, patch) for idx in batches]
        draw_ms = 1e3 * (time.perf_counter() - t0) / len(plans)
        plain = [plain_of(p) for p in plans]
        out = {k: assemble_batch_rot(cache, plans[0], label_dtype=torch.int64, onehot=2, onehot_dtype=dt)
               for k, dt in (("h", torch.int64), ("u", torch.uint8))}
        out["p"] = assemble_batch(cache, plain[0], label_dtype=torch.int64)
        out["0"] = assemble_batch_rot(cache, plain[0], label_dtype=torch.int64)
        out["r"] = assemble_batch_rot(cache, plans[0], label_dtype=torch.int64)
        fns = {"p": lambda n: assemble_batch(cache, plain[n], out=out["p"], label_dtype=torch.int64),
               "0": lambda n: assemble_batch_rot(cache, plain[n], out=out["0"], label_dtype=torch.int64),
               "r": lambda n: assemble_batch_rot(cache, plans[n], out=out["r"], label_dtype=torch.int64),
               "h": lambda n: assemble_batch_rot(cache, plans[n], out=out["h"], label_dtype=torch.int64, onehot=2),
               "u": lambda n: assemble_batch_rot(cache, plans[n], out=out["u"], label_dtype=torch.int64, onehot=2,
                                                 onehot_dtype=torch.uint8)}
        for n in range(4):                                             # equal before timed; also the warm-up of every variant
            res = {k: {kk: v.clone() for kk, v in f(n).items()} for k, f in fns.items()}
            assert torch.equal(res["0"]["image"], res["p"]["image"]) and torch.equal(res["0"]["label"], res["p"]["label"]), patch
            for k in ("h", "u"):
                assert torch.equal(res[k]["image"], res["r"]["image"]) and torch.equal(res[k]["label"], res["r"]["label"]), patch
        order = list(range(len(plans)))
        host, gpu, retaken = {k: [] for k in fns}, {k: [] for k in fns}, [0]
        for _ in range(a.regions):
            for k, f in fns.items():
                host[k].append(host_region(f, order, a.batches))
        for _ in range(a.regions):
            for k, f in fns.items():
                gpu[k].append(gpu_region(f, order, a.batches, blocker, retaken))
        vox = B * patch[0] * patch[1] * patch[2]
        per_vox = {"p": 17, "0": 17, "r": 17, "h": 17 + 16, "u": 17 + 2}       # read 5 (fp32 + uint8), written 4 + 8 (+ 2 planes)
        emit(f"patch {patch[0]} x {patch[1]} x {patch[2]}, B = {B}; bytes per batch {vox * 17 / 1e6:.1f} MB (read 5 + written 12 per voxel), "
             f"+ {vox * 16 / 1e6:.1f} MB for two int64 one-hot planes, + {vox * 2 / 1e6:.1f} MB for two uint8 ones")
        names = {"p": "(p) assemble_batch (parent kernel)  ", "0": "(0) assemble_batch_rot, rotate = 0 ", "r": "(r) assemble_batch_rot, rotation   ",
                 "h": "(h) rotation + one-hot 2 x int64   ", "u": "(u) rotation + one-hot 2 x uint8   "}
        gp = statistics.median(gpu["p"])
        for k in fns:
            g = statistics.median(gpu[k])
            emit(f"  {names[k]} host ms/batch {fmt(host[k])}   GPU ms/batch {fmt(gpu[k])}   {g / gp:5.2f} x (p)   "
                 f"{vox * per_vox[k] / g / 1e9:5.2f} TB/s")
        emit(f"      blocker groups re-taken: {retaken[0]}; draw_plan_rot {draw_ms:.3f} ms/batch on the host (not in the rows above)")
        emit(f"  host chain RandomRot -> RandomCrop -> RandomRotFlip -> ToTensor (scipy), wall clock ms/batch over {a.host_batches} batches: "
             f"{fmt(host_ms)}   = {statistics.median(host_ms) / statistics.median(gpu['r']):.0f} x GPU ms of (r)")

    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    patch = (96, 96, 96)
    tr = DyconTrainer(TrainConfig(model="vnet", batch_size=4, labeled_bs=2, dtype=torch.bfloat16, seed=1337), dev)
    sampler = TwoStreamBatchSampler(list(range(4)), list(range(4, len(cache))), 4, 2)

    def forever(loader):
        while True:
            yield from loader
    np.random.seed(13)
    feeds = {"plain": forever(DeviceBatchLoader(cache, sampler, patch)), "rot": forever(DeviceBatchLoader(cache, sampler, patch, rot=True))}
    fixed = {k: v.clone() for k, v in next(feeds["rot"]).items()}
    gets = {"fixed": lambda: fixed, "plain": lambda: next(feeds["plain"]), "rot": lambda: next(feeds["rot"])}

    def region(get):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = get()
            out = tr.step(b["image"], b["label"])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps, out

    for get in gets.values():                                          # eager, eager, record, first replays
        for _ in range(6):
            b = get()
            tr.step(b["image"], b["label"])
    res = {k: [] for k in gets}
    for _ in range(a.regions):
        for k, get in gets.items():
            ms, out = region(get)
            res[k].append(ms)
    emit(f"DyconTrainer.step, V-Net bf16, B = 4 (2 + 2) at 96^3, uint8 labels, replay on; median of {a.regions} regions of {a.steps} "
         f"steps, synchronised wall clock, alternating; skipped steps {tr.skipped_steps}, last loss {float(out['loss']):.4f}")
    emit(f"  fed one resident batch                  ms/step {fmt(res['fixed'])}")
    emit(f"  fed by DeviceBatchLoader                ms/step {fmt(res['plain'])}")
    emit(f"  fed by DeviceBatchLoader(rot=True)      ms/step {fmt(res['rot'])}")
    fx = statistics.median(res["fixed"])
    emit(f"      loader-fed - resident: plain {statistics.median(res['plain']) - fx:+.4f} ms/step, rot=True "
         f"{statistics.median(res['rot']) - fx:+.4f} ms/step")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
