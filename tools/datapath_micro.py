#!/usr/bin/env python3
"""Batch assembly from a volume cache in HBM (dataloaders/device_cache.py, csrc/datapath.hip) next to the path it replaces, in the same
process on the same box, and a trainer fed by the loader next to a trainer fed one resident batch.

  (a) the per-sample device path: this package's RandomCrop -> RandomRotFlip -> ToTensor applied to CUDA tensors (views of the same
      cached volumes), image and label, then torch.stack;
  (b) draw_plan + assemble_batch into a preallocated output pair (one launch).

Data: synthetic cases of BraTS-like stored shapes (about 150 x 175 x 140 after SagittalToAxial), z-scored noise images, blob labels.
Sizes: B = 4 at 96^3 and at 112 x 112 x 80.  Before anything is timed the two paths are compared bit for bit on the same seed.

What is timed, per batch.  The two paths ALTERNATE region by region; a region is --batches batches; the figure is the median over
--regions regions (min .. max in brackets: the run-to-run spread on this box).
  host ms : wall clock of the enqueue loop alone (no synchronisation inside the region): what the host spends to issue a batch.
  GPU ms  : the batches of a region are enqueued in groups behind a spinning blocker kernel, so that they execute back to back; HIP
            events around each group, summed over the region.  This is the time the GPU needs, without the gaps the host leaves.
            A group whose enqueue outlasted the blocker is re-taken with a longer blocker (counted in the report).
  trainer : synchronised wall clock over --steps steps of DyconTrainer.step (V-Net bf16, B = 4 (2 + 2) at 96^3, replay on), fed
            (i) one fixed resident batch, (ii) the DeviceBatchLoader's batches; alternating, median of --regions regions.

    python tools/datapath_micro.py --out profiles/datapath_micro.txt --commit $(git rev-parse --short HEAD)
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

from dycon_paper_replication_amd.dataloaders import DeviceBatchLoader, DeviceVolumeCache, assemble_batch, draw_plan  # noqa: E402
from dycon_paper_replication_amd.dataloaders.brats19 import RandomCrop, RandomRotFlip, ToTensor, TwoStreamBatchSampler  # noqa: E402
from dycon_paper_replication_amd.synthetic import blob_labels  # noqa: E402

GROUP = 20          # batches enqueued behind one blocker


def make_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        shape = tuple(int(v) for v in (rng.integers(140, 161), rng.integers(165, 186), rng.integers(130, 151)))
        cases.append({"image": rng.standard_normal(shape).astype(np.float32), "label": blob_labels(rng, 1, *shape)[0]})
    return cases


def case_views(cache):
    """the cached cases as (X, Y, Z) CUDA tensors: views of the arenas, so both paths read the same memory"""
    out = []
    for i, s in enumerate(cache.shapes):
        n, oi, ol = s[0] * s[1] * s[2], int(cache._img_off[i]), int(cache._lab_off[i])
        out.append({"image": cache.images[oi:oi + n].view(s), "label": cache.labels[ol:ol + n].view(s)})
    return out


class PerSamplePath:
    """(a): the transforms of dataloaders/brats19.py on CUDA tensors, sample by sample, then torch.stack"""

    def __init__(self, views, patch):
        self.views, self.tfs = views, (RandomCrop(patch), RandomRotFlip(), ToTensor())

    def __call__(self, indices):
        outs = []
        for i in indices:
            s = self.views[i]
            for t in self.tfs:
                s = t(s)
            outs.append(s)
        return {"image": torch.stack([o["image"] for o in outs]), "label": torch.stack([o["label"] for o in outs])}


class OneLaunchPath:
    """(b): draw_plan + assemble_batch into a preallocated pair"""

    def __init__(self, cache, patch, B):
        self.cache, self.patch, self.shapes = cache, patch, cache.shapes
        self.out = assemble_batch(cache, draw_plan(self.shapes, [0] * B, patch), label_dtype=torch.int64)

    def __call__(self, indices):
        return assemble_batch(self.cache, draw_plan(self.shapes, indices, self.patch), out=self.out, label_dtype=torch.int64)


def host_region(fn, batches, nb):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for n in range(nb):
        fn(batches[n % len(batches)])
    dt = time.perf_counter() - t0
    torch.cuda.synchronize()
    return 1e3 * dt / nb


def gpu_region(fn, batches, nb, blocker_cycles, retaken):
    """-> ms per batch of back-to-back execution; blocker_cycles is a one-element list (lengthened when a group has to be re-taken)"""
    total, done = 0.0, 0
    while done < nb:
        g = min(GROUP, nb - done)
        for _ in range(6):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda._sleep(blocker_cycles[0])
            e0.record()
            for n in range(g):
                fn(batches[(done + n) % len(batches)])
            e1.record()
            behind = not e0.query()             # the blocker was still spinning when the last launch was enqueued
            e1.synchronize()
            if behind:
                break
            retaken[0] += 1
            blocker_cycles[0] *= 2
        else:
            raise RuntimeError("the enqueue of a group outlasts every blocker tried")
        total += e0.elapsed_time(e1)
        done += g
    return total / nb


def fmt(v):
    return f"{statistics.median(v):8.4f} ({min(v):.4f} .. {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--cases", type=int, default=12)
    a = ap.parse_args()
    if a.regions < 3 or a.batches < 200:
        print("note: fewer than 3 regions of 200 batches is a rehearsal, not a measurement", flush=True)
    dev = "cuda:0"
    B = 4
    lines = [f"# datapath_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; {a.cases} synthetic cases, B = {B}; (a) and (b) alternate, "
             f"median of {a.regions} regions of {a.batches} batches (min .. max); host ms = enqueue loop, no synchronisation; GPU ms = "
             f"HIP events around groups of {GROUP} batches enqueued behind a blocker kernel (back-to-back execution)"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    cases = make_cases(a.cases, 0)
    cache = DeviceVolumeCache(cases, device=dev)
    views = case_views(cache)
    emit(f"cache: {len(cache)} cases, {cache.nbytes / 2**20:.1f} MiB, stored shapes {cache.shapes[0]} .. {cache.shapes[-1]}")
    rng = np.random.default_rng(1)
    batches = [[int(i) for i in rng.integers(0, len(cache), B)] for _ in range(64)]
    blocker = [2_000_000]
    for patch in ((96, 96, 96), (112, 112, 80)):
        pa, pb = PerSamplePath(views, patch), OneLaunchPath(cache, patch, B)
        for idx in batches[:4]:                                        # equal before timed; also the warm-up of both paths
            np.random.seed(7)
            ra = pa(idx)
            np.random.seed(7)
            rb = pb(idx)
            assert torch.equal(ra["image"], rb["image"]) and torch.equal(ra["label"], rb["label"]), patch
        host, gpu, retaken = {"a": [], "b": []}, {"a": [], "b": []}, [0]
        np.random.seed(11)
        for _ in range(a.regions):
            for name, fn in (("a", pa), ("b", pb)):
                host[name].append(host_region(fn, batches, a.batches))
        for _ in range(a.regions):
            for name, fn in (("a", pa), ("b", pb)):
                gpu[name].append(gpu_region(fn, batches, a.batches, blocker, retaken))
        vox = B * patch[0] * patch[1] * patch[2]
        emit(f"patch {patch[0]} x {patch[1]} x {patch[2]}, B = {B}, labels int64 (as ToTensor); bytes per batch {vox * (4 + 1 + 4 + 8) / 1e6:.1f} MB "
             f"(read 5 + written 12 per voxel)")
        emit(f"  (a) per-sample transforms + stack   host ms/batch {fmt(host['a'])}   GPU ms/batch {fmt(gpu['a'])}")
        emit(f"  (b) draw_plan + assemble_batch      host ms/batch {fmt(host['b'])}   GPU ms/batch {fmt(gpu['b'])}")
        gb = statistics.median(gpu["b"])
        emit(f"      (a) / (b): host {statistics.median(host['a']) / statistics.median(host['b']):.1f}x, GPU "
             f"{statistics.median(gpu['a']) / gb:.1f}x; (b) moves {vox * 17 / gb / 1e9:.2f} TB/s; blocker groups re-taken: {retaken[0]}")

    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    patch = (96, 96, 96)
    tr = DyconTrainer(TrainConfig(model="vnet", batch_size=4, labeled_bs=2, dtype=torch.bfloat16, seed=1337), dev)
    sampler = TwoStreamBatchSampler(list(range(4)), list(range(4, len(cache))), 4, 2)
    loader = DeviceBatchLoader(cache, sampler, patch)

    def forever():
        while True:
            yield from loader
    np.random.seed(13)
    feed = forever()
    fixed = {k: v.clone() for k, v in next(feed).items()}

    def region(get):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            b = get()
            out = tr.step(b["image"], b["label"])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.steps, out

    for get in (lambda: fixed, lambda: next(feed)):                # eager, eager, record, first replays
        for _ in range(6):
            b = get()
            tr.step(b["image"], b["label"])
    res = {"fixed": [], "loader": []}
    for _ in range(a.regions):
        for name, get in (("fixed", lambda: fixed), ("loader", lambda: next(feed))):
            ms, out = region(get)
            res[name].append(ms)
    emit(f"DyconTrainer.step, V-Net bf16, B = 4 (2 + 2) at 96^3, uint8 labels, replay on; median of {a.regions} regions of {a.steps} "
         f"steps, synchronised wall clock, alternating; skipped steps {tr.skipped_steps}, last loss {float(out['loss']):.4f}")
    emit(f"  fed one resident batch        ms/step {fmt(res['fixed'])}")
    emit(f"  fed by DeviceBatchLoader      ms/step {fmt(res['loader'])}")
    emit(f"      loader-fed - resident: {statistics.median(res['loader']) - statistics.median(res['fixed']):+.4f} ms/step")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
