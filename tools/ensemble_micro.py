#!/usr/bin/env python3
"""The model-ensemble sliding window (utils/ensemble_eval.py, csrc/ensemble.hip) next to what it stands beside, in the same process on
the same box, at the LA geometry: a 175 x 132 x 88 volume, windows 112 x 112 x 80, stride 18 / 4 (45 windows, chunks of 4), two bf16
V-Nets.

  per chunk  (a) the glue the single-model evaluators had before they shared the ensemble's driver: `batch_size` slice copies, stack,
                 contiguous, and the host-to-device copy of the chunk's origins;
             (b) one dycon_sw_gather launch from the origin table uploaded once per case, what sliding_window._sliding_window does.
             Compared bit for bit before anything is timed.  host ms: wall clock of the enqueue loop, no synchronisation inside a
             region.  GPU ms: HIP events around groups of chunks enqueued behind a blocker kernel (back-to-back execution); the
             origin upload of (a) is a synchronous copy that cannot be enqueued behind a blocker, so it is in (a)'s host ms only.
  per case   (c) single_case_plus_device(l, r): gather, two forwards, one accumulate per chunk;
             (d) single_case_device(l) then single_case_device(r): the floor the two forwards set (and not the same function: the
                 mean of two probability maps is not the softmax of the mean logits).
             Synchronised wall clock, (c) and (d) alternating.
The figure is the median over --regions regions (min .. max: the spread on this box).

    python tools/ensemble_micro.py --out profiles/ensemble_micro.txt --commit $(git rev-parse --short HEAD)
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

from datapath_micro import fmt, gpu_region, host_region  # noqa: E402
from dycon_paper_replication_amd import _lib  # noqa: E402
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d  # noqa: E402
from dycon_paper_replication_amd.utils import ensemble_eval as EE  # noqa: E402
from dycon_paper_replication_amd.utils import sliding_window as SW  # noqa: E402
from dycon_paper_replication_amd.utils.test_3d_patch import _windows  # noqa: E402

SHAPE, PATCH, STRIDE_XY, STRIDE_Z, BATCH = (175, 132, 88), (112, 112, 80), 18, 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--chunks", type=int, default=200, help="chunks per region of the per-chunk comparison")
    ap.add_argument("--cases", type=int, default=20, help="cases per region of the per-case comparison")
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPE)
    ap.add_argument("--patch", type=int, nargs=3, default=PATCH)
    a = ap.parse_args()
    shape, patch = tuple(a.shape), tuple(a.patch)
    if a.regions < 3 or a.chunks < 200 or shape != SHAPE or patch != PATCH:
        print("note: fewer than 3 regions of 200 chunks, or another geometry than LA's, is a rehearsal, not a measurement", flush=True)
    dev = "cuda:0"
    lines = [f"# ensemble_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; volume {shape}, windows {patch}, stride {STRIDE_XY} / "
             f"{STRIDE_Z}, chunks of {BATCH}; alternating, median of {a.regions} regions (min .. max)"]

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    rng = np.random.default_rng(0)
    image = rng.standard_normal(shape).astype(np.float32)
    vol = torch.from_numpy(image).to(dev)
    assert all(s >= p for s, p in zip(shape, patch)), "the glue of (a) slices the volume itself: no padded axis here"
    wins = _windows(shape, patch, STRIDE_XY, STRIDE_Z)
    chunks = [wins[i:i + BATCH] for i in range(0, len(wins), BATCH)]
    table = torch.tensor(wins, dtype=torch.int32).to(dev)
    p0, p1, p2 = patch
    out = torch.empty((BATCH, 1) + patch, dtype=torch.float32, device=dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731

    def glue(i, upload=True):
        chunk = chunks[i]
        patches = torch.stack([vol[x:x + p0, y:y + p1, z:z + p2] for x, y, z in chunk]).unsqueeze(1).contiguous()
        if upload:
            torch.tensor(chunk, dtype=torch.int32).to(dev)
        return patches

    def gather(i):
        nb = len(chunks[i])
        _lib.call("dycon_sw_gather", vol.data_ptr(), *shape, table.data_ptr(), len(wins), BATCH * i, nb, p0, p1, p2, out.data_ptr(), stream())
        return out[:nb]

    for i in range(len(chunks)):                                       # equal before timed; also the warm-up of both
        assert torch.equal(glue(i), gather(i)), i
    idx = list(range(len(chunks)))
    host, gpu, retaken, blocker = {"a": [], "b": []}, {"a": [], "b": []}, [0], [2_000_000]
    for _ in range(a.regions):
        for name, fn in (("a", glue), ("b", gather)):
            host[name].append(host_region(fn, idx, a.chunks))
    for _ in range(a.regions):
        for name, fn in (("a", lambda i: glue(i, upload=False)), ("b", gather)):
            gpu[name].append(gpu_region(fn, idx, a.chunks, blocker, retaken))
    nbytes = 2 * 4 * BATCH * p0 * p1 * p2
    emit(f"per chunk of {BATCH} windows ({len(wins)} windows, {len(chunks)} chunks per case; {nbytes / 1e6:.1f} MB read + written); "
         f"{a.chunks} chunks per region")
    emit(f"  (a) slices + stack + contiguous + origin upload   host ms/chunk {fmt(host['a'])}   GPU ms/chunk {fmt(gpu['a'])} (no upload)")
    emit(f"  (b) dycon_sw_gather, origins uploaded per case    host ms/chunk {fmt(host['b'])}   GPU ms/chunk {fmt(gpu['b'])}")
    gb = statistics.median(gpu["b"])
    emit(f"      (a) / (b): host {statistics.median(host['a']) / statistics.median(host['b']):.2f}x, GPU "
         f"{statistics.median(gpu['a']) / gb:.2f}x; (b) moves {nbytes / gb / 1e9:.2f} TB/s; blocker groups re-taken: {retaken[0]}")

    torch.manual_seed(0)
    nets = [net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).to(dev) for _ in range(2)]
    args = (image, STRIDE_XY, STRIDE_Z, patch)

    def ensemble():
        return EE.single_case_plus_device(nets[0], nets[1], *args, batch_size=BATCH)

    def singles():
        return [SW.single_case_device(n, *args, batch_size=BATCH) for n in nets]

    def region(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.cases):
            r = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / a.cases, r

    for fn in (ensemble, singles, ensemble, singles):                 # warm-up: code objects, packed weights, the allocator
        fn()
    res = {"c": [], "d": []}
    for _ in range(a.regions):
        for name, fn in (("c", ensemble), ("d", singles)):
            ms, r = region(fn)
            res[name].append(ms)
            if name == "c":
                ens = r
            else:
                one = r
    self_l, self_p = EE.single_case_plus_device(nets[0], nets[0], *args, batch_size=BATCH)
    emit(f"per case, two bf16 V-Nets, {a.cases} cases per region, synchronised wall clock; self-ensemble == single_case_device: "
         f"{bool(torch.equal(self_l, one[0][0]) and torch.equal(self_p, one[0][1]))}; ensemble label != member label on "
         f"{[round(float((ens[0] != o[0]).float().mean()), 4) for o in one]} of the voxels")
    emit(f"  (c) single_case_plus_device(l, r)                  ms/case {fmt(res['c'])}")
    emit(f"  (d) single_case_device(l); single_case_device(r)   ms/case {fmt(res['d'])}")
    emit(f"      (c) - (d): {statistics.median(res['c']) - statistics.median(res['d']):+.3f} ms/case; (c) / (d) "
         f"{statistics.median(res['c']) / statistics.median(res['d']):.3f}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
