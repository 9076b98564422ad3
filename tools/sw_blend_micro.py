#!/usr/bin/env python3
"""What `sliding_window.Blend` costs, at the BraTS geometry: one bf16 V-Net, a 192 x 192 x 64 volume, windows 96 x 96 x 64, stride
16 / 4 (49 windows), batch 4.

  (a) blend=None against the parent commit.  `--parent DIR` names a checkout of the parent with its library built; every run is a
      fresh process that imports ONE of the two trees, parent and this tree alternating.  The figure of a run is the median of its
      regions; "range" is the parent's own min .. max over its runs, the spread this file shows for repeated runs of the same code.
      The two trees' probability maps are compared as bytes.
  (b) Blend("gaussian"), no mirror.  The gather and accumulate launches of one chunk, plain and blended, on the same buffers: GPU ms
      from HIP events around groups of launches enqueued behind a blocker kernel (tools/datapath_micro.py), and the case time.
  (c) Blend("gaussian", mirror_axes=(0, 1, 2)): 8 forwards per window.  The case time, and the share of it that is not model
      forward: (the same case with every forward replaced by a cached logits tensor: upload, gathers, layout conversion, accumulates,
      finalize and the host's work between them) / (the case).  The forwards are not timed in a loop of their own: without the
      launches between them they do not run as they do inside the case.
Case times are synchronised wall clock over --cases cases per region, median of --regions regions (min .. max), the variants
alternating.

    python tools/sw_blend_micro.py --parent ../parent --out profiles/sw_blend_micro.txt --commit $(git rev-parse --short HEAD)
"""
import argparse
import ctypes
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


def _case_region(fn, cases):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(cases):
        r = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / cases, r


def _net_and_image(shape):
    import torch
    from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
    torch.manual_seed(0)
    net = net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).to("cuda:0")
    return net, np.random.default_rng(0).standard_normal(shape).astype(np.float32)


def worker(a):
    """(a): blend=None in the tree `a.root`, through nothing but what both trees have"""
    sys.path.insert(0, a.root)
    from dycon_paper_replication_amd.utils import sliding_window as SW
    assert os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(SW.__file__)))) == os.path.abspath(a.root)
    net, image = _net_and_image(tuple(a.shape))

    def plain():
        return SW.single_case_device(net, image, STRIDE_XY, STRIDE_Z, tuple(a.patch), batch_size=BATCH)

    for _ in range(3):
        plain()
    ms = []
    for _ in range(a.regions):
        t, r = _case_region(plain, a.cases)
        ms.append(t)
    print("RESULT " + json.dumps({"ms": ms, "sha": hashlib.sha1(r[1].cpu().numpy().tobytes()).hexdigest()}), flush=True)


def _spread(v):
    return f"median {statistics.median(v):.3f} (min {min(v):.3f} .. max {max(v):.3f}; runs {', '.join(f'{x:.3f}' for x in v)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit with libdycon_hip.so built")
    ap.add_argument("--runs", type=int, default=5, help="fresh processes per tree for (a)")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--cases", type=int, default=10, help="cases per region")
    ap.add_argument("--launches", type=int, default=200, help="launches per region of the kernel comparison")
    ap.add_argument("--shape", type=int, nargs=3, default=SHAPE)
    ap.add_argument("--patch", type=int, nargs=3, default=PATCH)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--root", default=HERE, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    shape, patch = tuple(a.shape), tuple(a.patch)
    rehearsal = a.parent is None or a.runs < 3 or a.regions < 3 or shape != SHAPE or patch != PATCH
    if rehearsal:
        print("note: without --parent, with fewer than 3 runs or regions, or at another geometry, this is a rehearsal, not a measurement",
              flush=True)
    lines = []

    def emit(s):
        lines.append(s)
        print(s, flush=True)

    # ---- (a): fresh processes, before this process touches the GPU
    trees = ([("parent", os.path.abspath(a.parent))] if a.parent else []) + [("branch", HERE)]
    runs, shas = {name: [] for name, _ in trees}, {name: set() for name, _ in trees}
    for _ in range(a.runs):
        for name, root in trees:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--regions", str(a.regions), "--cases", str(a.cases),
                   "--shape", *map(str, shape), "--patch", *map(str, patch)]
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600).stdout
            res = json.loads([l for l in out.splitlines() if l.startswith("RESULT ")][-1][7:])
            runs[name].append(statistics.median(res["ms"]))
            shas[name].add(res["sha"])
            print(f"  {name}: {runs[name][-1]:.3f} ms/case", flush=True)

    import torch
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(HERE, "tools"))
    from datapath_micro import fmt, gpu_region
    from dycon_paper_replication_amd import _lib
    from dycon_paper_replication_amd.utils import sliding_window as SW
    from dycon_paper_replication_amd.utils.sliding_window import Blend

    dev = "cuda:0"
    lines[:0] = [f"# sw_blend_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
                 f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; one bf16 V-Net, volume {shape}, windows {patch}, stride "
                 f"{STRIDE_XY} / {STRIDE_Z}, chunks of {BATCH}; {a.cases} cases per region, median of {a.regions} regions (min .. max)"]
    for l in lines:
        print(l, flush=True)
    emit(f"(a) blend=None, ms/case; {a.runs} fresh processes per tree, alternating; a run = the median of its {a.regions} regions")
    for name, _ in trees:
        emit(f"    {name:6s}  {_spread(runs[name])}")
    if a.parent:
        ratio = statistics.median(runs["branch"]) / statistics.median(runs["parent"])
        med = statistics.median(runs["branch"])
        where = "inside" if min(runs["parent"]) <= med <= max(runs["parent"]) else "below" if med < min(runs["parent"]) else "ABOVE"
        emit(f"    branch / parent {ratio:.3f}: {where} the parent's range; probability maps equal as bytes: "
             f"{len(shas['parent'] | shas['branch']) == 1}")

    # ---- (b), kernels: one chunk's launches on the same buffers
    net, image = _net_and_image(shape)
    p0, p1, p2 = patch
    wins = SW._windows(shape, patch, STRIDE_XY, STRIDE_Z)
    assert all(s >= p for s, p in zip(shape, patch))
    nchunks = (len(wins) + BATCH - 1) // BATCH
    vol = torch.from_numpy(image).to(dev)
    org = torch.tensor(wins, dtype=torch.int32).to(dev)
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    gaussian = Blend("gaussian")
    ent = {"gaussian": torch.from_numpy(SW.window_entries(wins, ())).to(dev)}
    flipped = SW.window_entries(wins, ())
    flipped[:, 3] = 7
    ent["gaussian, mask 7"] = torch.from_numpy(flipped).to(dev)
    tabs = [torch.from_numpy(g).to(dev) for g in SW.window_weights(patch, gaussian)]
    out = torch.empty((BATCH, 1) + patch, dtype=torch.float32, device=dev)
    logits = torch.randn((BATCH,) + patch + (2,), dtype=torch.float32, device=dev)
    score, cnt = torch.zeros(shape, dtype=torch.float32, device=dev), torch.zeros(shape, dtype=torch.float32, device=dev)
    int3 = lambda v: (ctypes.c_int * 3)(*v)   # noqa: E731

    def nb(i):
        return min(BATCH, len(wins) - BATCH * i)

    def gather_plain(i):
        _lib.call("dycon_sw_gather", vol.data_ptr(), *shape, org.data_ptr(), len(wins), BATCH * i, nb(i), p0, p1, p2, out.data_ptr(), stream())

    def gather_mirror(table):
        def fn(i):
            _lib.call("dycon_sw_gather_mirror", vol.data_ptr(), *shape, table.data_ptr(), len(wins), BATCH * i, nb(i), p0, p1, p2,
                      out.data_ptr(), stream())
        return fn

    def acc_plain(i):
        _lib.call("dycon_sw_accumulate", logits.data_ptr(), nb(i), p0, p1, p2, org.data_ptr() + 12 * BATCH * i, score.data_ptr(),
                  cnt.data_ptr(), *shape, stream())

    def acc_weighted(table, boxed):
        def fn(i):
            lo, hi = SW.chunk_box(wins[BATCH * i:BATCH * i + nb(i)], patch) if boxed else (None, None)
            _lib.call("dycon_sw_accumulate_weighted", logits.data_ptr(), None, None, None, 1, 2, 0, nb(i), p0, p1, p2,
                      table.data_ptr() + 16 * BATCH * i, *(t.data_ptr() for t in tabs), score.data_ptr(), cnt.data_ptr(), *shape,
                      int3(lo) if boxed else None, int3(hi) if boxed else None, stream())
        return fn

    variants = [("gather", "dycon_sw_gather", gather_plain),
                ("gather", "dycon_sw_gather_mirror, mask 0", gather_mirror(ent["gaussian"])),
                ("gather", "dycon_sw_gather_mirror, mask 7", gather_mirror(ent["gaussian, mask 7"])),
                ("accumulate", "dycon_sw_accumulate (whole volume)", acc_plain),
                ("accumulate", "dycon_sw_accumulate_weighted, mask 0, whole volume", acc_weighted(ent["gaussian"], False)),
                ("accumulate", "dycon_sw_accumulate_weighted, mask 0, the chunk's box", acc_weighted(ent["gaussian"], True)),
                ("accumulate", "dycon_sw_accumulate_weighted, mask 7, the chunk's box", acc_weighted(ent["gaussian, mask 7"], True))]
    idx = list(range(nchunks))
    for _, _, fn in variants:
        for i in idx:
            fn(i)
    gpu, retaken, blocker = {name: [] for _, name, _ in variants}, [0], [2_000_000]
    for _ in range(a.regions):
        for _, name, fn in variants:
            gpu[name].append(gpu_region(fn, idx, a.launches, blocker, retaken))
    emit(f"(b) one chunk of {BATCH} windows ({len(wins)} windows, {nchunks} chunks per case), GPU ms/launch, {a.launches} launches per region; "
         f"blocker groups re-taken: {retaken[0]}")
    base = {}
    for kind, name, _ in variants:
        base.setdefault(kind, statistics.median(gpu[name]))
        emit(f"    {name:58s} {fmt(gpu[name])}   x {statistics.median(gpu[name]) / base[kind]:.3f}")

    # ---- (b), (c): the case
    args = (image, STRIDE_XY, STRIDE_Z, patch)
    mirror = Blend("gaussian", mirror_axes=(0, 1, 2))

    class Cached(torch.nn.Module):
        """the net's logits of one chunk, computed once: the case without its forwards"""

        def __init__(self):
            super().__init__()
            net.eval()
            with torch.no_grad():
                self.logits = net(torch.zeros((BATCH, 1) + patch, dtype=torch.float32, device=dev))[1]
            net.train()

        def forward(self, x):
            return None, self.logits[:x.shape[0]], None

    cached = Cached()

    cases = [("blend=None", lambda: SW.single_case_device(net, *args, batch_size=BATCH)),
             ("Blend('gaussian')", lambda: SW.single_case_device(net, *args, batch_size=BATCH, blend=gaussian)),
             ("Blend('gaussian', mirror_axes=(0, 1, 2))", lambda: SW.single_case_device(net, *args, batch_size=BATCH, blend=mirror)),
             ("the line above, every forward replaced by cached logits",
              lambda: SW.single_case_device(cached, *args, batch_size=BATCH, device=dev, blend=mirror))]
    res, last = {name: [] for name, _ in cases}, {}
    for _, fn in cases:
        fn()
        fn()
    for _ in range(a.regions):
        for name, fn in cases:
            ms, last[name] = _case_region(fn, max(a.cases // 5, 1) if "mirror" in name else a.cases)
            res[name].append(ms)
    emit("(b), (c) the case, ms/case, synchronised wall clock, the four lines alternating")
    for name, _ in cases:
        emit(f"    {name:58s} {fmt(res[name])}")
    med = {name: statistics.median(v) for name, v in res.items()}
    names = [name for name, _ in cases]
    changed = [float((last[n][0] != last[names[0]][0]).float().mean()) for n in names[1:3]]
    emit(f"    gaussian / none {med[names[1]] / med[names[0]]:.3f}; mirror / none {med[names[2]] / med[names[0]]:.3f} (8 forwards per window); "
         f"not model forward in the mirrored case: {med[names[3]] / med[names[2]]:.3f} of its time; labels changed against "
         f"blend=None (random weights): {changed[0]:.4f}, {changed[1]:.4f}")
    same = SW.single_case_device(net, *args, batch_size=BATCH, blend=Blend("constant"))
    emit(f"    Blend('constant') == blend=None as bits: {bool(torch.equal(same[1], last[names[0]][1]) and torch.equal(same[0], last[names[0]][0]))}")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
