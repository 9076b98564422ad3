#!/usr/bin/env python3
"""Time of the device `nms` step (utils/components.py, csrc/components.hip) next to the host path it replaces, in the same process on
the same box:

  * components.largest_component on one 240 x 240 x 155 mask, a ball and a ball plus 1 % speckle, and on a (4, 96, 96, 96) batch,
    against what the host path needs for the same step: the `.cpu()` of the uint8 label map, `test_3d_patch.getLargestCC`, and the
    copy of the kept mask back to the device;
  * one synthetic 240 x 240 x 155 case through the bf16 V-Net end to end: device_eval.test_all_case(nms=1) against
    surface_eval.test_all_case(device_surface=True, nms=1).

Kernel rows, device: HIP events around the call, warm-up, then the median of the timed repeats (min in brackets).  Host and the
end-to-end rows: synchronised wall clock, median of --host-reps.  Before anything is timed the device result is checked against the
host result, bit for bit.  Under each kernel row: the mean time of each kernel of one call (cc_<name>_kernel, the library's per-launch
events, which cost the launches their overlap: the sum exceeds the row above it).

    python tools/components_micro.py --out profiles/components_micro.txt --commit $(git rev-parse --short HEAD)
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
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d  # noqa: E402
from dycon_paper_replication_amd.utils import components, device_eval, sliding_window, surface_eval  # noqa: E402
from dycon_paper_replication_amd.utils import test_3d_patch as T3  # noqa: E402


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


def ball(shape, radius_fraction=0.3):
    x, y, z = np.ogrid[:shape[0], :shape[1], :shape[2]]
    c = [(n - 1) / 2 for n in shape]
    return ((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= (radius_fraction * min(shape)) ** 2).astype(np.uint8)


def speckled(mask, seed):
    return (mask | (np.random.default_rng(seed).random(mask.shape) < 0.01)).astype(np.uint8)


def host_nms(label):
    """the host path of the step: the label map to the host, getLargestCC per volume, the kept mask back to the device"""
    vols = label.cpu().numpy()
    kept = np.stack([np.asarray(T3.getLargestCC(v)).astype(np.uint8) for v in (vols if vols.ndim == 4 else vols[None])])
    return torch.from_numpy(kept if vols.ndim == 4 else kept[0]).to(label.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# components_micro  {datetime.datetime.now(datetime.timezone.utc).strftime('%Y-%m-%d %H:%M UTC')}  commit {a.commit}",
             f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; kernel rows, device: HIP events, median of {a.reps} after "
             f"{a.warmup} warm-up (min in brackets); host and end to end: synchronised wall clock, median of {a.host_reps}",
             f"{'configuration':<52}{'device ms':>20}{'host ms':>22}{'host / device':>15}"]

    def row(name, d, h):
        lines.append(f"{name:<52}{d[0]:>11.3f} ({d[1]:.3f}){h[0]:>13.1f} ({h[1]:.1f}){h[0] / d[0]:>14.1f}x")
        print(lines[-1], flush=True)

    big = (240, 240, 155)
    masks = [("ball", ball(big)), ("ball + 1 % speckle", speckled(ball(big), 0)),
             ("(4, 96, 96, 96) balls + 1 % speckle", np.stack([speckled(ball((96, 96, 96), 0.2 + 0.05 * i), i) for i in range(4)]))]
    for name, m in masks:
        t = torch.from_numpy(m).to(dev)
        got, ref = components.largest_component(t), host_nms(t)
        assert torch.equal(got, ref), name
        ncomp = components.label_components(t)[1].tolist()
        label = name if m.ndim == 4 else f"240 x 240 x 155 {name}"
        row(f"largest_component {label}", timed_events(lambda: components.largest_component(t), a.warmup, a.reps),
            timed_wall(lambda: host_nms(t), 0, a.host_reps))
        lines.append(f"    foreground {int(m.sum())} voxels, components per volume {ncomp}")
        lines.append("    kernels, ms: " + ", ".join(f"{k[3:-7]} {v:.3f}" for k, v in
                                                    kernel_breakdown(lambda: components.largest_component(t)).items()))

    # one case end to end: a noisy ball through the bf16 V-Net (random weights: the prediction is whatever the net makes of it)
    rng = np.random.default_rng(1)
    gt = ball(big)
    image = (rng.standard_normal(big) + 2.0 * gt).astype(np.float32)
    torch.manual_seed(0)
    model = net_factory_3d("vnet", 1, 2, 2, dtype=torch.bfloat16).to(dev)
    kw = dict(patch_size=(96, 96, 64), stride_xy=16, stride_z=4, batch_size=8, nms=1)
    cases = [(image, gt)]
    on_device = device_eval.test_all_case(model, cases, 2, **kw)
    on_host = surface_eval.test_all_case(model, cases, 2, device_surface=True, **kw)
    assert np.array_equal(on_device, on_host), (on_device, on_host)
    pred = sliding_window.single_case_device(model, image, 16, 4, (96, 96, 64), batch_size=8)[0]
    row("test_all_case(nms=1), one 240 x 240 x 155 case",
        timed_wall(lambda: device_eval.test_all_case(model, cases, 2, **kw), 0, a.host_reps),
        timed_wall(lambda: surface_eval.test_all_case(model, cases, 2, device_surface=True, **kw), 0, a.host_reps))
    lines.append(f"    device = device_eval.test_all_case, host = surface_eval.test_all_case(device_surface=True); prediction "
                 f"{int(pred.sum())} voxels in {components.label_components(pred)[1].item()} components; metrics {on_device.tolist()}")
    row("  the nms step of that case alone", timed_events(lambda: components.largest_component(pred), a.warmup, a.reps),
        timed_wall(lambda: host_nms(pred), 0, a.host_reps))
    lines.append("    kernels, ms: " + ", ".join(f"{k[3:-7]} {v:.3f}" for k, v in
                                                kernel_breakdown(lambda: components.largest_component(pred)).items()))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
