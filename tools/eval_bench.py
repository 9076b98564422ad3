"""Sliding-window evaluation throughput: one BraTS-sized volume (240 x 240 x 155, z-scored noise), the reference's test
settings (patch 96 x 96 x 64, stride_xy 16, stride_z 4: code/test_BraTS19.py) through the bf16 V-Net.
usage: eval_bench.py [batch] [classes]

classes (default 2) > 2 times, on one model and volume in alternating runs, the class-1 evaluator (utils.test_3d_patch.test_single_case)
and the all-class evaluator (utils.eval_classes.test_single_case_classes), and then one accumulate launch of each kind on a chunk of
`batch` windows."""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])
from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
from dycon_paper_replication_amd.utils import test_3d_patch as T3

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 8
classes = int(sys.argv[2]) if len(sys.argv) > 2 else 2
shape, patch = (240, 240, 155), (96, 96, 64)
img = np.random.default_rng(0).standard_normal(shape).astype(np.float32)
model = net_factory_3d("vnet", 1, classes, 2, dtype=torch.bfloat16).cuda()
nwin = len(T3._windows(shape, patch, 16, 4))


def timed(fn, volume):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(volume)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def class1(volume):
    return T3.test_single_case(model, volume, 16, 4, patch, num_classes=classes, batch_size=batch)


if classes == 2:
    class1(img[:96, :96, :64])   # warm-up (weight packs, allocator)
    dt = timed(class1, img)
    print(f"sliding-window eval, vnet bf16, {shape} volume, {nwin} windows of {patch}, batch {batch}: {dt:.2f} s/volume, {nwin / dt:.0f} windows/s")
    sys.exit(0)

import ctypes  # noqa: E402

from dycon_paper_replication_amd import _lib  # noqa: E402
from dycon_paper_replication_amd.utils import eval_classes as EC  # noqa: E402


def allclass(volume):
    return EC.test_single_case_classes(model, volume, 16, 4, patch, batch_size=batch)


runs = {"class-1 test_single_case": class1, "all-class test_single_case_classes": allclass}
for fn in runs.values():
    fn(img[:96, :96, :64])       # warm-up (weight packs, allocator)
times = {k: [] for k in runs}
for _ in range(2):
    for k, fn in runs.items():
        times[k].append(timed(fn, img))
        print(f"  run: {k} {times[k][-1]:.2f} s", flush=True)
print(f"sliding-window eval, vnet bf16, {classes} classes, {shape} volume, {nwin} windows of {patch}, batch {batch}")
for k, v in times.items():
    print(f"  {k}: {min(v):.2f} s/volume (runs {', '.join('%.2f' % t for t in v)}), {nwin / min(v):.0f} windows/s")
a, b = (min(v) for v in times.values())
print(f"  all-class / class-1 = {b / a:.3f}")

# one accumulate launch of each kind on the first chunk's windows (device events around 20 launches)
wins = T3._windows(shape, patch, 16, 4)[:batch]
lg = torch.randn((len(wins),) + patch + (classes,), device="cuda")
org = torch.tensor(wins, dtype=torch.int32, device="cuda")
score = torch.zeros((classes,) + shape, device="cuda")
cnt = torch.zeros(shape, device="cuda")
lo, hi = EC.chunk_box(wins, patch)
int3 = ctypes.c_int * 3
stream = torch.cuda.current_stream().cuda_stream
launches = {
    "dycon_sw_accumulate_c": lambda: _lib.call("dycon_sw_accumulate_c", lg.data_ptr(), classes, len(wins), *patch, org.data_ptr(),
                                               score.data_ptr(), cnt.data_ptr(), *shape, stream),
    "dycon_sw_accumulate_all": lambda: _lib.call("dycon_sw_accumulate_all", lg.data_ptr(), classes, len(wins), *patch, org.data_ptr(),
                                                 score.data_ptr(), cnt.data_ptr(), *shape, int3(*lo), int3(*hi), stream),
}
for k, fn in launches.items():
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"  {k}: {e0.elapsed_time(e1) / 20 * 1e3:.1f} us per launch ({len(wins)} windows, box {lo}..{hi})")
