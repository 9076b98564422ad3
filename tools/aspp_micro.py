"""Time the ASPP's nine-tap branch (aspp2, d = 6, on the 7 x 7 x 5 bottleneck of a 112 x 112 x 80 patch, B = 4, 256 -> 256) as the
package runs it (aspp.dilated_conv3d*: live-tap gather + MFMA GEMM, weight gradient through the dense GEMM + unpack) against torch's
own F.conv3d(dilation=6, padding=6) on the GPU, forward, data gradient and weight gradient; bf16 and fp32 storage.

    python tools/aspp_micro.py [--reps 50] [--out profiles/aspp_micro.txt]

HIP events around each call after warm-up, median of --reps.  The package's weight pack (pack_wblocks) is included in its forward and
data-gradient times; the step packs once per parameter update instead.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dycon_paper_replication_amd.aspp import dilated_conv3d, dilated_conv3d_bwd_data, dilated_conv3d_bwd_weight  # noqa: E402


def med_ms(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "aspp_micro.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    B, C, dhw, d = 4, 256, (7, 7, 5), 6
    lines = [f"aspp2 branch: B={B}, {C}->{C}, grid {dhw}, dilation {d} (9 live taps of 27); median of {args.reps}, ms"]
    for dtype in (torch.bfloat16, torch.float32):
        x = torch.randn((B, C) + dhw, device=dev).to(dtype)
        w = torch.randn((C, C, 3, 3, 3), device=dev) * (2.0 / (27 * C)) ** 0.5
        gy = torch.randn((B, C) + dhw, device=dev).to(dtype)
        xl, gyl = x.permute(0, 2, 3, 4, 1).contiguous(), gy.permute(0, 2, 3, 4, 1).contiguous()
        wt = w.to(dtype)
        gw = torch.empty_like(w)
        ours = [med_ms(lambda: dilated_conv3d(xl, w, d), args.reps),
                med_ms(lambda: dilated_conv3d_bwd_data(gyl, w, d), args.reps),
                med_ms(lambda: dilated_conv3d_bwd_weight(xl, gyl, d, gw), args.reps)]
        ref = [med_ms(lambda: F.conv3d(x, wt, padding=d, dilation=d), args.reps),
               med_ms(lambda: torch.nn.grad.conv3d_input(x.shape, wt, gy, padding=d, dilation=d), args.reps),
               med_ms(lambda: torch.nn.grad.conv3d_weight(x, wt.shape, gy, padding=d, dilation=d), args.reps)]
        for what, o, r in zip(("forward", "data gradient", "weight gradient"), ours, ref):
            lines.append(f"{str(dtype)[6:]:9s} {what:16s} package {o:8.4f}   torch F.conv3d {r:8.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
