"""Time the fused up-sampling convolution (ops.upconv_k3: trilinear x2 folded into the k=3 convolution's operand staging) against the
composition it replaces (ops.trilinear_fwd -> ops.conv_gemm, which writes and re-reads the up-sampled tensor), forward, bf16, B = 4,
at the three decoder levels of a 96^3 patch.

    python tools/upconv_micro.py [--reps 50] [--out profiles/upconv_micro.txt]

HIP events around 20 back-to-back calls of each form after warm-up, per-call time, median of --reps; the weights are packed once outside the timed region (both forms take
the same operand).  Algorithmic bytes: fused = low-resolution read + output write + weights; composition = that + one write and
one read of the up-sampled tensor (8 x the input).
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dycon_paper_replication_amd import ops  # noqa: E402
from dycon_paper_replication_amd._lib import CONV_K3  # noqa: E402

SHAPES = [(48, 32, 16), (24, 64, 32), (6, 256, 128)]      # low-resolution edge, Cin, Cout


INNER = 20      # calls enqueued between the two events: at 6^3 a call is microseconds, one call per region would time the launch path


def med_ms(fn, reps):
    for _ in range(5):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / INNER)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "upconv_micro.txt"))
    args = ap.parse_args()
    dev, B, dtype = "cuda:0", 4, torch.bfloat16
    lines = [f"Upsampling forward (trilinear x2 -> conv k3), bf16, B={B}; ms per call ({INNER} calls per timed region, median of {args.reps}); MB = algorithmic bytes"]
    for n, Cin, Cout in SHAPES:
        x = torch.randn((B, n, n, n, Cin), device=dev).to(dtype)
        w = torch.randn((Cout, Cin, 3, 3, 3), device=dev) * (2.0 / (27 * Cin)) ** 0.5
        bias = torch.zeros(Cout, device=dev)
        wf = ops.pack_bfrag(w, dtype, 27, Cin, Cout, Cout, 1, 27, 0, Cin * 27)
        y = torch.empty((B, 2 * n, 2 * n, 2 * n, Cout), device=dev, dtype=dtype)
        up = torch.empty((B, 2 * n, 2 * n, 2 * n, Cin), device=dev, dtype=dtype)

        def comp():
            ops.trilinear_fwd(x, (2 * n, 2 * n, 2 * n), False, out=up)
            ops.conv_gemm(up, wf, bias, CONV_K3, Cout, Cout, out=y)

        t_res = med_ms(lambda: ops.trilinear_fwd(x, (2 * n, 2 * n, 2 * n), False, out=up), args.reps)
        t_comp = med_ms(comp, args.reps)
        t_fused = med_ms(lambda: ops.upconv_k3(x, wf, bias, Cout, out=y), args.reps)
        mb_f = (x.numel() + y.numel() + 27 * Cin * Cout) * 2 / 1e6
        mb_c = mb_f + 2 * up.numel() * 2 / 1e6
        lines.append(f"{n}^3 -> {2 * n}^3, {Cin:3d} -> {Cout:3d}: fused {t_fused:8.4f} ({mb_f:7.1f} MB)   "
                     f"resize + conv {t_comp:8.4f} ({mb_c:7.1f} MB; the resize alone {t_res:8.4f})   fused / composition {t_fused / t_comp:5.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
