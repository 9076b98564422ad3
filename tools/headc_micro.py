"""Time the C-class head fused into block_nine's normalisation (ops.norm_head_fwd / norm_head_bwd + norm_head_dparams) against the
composition it replaces -- ops.norm_apply + ops.conv_direct forward; ops.conv_direct's data gradient + ops.norm_bwd + ops.conv_wgrad
backward -- which writes and re-reads the normalised 16-channel tensor and its gradient.  bf16, B = 4, the two training patches,
C in {2, 3, 4, 8}; the statistics launch (the same in both forms) is outside the timed regions.

    python tools/headc_micro.py [--reps 50] [--out profiles/headc_micro.txt]

HIP events around 20 back-to-back calls of each form after warm-up, per-call time, median of --reps (as tools/upconv_micro.py).
Engine._norm_head takes the fused kernels for a class count only where they are the faster form here.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dycon_paper_replication_amd import ops  # noqa: E402
from dycon_paper_replication_amd._lib import CONV_1X1  # noqa: E402

SHAPES = [(96, 96, 96), (112, 112, 80)]
CLASSES = [2, 3, 4, 8]
INNER = 20


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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "headc_micro.txt"))
    args = ap.parse_args()
    dev, B, dtype, C, G = "cuda:0", 4, torch.bfloat16, 16, 16
    lines = [f"block_nine norm + ReLU + C-class head, bf16, B={B}, GroupNorm(16, 16); ms per call ({INNER} calls per timed region, "
             f"median of {args.reps}); fused = norm_head_*, composition = norm_apply + conv_direct | conv_direct + norm_bwd + conv_wgrad"]
    for sp in SHAPES:
        V = sp[0] * sp[1] * sp[2]
        x = (torch.randn((B,) + sp + (C,), device=dev) * 1.5 + 0.3).to(dtype)
        gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.3
        stats = ops.norm_stats(x, B, V, C, G)
        y, gy, gx = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
        for K in CLASSES:
            W = torch.randn((K, C, 1, 1, 1), device=dev) * 0.4
            hb = torch.randn(K, device=dev)
            w_fwd, w_bwd = W.reshape(K, C).t().contiguous(), W.reshape(K, C).contiguous()
            gl = torch.randn((B,) + sp + (K,), device=dev)
            logits = torch.empty((B,) + sp + (K,), device=dev)
            gw, gb = torch.empty_like(W), torch.empty_like(hb)
            ws = ops.conv_wgrad_workspace(y, gl, CONV_1X1)

            def comp_fwd():
                ops.norm_apply(x, stats, B, V, C, G, gamma, beta, True, None, y)
                ops.conv_direct(y, w_fwd, hb, CONV_1X1, K, torch.float32, out=logits)

            def comp_bwd():
                ops.conv_direct(gl, w_bwd, None, CONV_1X1, C, dtype, out=gy)
                ops.norm_bwd(x, False, gy, stats, B, V, C, G, gamma, beta, True, dg, db, out=gx)
                ops.conv_wgrad(y, gl, gw, CONV_1X1, 0, 1, C, dbias=gb, ws=ws)

            def fused_fwd():
                ops.norm_head_fwd(x, stats, B, V, G, W, hb, gamma, beta, True)

            def fused_bwd():
                _, pend = ops.norm_head_bwd(x, gl, stats, B, V, G, W, gamma, beta, True, dg, db)
                ops.norm_head_dparams(pend, gw, gb)

            comp_fwd()      # y for the composition's weight gradient
            tf, tcf = med_ms(fused_fwd, args.reps), med_ms(comp_fwd, args.reps)
            tb, tcb = med_ms(fused_bwd, args.reps), med_ms(comp_bwd, args.reps)
            lines.append(f"{sp[0]}x{sp[1]}x{sp[2]}  C={K}:  forward fused {tf:7.4f}  composition {tcf:7.4f}  ratio {tf / tcf:5.2f}   |   "
                         f"backward fused {tb:7.4f}  composition {tcb:7.4f}  ratio {tb / tcb:5.2f}   |   "
                         f"both {tf + tb:7.4f} vs {tcf + tcb:7.4f}  ratio {(tf + tb) / (tcf + tcb):5.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
