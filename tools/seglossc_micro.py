"""Time the C-class one-pass voxel losses (ops.seg_lossesc_fwd + step_lossesc + seg_lossesc_bwd, fast sequences as the bf16 step
runs them) against the composition they replace in a training loop -- nn.CrossEntropyLoss + torch softmax + the package's
reference-semantics callables losses.DiceLoss(C), losses.softmax_mse_loss(...).mean() and dycon_losses.UnCLoss, forward and
autograd backward -- on (4, C, 96, 96, 96) logits with 2 labelled samples, C in {3, 4, 8}; the 2-class pass is listed for scale.

    python tools/seglossc_micro.py [--reps 50] [--out profiles/seglossc_micro.txt]

HIP events around 20 back-to-back calls of each form after warm-up, per-call time, median of --reps (as tools/headc_micro.py).
No threshold: the step needs one launch path per class count; the ratio is reported.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dycon_paper_replication_amd import ops  # noqa: E402
from dycon_paper_replication_amd.utils import dycon_losses, losses  # noqa: E402

SHAPE, B, LB, BETA = (96, 96, 96), 4, 2, 2.5
CLASSES = [3, 4, 8]
INNER = 20


def med_ms(fn, reps, inner=INNER):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "seglossc_micro.txt"))
    args = ap.parse_args()
    dev = "cuda:0"
    V = SHAPE[0] * SHAPE[1] * SHAPE[2]
    lines = [f"one-pass voxel losses, fast sequences, logits ({B}, C, {SHAPE[0]}, {SHAPE[1]}, {SHAPE[2]}) fp32 channels-last, LB={LB}, mse "
             f"consistency, multi-class Dice; ms per call ({INNER} calls per timed region, median of {args.reps}; composition: 4 calls, "
             f"median of {max(args.reps // 5, 5)})"]
    coef = torch.tensor([1.0, 0.0, 1.0, 0.1, 0.5], device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for C in [2] + CLASSES:
        gen = torch.Generator(device=dev).manual_seed(C)
        s = torch.randn((B,) + SHAPE + (C,), device=dev, generator=gen) * 2.0
        t = s + 0.3 * torch.randn((B,) + SHAPE + (C,), device=dev, generator=gen)
        lab = torch.randint(0, C, (B,) + SHAPE, device=dev, generator=gen).to(torch.uint8)
        sums = torch.zeros(16 if C == 2 else ops.seg_lossesc_nsums(C), dtype=torch.float64, device=dev)

        if C == 2:
            def fwd():
                ops.seg_losses_fwd(s, t, lab, LB, BETA, fast=True, out=sums)
                ops.step_losses(sums, None, B, LB, V, BETA, 1.0, 1.0, False, 1.0, 0.1, 0.5, 1, 0, flag)

            def bwd():
                ops.seg_losses_bwd(s, t, lab, LB, BETA, sums, coef, 0, fast=True)
        else:
            def fwd():
                ops.seg_lossesc_fwd(s, t, lab, LB, BETA, 0, fast=True, out=sums)
                ops.step_lossesc(sums, None, B, LB, V, C, BETA, 1.0, 1.0, False, 1.0, 0.1, 0.5, 1, 0, flag)

            def bwd():
                ops.seg_lossesc_bwd(s, t, lab, LB, BETA, sums, coef, 0, fast=True)

        tf, tb = med_ms(fwd, args.reps), med_ms(bwd, args.reps)
        row = f"C={C}:  fused forward {tf:7.4f}  backward {tb:7.4f}  both {tf + tb:7.4f}"
        if C != 2:
            sl = s.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)       # (B, C, D, H, W) view, as the nets return their logits
            tl = t.permute(0, 4, 1, 2, 3)
            labl = lab.long()
            ce, dice, uncl = torch.nn.CrossEntropyLoss(), losses.DiceLoss(C), dycon_losses.UnCLoss()

            def comp():
                sp, tp = torch.softmax(sl, 1), torch.softmax(tl, 1)
                total = ce(sl[:LB], labl[:LB]) + dice(sp[:LB], labl[:LB].unsqueeze(1)) \
                    + 0.1 * losses.softmax_mse_loss(sp[LB:], tp[LB:]).mean() + 0.5 * uncl(sl, tl, BETA)
                sl.grad = None
                total.backward()

            tc = med_ms(comp, max(args.reps // 5, 5), inner=4)
            row += f"   |   composition forward + backward {tc:8.4f}   fused / composition {(tf + tb) / tc:5.3f}"
            del sl, tl, labl
        lines.append(row)
        del s, t, lab
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
