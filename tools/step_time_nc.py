"""Step time of DyconTrainer for a class count next to the 2-class step of the same run: V-Net, bf16, B = 4 (2 labelled) of 96^3,
replayed steps, on-device Philox randomness.

    python tools/step_time_nc.py [--classes 3] [--steps 40] [--warmup 10] [--out profiles/step_time_nc.txt]

Three rounds, alternating between the class counts; each measurement is a fresh child process with ONE trainer (a second trainer in
the same process doubles the streams, which then share the hardware queues: every kernel of it ran ~3x slower).  A child runs
`--warmup` steps (two eager, one recorded, the rest replayed), then times `--steps` steps between two device synchronisations.
"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(C, steps, warmup):
    import torch
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    dev = "cuda:0"
    vol, lab, _ = make_batch(3, 4, (96, 96, 96))
    vol, lab = vol.to(dev), lab.to(dev)
    if C != 2:        # three label values
        lab = torch.where((lab == 0) & (vol[:, 0] > 1.0), torch.full_like(lab, 2), lab)
    tr = DyconTrainer(TrainConfig(model="vnet", num_classes=C, batch_size=4, labeled_bs=2, dtype=torch.bfloat16, seed=3,
                                  dice_variant="fg" if C == 2 else "multiclass"), dev)
    for _ in range(warmup):
        tr.step(vol, lab)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = tr.step(vol, lab)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    assert tr.skipped_steps == 0 and tr._rp is not None
    print(f"STEP_MS {ms:.4f} loss {float(out['loss']):.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--child", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_time_nc.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.warmup)
    ts = {2: [], args.classes: []}
    for _ in range(3):
        for C in ts:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(C), "--steps", str(args.steps), "--warmup",
                                str(args.warmup)], capture_output=True, text=True, timeout=120, check=True)
            ts[C].append(float(r.stdout.split("STEP_MS")[1].split()[0]))
    lines = [f"DyconTrainer step, V-Net, bf16, B=4 (LB=2), 96x96x96, replay; ms per step over {args.steps} steps, three rounds alternating, "
             f"one process per measurement"]
    for C, t in ts.items():
        lines.append(f"num_classes={C}:  " + "  ".join(f"{v:6.3f}" for v in t) + f"   median {sorted(t)[1]:6.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
