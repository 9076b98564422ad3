"""Time ops.similarity_histograms (dycon_simhist: Gram tiles recomputed on MFMA, binned on chip) against a torch restatement of the
device-side work of the reference monitor (code/utils/monitor.py:15-33: the (B, N, N) similarity matrix, two float pair masks,
boolean indexing, then the copies to the host for np.histogram).

    python tools/simhist_micro.py [--reps 30] [--torch-reps 3] [--out profiles/simhist_micro.txt]

The op: HIP events around each call, after warm-up; the median of --reps calls.  Its FLOPs: 2 sweeps x 2*B*N^2*Dm / 2 (the tile
pairs j >= i only), against the MFMA peak of the storage type.  The torch path: a host clock around the whole of it, ending in the
D2H copies (which synchronise), median of --torch-reps; its peak extra device memory as the max_memory_allocated delta.
"""
import argparse
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dycon_paper_replication_amd import ops  # noqa: E402

SHAPES = [("96^3 headline", 2, 1728, 256), ("Pancreas", 2, 2352, 256), ("ISLES", 2, 15680, 256)]
PEAK_TF = {torch.bfloat16: 2500.0, torch.float32: 157.3}      # dense MFMA peaks (spec)


def torch_reference(feat, mask, tau=0.6):
    mem = torch.eq(mask, mask.transpose(1, 2)).float()
    neg = 1 - mem
    fn = F.normalize(feat, dim=-1)
    sim = torch.matmul(fn, fn.transpose(1, 2)) / tau
    return sim[mem.bool()].cpu(), sim[neg.bool()].cpu()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"# simhist_micro: {torch.cuda.get_device_name(0)}, op median of {a.reps} (HIP events), torch median of {a.torch_reps}",
             "# shape                      dtype  op_ms   GramTF  %peak   torch_ms   torch_extra_MB  op_extra_MB"]
    for name, B, N, Dm in SHAPES:
        for dtype in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=dev).manual_seed(N)
            feat = torch.randn(B, N, Dm, device=dev, generator=g).to(dtype)
            mask = (torch.rand(B, 1, N, device=dev, generator=g) < 0.3).float()
            for _ in range(3):
                ops.similarity_histograms(feat, mask)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)]
            for e0, e1 in ev:
                e0.record()
                ops.similarity_histograms(feat, mask)
                e1.record()
            torch.cuda.synchronize()
            op_extra = (torch.cuda.max_memory_allocated() - base) / 2**20
            ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)[len(ev) // 2]
            flops = 2 * 2.0 * B * N * N * Dm / 2
            tf = flops / ms / 1e9
            tms, textra = [], 0.0
            for _ in range(a.torch_reps):
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                t0 = time.perf_counter()
                p, n = torch_reference(feat, mask)
                torch.cuda.synchronize()
                tms.append((time.perf_counter() - t0) * 1e3)
                textra = max(textra, (torch.cuda.max_memory_allocated() - base) / 2**20)
                del p, n
            tm = sorted(tms)[len(tms) // 2]
            line = (f"{name:>14} B={B} N={N:>5} Dm={Dm}  {str(dtype)[6:]:>8} {ms:7.3f} {tf:8.1f} {100 * tf / PEAK_TF[dtype]:6.2f}  "
                    f"{tm:9.1f} {textra:15.0f} {op_extra:12.2f}")
            print(line, flush=True)
            lines.append(line)
            del feat, mask
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
