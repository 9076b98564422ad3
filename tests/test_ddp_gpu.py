"""GPU, 2 ranks sharing the one GPU of the test box (gloo rendezvous; RCCL refuses duplicate devices): the sharded DyCON step --
bucketed gradient all-reduce overlapped with the backward, all-reduced Dice / FeCL accumulators, x world pre-scaling, 1/world folded
into the SGD kernel.

* u_weight = 0: equals the single-process HIP step on the global batch (no per-rank BatchNorm in play).
* u_weight = 0.5 (FeCL + UnCL ON, the default): against oracle.step.ddp_train_step, the CPU emulation in which every rank forwards
  its own shard (per-rank BatchNorm statistics in the projection head, as the reference's DataParallel replicas) and the 16 + 4
  accumulators are summed over ranks -- exercises fecl_finalize(rows = B*world*N) and the x world cross-branch gradient.
* replay == eager under a process group (the recorded step contains the collectives).
* RCCL itself (backend "nccl"), with the ONE rank a single-GPU box allows: TrainConfig.ddp_force runs the whole exchange -- bucketed
  async all-reduces issued from inside the backward, the fp64 accumulator exchange, the joins -- through RCCL, eager and replayed;
  every collective is then the identity, so the run must reproduce the plain single-GPU run."""
import os
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("loss", "ce", "dice", "cons", "fecl", "uncl")


def _cfg(u_weight=0.0, dtype=torch.float32, replay=True):
    from dycon_paper_replication_amd.trainer import TrainConfig
    return TrainConfig(model="vnet", labeled_bs=1, batch_size=2, dtype=dtype, seed=5, u_weight=u_weight, base_lr=0.01, replay=replay)


def _worker(rank, init_file, out_file, mode):
    import torch.distributed as dist
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer
    from oracle import nets as ON
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    vol, lab, noise = make_batch(9, 4, (32, 32, 32))          # global batch [lab0, lab1 | unl0, unl1]
    idx = [rank, 2 + rank]
    off = DropoutSpec("off")
    res = {}
    if mode in ("global", "fecl"):
        init = dict(student_init=ON.make_vnet_params(5), teacher_init=ON.make_vnet_params(6)) if mode == "fecl" else {}
        tr = DyconTrainer(_cfg(0.5 if mode == "fecl" else 0.0), DEV, process_group=dist.group.WORLD, **init)
        assert len(tr.buckets) >= 2
        rows, g0 = [], None
        for it in range(2):
            out = tr.step(vol[idx].to(DEV), lab[idx].to(DEV), noise=noise[idx].to(DEV), s_drop=off, t_drop=off, epoch=300, beta=2.5)
            if it == 0 and mode == "fecl":
                g0 = {k: (tr.g[k] / 2).cpu() for k in tr.names}     # the arena holds the SUM over the two ranks
            # grad_sumsq is taken over the all-reduced arena, which holds the SUM over ranks (1/world is folded into the SGD kernel)
            rows.append([float(out[k]) for k in KEYS] + [float(out["grad_sumsq"].sqrt()) / 2])
        res = {"p": tr.flat_p.cpu(), "t": tr.flat_t.cpu(), "rows": rows, "names": tr.names, "g0": g0,
               "params": {k: tr.p[k].cpu() for k in ("block_one.conv.0.weight", "block_five.conv.3.weight", "projection.3.weight",
                                                     "projection.0.weight", "out_conv.weight")}}
    else:   # replay vs eager, bf16, on-device Philox randomness, changing batches
        batches = [make_batch(500 + i, 4, (32, 32, 32)) for i in range(7)]
        for replay in (False, True):
            tr = DyconTrainer(_cfg(0.5, torch.bfloat16, replay), DEV, process_group=dist.group.WORLD)
            losses = []
            for v, l, _ in batches:
                out = tr.step(v[idx].to(DEV), l[idx].to(DEV))
                losses.append([float(out[k]) for k in KEYS])
            assert (tr._rp is not None) == replay and tr.iter_num == 7
            res[replay] = (np.array(losses), tr.flat_p.cpu(), tr.flat_t.cpu())
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(res, out_file)
    dist.barrier()
    dist.destroy_process_group()


def _run(mode):
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        init_file, out_file = os.path.join(d, "init"), os.path.join(d, "out.pt")
        mp.spawn(_worker, args=(init_file, out_file, mode), nprocs=2, join=True)
        return torch.load(out_file, weights_only=False)


def test_two_rank_step_equals_global_batch_step():
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer
    got = _run("global")
    cfg = _cfg()
    cfg.labeled_bs, cfg.batch_size = 2, 4
    cfg.base_lr = 0.02            # the 2-rank run scales LR x world (train_DyCON_BraTS19.py:108-110)
    tr = DyconTrainer(cfg, DEV)
    vol, lab, noise = make_batch(9, 4, (32, 32, 32))
    off = DropoutSpec("off")
    for _ in range(2):
        out = tr.step(vol.to(DEV), lab.to(DEV), noise=noise.to(DEV), s_drop=off, t_drop=off, epoch=300, beta=2.5)
    assert got["rows"][-1][0] == pytest.approx(float(out["loss"]), rel=1e-4)
    assert got["rows"][-1][2] == pytest.approx(float(out["dice"]), rel=1e-4)
    np.testing.assert_allclose(got["p"].numpy(), tr.flat_p.cpu().numpy(), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(got["t"].numpy(), tr.flat_t.cpu().numpy(), rtol=2e-4, atol=2e-6)


def test_two_rank_step_with_fecl_vs_ddp_oracle():
    """FeCL / UnCL on (u_weight = 0.5): the all_reduce of the FeCL accumulators, fecl_finalize with world > 1 and the x world
    scaling of the cross-branch gradient, against the CPU emulation of the data-parallel step (run in DOUBLE: the true values)."""
    from dycon_paper_replication_amd.synthetic import make_batch
    from oracle import nets as ON
    from oracle import step as OS
    got = _run("fecl")
    dbl = lambda p: {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}  # noqa: E731
    states = [OS.StepState(student=dbl(ON.make_vnet_params(5)), teacher=dbl(ON.make_vnet_params(6))) for _ in range(2)]
    states32 = [OS.StepState(student=ON.make_vnet_params(5), teacher=ON.make_vnet_params(6)) for _ in range(2)]
    cfg = OS.StepConfig(net_type="vnet", labeled_bs=1, u_weight=0.5, base_lr=0.02)
    vol, lab, noise = make_batch(9, 4, (32, 32, 32))
    shards32 = [(vol[[r, 2 + r]], lab[[r, 2 + r]], noise[[r, 2 + r]]) for r in range(2)]
    shards = [(v.double(), l, n.double()) for v, l, n in shards32]
    for step in range(2):
        ref = OS.ddp_train_step(cfg, states, shards, 2.5, 300)
        ref32 = OS.ddp_train_step(cfg, states32, shards32, 2.5, 300)
        exp = np.array([float(ref[k]) for k in KEYS] + [float(ref["grad_norm"])])
        exp32 = np.array([float(ref32[k]) for k in KEYS] + [float(ref32["grad_norm"])])
        # loss terms: the north-star's 1e-4.  Gradient norm: 5e-4 -- ReLU decisions of voxels whose pre-activation is within fp32
        # round-off of zero differ between any two fp32 implementations, and a flipped voxel changes its whole gradient
        # (tools/bwd_bisect.py: ONE voxel at -2e-6 explains a 1e-2 difference of the deep-layer gradients of this very batch; the
        # reference's own fp32 run is 1.2e-4 off its fp64 twin on this quantity in step_unet.npz).
        got_row = np.array(got["rows"][step])
        np.testing.assert_allclose(got_row[:6], exp[:6], rtol=1e-4, atol=1e-6, err_msg=f"step {step}")
        assert abs(got_row[6] - exp[6]) <= max(5e-4 * exp[6], 2 * abs(exp32[6] - exp[6])), (step, got_row[6], exp[6], exp32[6])
        if step == 0:                # the averaged gradient itself, parameter by parameter, against the double run
            worst_h = worst_r = 0.0
            gh = torch.cat([got["g0"][k].double().reshape(-1) for k in ref["grads"]])
            gr = torch.cat([ref["grads"][k].reshape(-1) for k in ref["grads"]])
            cos = float((gh * gr).sum() / (gh.norm() * gr.norm()))
            for k, g64 in ref["grads"].items():
                assert bool(torch.isfinite(got["g0"][k]).all()), f"{k}: averaged gradient holds NaN / Inf"   # (max() keeps 0.0 over a NaN)
                nrm = float(g64.norm()) + 1e-30
                if nrm > 1e-6 * float(ref["grad_norm"]):      # (analytically zero gradients hold round-off only)
                    worst_h = max(worst_h, float((got["g0"][k].double() - g64).norm()) / nrm)
                    worst_r = max(worst_r, float((ref32["grads"][k].double() - g64).norm()) / nrm)
            print(f"averaged gradient: cos {cos:.8f}; worst per-parameter relative L2 error: hip {worst_h:.3e}, fp32 emulation {worst_r:.3e}")
            assert cos >= 0.9999 and worst_h <= 3e-2, (cos, worst_h)       # ReLU flips (see above): isolated voxels, direction intact
        assert exp[4] > 0.1          # FeCL really is in play
    for k, v in got["params"].items():
        ref_p = states[0].student[k].numpy()
        np.testing.assert_allclose(v.numpy(), ref_p, rtol=1e-4, atol=1e-4 * float(np.abs(ref_p).max()), err_msg=k)


def test_two_rank_replay_equals_eager():
    got = _run("replay")
    np.testing.assert_allclose(got[True][0], got[False][0], rtol=1e-5, atol=1e-6)
    for a, b in zip(got[True][1:], got[False][1:]):
        assert float((a - b).abs().max()) <= 1e-6 * float(b.abs().max())


def _rccl_worker(rank, init_file, out_file):
    import torch.distributed as dist
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{init_file}", rank=0, world_size=1)
    batches = [make_batch(700 + i, 4, (32, 32, 32)) for i in range(7)]
    res = {}
    for tag, kw, pg in (("plain", {}, None), ("rccl_eager", dict(ddp_force=True, replay=False), dist.group.WORLD),
                        ("rccl_replay", dict(ddp_force=True, replay=True), dist.group.WORLD)):
        tr = DyconTrainer(TrainConfig(model="vnet", labeled_bs=2, batch_size=4, dtype=torch.bfloat16, seed=5, base_lr=0.01, **kw), DEV,
                          process_group=pg)
        assert (len(tr.buckets) >= 2) == (pg is not None)
        losses = []
        for v, l, _ in batches:
            out = tr.step(v.to(DEV), l.to(DEV))
            losses.append([float(out[k]) for k in KEYS])
        if tag == "rccl_replay":
            assert tr._rp is not None
        res[tag] = (np.array(losses), tr.flat_p.cpu(), tr.flat_t.cpu())
    torch.cuda.synchronize()
    torch.save(res, out_file)
    dist.destroy_process_group()


def test_rccl_one_rank_exchange_equals_plain_step():
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        init_file, out_file = os.path.join(d, "init"), os.path.join(d, "out.pt")
        mp.spawn(_rccl_worker, args=(init_file, out_file), nprocs=1, join=True)
        res = torch.load(out_file, weights_only=False)
    ref = res["plain"]
    for tag in ("rccl_eager", "rccl_replay"):
        got = res[tag]
        # same kernels, same order; only the FeCL / voxel-loss scalars are finalised by the exchange path's kernels
        np.testing.assert_allclose(got[0], ref[0], rtol=2e-5, atol=1e-6, err_msg=tag)
        for a, b, what in ((got[1], ref[1], "student"), (got[2], ref[2], "teacher")):
            err = float((a - b).abs().max())
            assert err <= 1e-5 * float(b.abs().max()), (tag, what, err)
    assert torch.equal(res["rccl_eager"][1], res["rccl_replay"][1])
