"""TrainConfig(use_gambling=1) on two gloo ranks sharing the one GPU of the test box (the harness of tests/test_ddp_gpu.py): both
ranks end with the same parameters, and the step matches oracle.step.ddp_train_step with the gambling term -- the student sum
r*u of each rank all-reduced with the other FeCL accumulators, gu scaled by the LOCAL B*N and averaged by the arena's 1/world."""
import os
import tempfile

import numpy as np
import pytest
import torch

from test_gambling_cpu import uncertainty_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("loss", "ce", "dice", "cons", "fecl", "uncl")


def _worker(rank, init_file, out_dir):
    import torch.distributed as dist
    from dycon_paper_replication_amd.engine import DropoutSpec
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    from oracle import nets as ON
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=2)
    torch.cuda.set_device(0)
    vol, lab, noise = make_batch(9, 4, (32, 32, 32))          # global batch [lab0, lab1 | unl0, unl1]
    idx = [rank, 2 + rank]
    off = DropoutSpec("off")
    cfg = TrainConfig(model="vnet", labeled_bs=1, batch_size=2, dtype=torch.float32, seed=5, u_weight=0.5, base_lr=0.01, use_gambling=1)
    tr = DyconTrainer(cfg, DEV, process_group=dist.group.WORLD, student_init=ON.make_vnet_params(5), teacher_init=ON.make_vnet_params(6))
    rows, g0, step0 = [], None, None
    for it in range(2):
        out = tr.step(vol[idx].to(DEV), lab[idx].to(DEV), noise=noise[idx].to(DEV), s_drop=off, t_drop=off, epoch=300, beta=2.5)
        if it == 0:
            g0 = {k: (tr.g[k] / 2).cpu() for k in tr.names}     # the arena holds the SUM over the two ranks
            step0 = {k: out[k].detach().cpu().clone() for k in ("s_logits", "s_feat", "t_feat", "mask")}
        rows.append([float(out[k]) for k in KEYS])
    torch.cuda.synchronize()
    torch.save({"p": tr.flat_p.cpu(), "t": tr.flat_t.cpu(), "rows": rows, "g0": g0, "step0": step0,
                "params": {k: tr.p[k].cpu() for k in ("block_one.conv.0.weight", "projection.3.weight", "out_conv.weight")}},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _oracle_patch(monkeypatch):
    """ddp_train_step's per-rank FeCL accumulators with the gambling weight: u from the rank's student logits (per-axis factor)"""
    from oracle import losses as L
    from oracle import nets as ON
    orig_forward = ON.forward
    last = {}

    def forward(*a, **kw):
        out = orig_forward(*a, **kw)
        if torch.is_grad_enabled():          # the student's forward (the teacher's runs under no_grad)
            last["logits"], last["feat_shape"] = out[1], tuple(out[2].shape)
        return out

    def fecl_parts(feat, mask, teacher_feat=None, epoch=0, temperature=0.6, gamma=2.0, use_focal=False, rampup_epochs=2000):
        lg = last["logits"]
        k = tuple(lg.shape[2 + a] // last["feat_shape"][2 + a] for a in range(3))
        u = uncertainty_ref(lg, k)
        tot = num_t = cnt_t = feat.new_zeros(())
        for pp, num, cnt in L._fecl_samples(feat, mask, teacher_feat, u, epoch, temperature, gamma, use_focal, rampup_epochs):
            tot, num_t, cnt_t = tot + pp.sum(), num_t + num, cnt_t + cnt
        return tot, num_t, cnt_t, feat.shape[0] * feat.shape[1]

    monkeypatch.setattr(ON, "forward", forward)
    monkeypatch.setattr(L, "fecl_parts", fecl_parts)


def test_two_rank_gambling_step_vs_ddp_oracle(monkeypatch):
    import torch.multiprocessing as mp
    from dycon_paper_replication_amd.synthetic import make_batch
    from oracle import losses as L
    from oracle import nets as ON
    from oracle import step as OS
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(os.path.join(d, "init"), d), nprocs=2, join=True)
        got = [torch.load(os.path.join(d, f"rank{r}.pt"), weights_only=False) for r in range(2)]
    # both ranks apply the same averaged update
    assert torch.equal(got[0]["p"], got[1]["p"]) and torch.equal(got[0]["t"], got[1]["t"])
    assert got[0]["rows"] == got[1]["rows"]
    # the FeCL scalar of step 0 from what the ranks returned, in fp64, under the global-batch rules: sum_r sum_i r_i u_i / (W B N)
    # + the cross numerator over the global count
    stud = num = cnt = 0.0
    rows = 0
    for g in got:
        s0 = g["step0"]
        lg = s0["s_logits"].double().permute(0, 4, 1, 2, 3)           # (B, D, H, W, 2) -> (B, 2, D, H, W)
        sf = s0["s_feat"].double()
        k = tuple(lg.shape[2 + a] // sf.shape[1 + a] for a in range(3))
        u = uncertainty_ref(lg, k)
        f = torch.nn.functional.normalize(sf.reshape(sf.shape[0], -1, sf.shape[-1]), dim=-1)
        t = torch.nn.functional.normalize(s0["t_feat"].double().reshape(f.shape[0], -1, f.shape[-1]), dim=-1)
        for pp, n_, c_ in L._fecl_samples(f, s0["mask"].double(), t, u, 300, 0.6, 2.0, True, 1500):
            stud, num, cnt = stud + float(pp.sum()), num + float(n_), cnt + float(c_)
        rows += f.shape[0] * f.shape[1]
    fecl64 = stud / rows + (num / (cnt + 1e-18) if cnt > 0 else 0.0)
    assert got[0]["rows"][0][4] == pytest.approx(fecl64, rel=1e-4)
    # the whole step against the CPU emulation of the data-parallel step, in fp64
    _oracle_patch(monkeypatch)
    dbl = lambda p: {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}  # noqa: E731
    states = [OS.StepState(student=dbl(ON.make_vnet_params(5)), teacher=dbl(ON.make_vnet_params(6))) for _ in range(2)]
    cfg = OS.StepConfig(net_type="vnet", labeled_bs=1, u_weight=0.5, base_lr=0.02)
    vol, lab, noise = make_batch(9, 4, (32, 32, 32))
    shards = [(vol[[r, 2 + r]].double(), lab[[r, 2 + r]], noise[[r, 2 + r]].double()) for r in range(2)]
    for step in range(2):
        ref = OS.ddp_train_step(cfg, states, shards, 2.5, 300)
        exp = np.array([float(ref[k]) for k in KEYS])
        np.testing.assert_allclose(np.array(got[0]["rows"][step]), exp, rtol=1e-4, atol=1e-6, err_msg=f"step {step}")
        if step == 0:
            gh = torch.cat([got[0]["g0"][k].double().reshape(-1) for k in ref["grads"]])
            gr = torch.cat([ref["grads"][k].reshape(-1) for k in ref["grads"]])
            assert float((gh * gr).sum() / (gh.norm() * gr.norm())) >= 0.9999
            k = "out_conv.weight"          # the segmentation head: where the u path's gradient lands first
            assert float((got[0]["g0"][k].double() - ref["grads"][k]).norm()) <= 1e-3 * float(ref["grads"][k].norm())
    for k, v in got[0]["params"].items():
        ref_p = states[0].student[k].numpy()
        np.testing.assert_allclose(v.numpy(), ref_p, rtol=1e-4, atol=1e-4 * float(np.abs(ref_p).max()), err_msg=k)
