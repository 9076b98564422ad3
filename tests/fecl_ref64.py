"""FeCL in float64 with explicit pair weights, and clustered inputs for it.  Test infrastructure only.

fecl_pairs64 restates oracle/losses.py::_fecl_samples / fecl (FeCLoss.forward, utils/dycon_losses.py:150-235) WITHOUT autograd:
the derivative of the loss with respect to every logit L_ij is written out, so that next to the gradient the same contraction can be
taken over the absolute values of its terms (`absgrad`), the scale against which a kernel's rounding is bounded element by element.
Row-blocked like oracle.losses.fecl_rowblocks -- never more than (block, N) alive -- and device-agnostic: it runs where its inputs are
(the CPU in tests/test_fecl_ref64_cpu.py, the GPU in fp64 in tests/test_fecl_clustered_gpu.py).

Per sample, with L_ij = f_i.f_j / tau off the diagonal and 0 on it, m_j = max_i L_ij (detached), E_ij = exp(L_ij - m_j),
n_i = sum_{j: other label} E_ij, d_ij = E_ij + n_i + 1e-18, P_ij = E_ij / d_ij, c_i = #{j: same label} (the diagonal included):

    phi(P)   = -log(P + 1e-18) (1 - P)^gamma          focal, no gambling        phi' = -(1-P)^gamma / (P+1e-18) + gamma (1-P)^(gamma-1) log(P+1e-18)
             = -log(P + 1e-18)                        otherwise                 phi' = -1 / (P + 1e-18)
    r_i      = sum_{j != i, same label} phi(P_ij)
    kappa_i  = u_i / (c_i - 1 + 1e-18) / (B N)        (u = 1 without gambling: gambling overrides focal)
    student  = sum_i kappa_i r_i (B N)                (= out[0] of the kernels: sum of the per-patch losses)
    H_i      = sum_{j != i, same label} phi'(P_ij) (-E_ij / d_ij^2)              (through n_i)

    W_ij = d loss / d L_ij = kappa_i phi'(P_ij) E_ij (n_i + 1e-18) / d_ij^2      same label, j != i
                           = kappa_i H_i E_ij                                    other label
                           = 0                                                   j == i (the diagonal logit is the constant 0)

Cross branch (teacher given): S_ij = f_i.t_j, hard_ij = other label and S_ij > thr, cross_num = sum -log(1 - S + 1e-18) over hard pairs,
cross_cnt = their number, both over the WHOLE batch; when cross_cnt > 0 the loss gains lambda cross_num / (cross_cnt + 1e-18) and
X_ij = lambda / (cross_cnt + 1e-18) / (1 - S_ij + 1e-18) on hard pairs.  The logarithm is taken on the hard pairs only, as the kernels
take it: the oracle's product log(1 - S + 1e-18) * hard is NaN * 0 where a SAME-label S exceeds 1, which f_i.t_i of bf16-rounded unit
rows does.

    grad_i    = sum_j (W_ij + W_ji) f_j / tau + sum_j X_ij t_j
    absgrad_i = sum_j (|W_ij| + |W_ji|) |f_j| / tau + sum_j |X_ij| |t_j|
    grad_u_i  = r_i / (c_i - 1 + 1e-18) / (B N)
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
import torch.nn.functional as F

EPS = 1e-18


class Fecl64(NamedTuple):
    loss: torch.Tensor            # ()
    student_sum: torch.Tensor     # ()  sum of the per-patch losses (out[0])
    cross_num: torch.Tensor       # ()  (out[1])
    cross_cnt: torch.Tensor       # ()  (out[2])
    grad: torch.Tensor            # (B, N, Dm)
    grad_u: Optional[torch.Tensor]  # (B, N) when gambling is given
    absgrad: torch.Tensor         # (B, N, Dm)


def _phi(P, focal, gamma):
    """phi(P), phi'(P) (see the module docstring)"""
    lg = torch.log(P + EPS)
    if not focal:
        return -lg, -1.0 / (P + EPS)
    om = 1.0 - P
    return -lg * om ** gamma, -(om ** gamma) / (P + EPS) + gamma * om ** (gamma - 1.0) * lg


def _blocks(N, block):
    return [(r0, min(N, r0 + block)) for r0 in range(0, N, block)]


def fecl_pairs64(feat, mask, teacher=None, gambling=None, thr=0.3, tau=0.6, gamma=2.0, use_focal=False, lambda_cross=1.0,
                 block=512) -> Fecl64:
    """feat / teacher (B, N, Dm), mask (B, N) or (B, 1, N), gambling (B, N) or None; any float dtype, computed in float64 on feat's
    device.  thr is the hard-negative threshold itself (oracle.losses.threshold_rampup of the epoch)."""
    B, N, Dm = feat.shape
    dev = feat.device
    f = feat.detach().double()
    t = teacher.detach().double() if teacher is not None else None
    m = mask.detach().reshape(B, N).double()
    u = gambling.detach().reshape(B, N).double() if gambling is not None else None
    focal = bool(use_focal) and u is None
    BN = float(B * N)
    ar = torch.arange(N, device=dev)

    # ---- sweep 1: column max, row statistics, the three accumulators
    cmax = torch.zeros(B, N, dtype=torch.float64, device=dev)       # 0: the diagonal logit
    nrow = torch.empty(B, N, dtype=torch.float64, device=dev)
    rrow = torch.empty(B, N, dtype=torch.float64, device=dev)
    hrow = torch.empty(B, N, dtype=torch.float64, device=dev)
    denom = torch.empty(B, N, dtype=torch.float64, device=dev)
    cross_num = torch.zeros((), dtype=torch.float64, device=dev)
    cross_cnt = torch.zeros((), dtype=torch.float64, device=dev)
    for b in range(B):
        for r0, r1 in _blocks(N, block):
            L = f[b, r0:r1] @ f[b].t() / tau
            L[ar[: r1 - r0], ar[r0:r1]] = 0.0
            cmax[b] = torch.maximum(cmax[b], L.max(0)[0])
        for r0, r1 in _blocks(N, block):
            L = f[b, r0:r1] @ f[b].t() / tau
            L[ar[: r1 - r0], ar[r0:r1]] = 0.0
            same = m[b, r0:r1, None] == m[b][None, :]
            on = same.clone()
            on[ar[: r1 - r0], ar[r0:r1]] = False                   # same label, off the diagonal
            E = torch.exp(L - cmax[b][None, :])
            n = (E * ~same).sum(-1, keepdim=True)
            d = E + n + EPS
            P = E / d
            phi, dphi = _phi(P, focal, gamma)
            nrow[b, r0:r1] = n[:, 0]
            rrow[b, r0:r1] = (phi * on).sum(-1)
            hrow[b, r0:r1] = (dphi * (-E / (d * d)) * on).sum(-1)
            denom[b, r0:r1] = same.sum(-1).double() - 1.0 + EPS
            if t is not None:
                S = f[b, r0:r1] @ t[b].t()
                hard = ~same & (S > thr)
                cross_num = cross_num - torch.log(torch.where(hard, 1.0 - S + EPS, torch.ones_like(S))).sum()
                cross_cnt = cross_cnt + hard.sum()
    kappa = (u if u is not None else 1.0) / denom / BN
    student_sum = (kappa * rrow).sum() * BN
    use_cross = t is not None and float(cross_cnt) > 0
    loss = student_sum / BN
    if use_cross:
        loss = loss + lambda_cross * cross_num / (cross_cnt + EPS)
    grad_u = rrow / denom / BN if u is not None else None

    # ---- sweep 2: pair weights of both directions, the gradient and its absolute-value twin
    grad = torch.empty(B, N, Dm, dtype=torch.float64, device=dev)
    absg = torch.empty(B, N, Dm, dtype=torch.float64, device=dev)
    for b in range(B):
        fa = f[b].abs()
        for r0, r1 in _blocks(N, block):
            L = f[b, r0:r1] @ f[b].t() / tau
            L[ar[: r1 - r0], ar[r0:r1]] = 0.0
            same = m[b, r0:r1, None] == m[b][None, :]
            W = torch.zeros_like(L)
            Wa = torch.zeros_like(L)
            # direction 0: row i's loss, column statistic m_j, row statistics of i; direction 1: row j's loss at its column i
            for cm, nn_, kk, hh in ((cmax[b][None, :], nrow[b, r0:r1, None], kappa[b, r0:r1, None], hrow[b, r0:r1, None]),
                                    (cmax[b, r0:r1, None], nrow[b][None, :], kappa[b][None, :], hrow[b][None, :])):
                E = torch.exp(L - cm)
                d = E + nn_ + EPS
                _, dphi = _phi(E / d, focal, gamma)
                w = torch.where(same, kk * dphi * E * (nn_ + EPS) / (d * d), kk * hh * E)
                W += w
                Wa += w.abs()
            W[ar[: r1 - r0], ar[r0:r1]] = 0.0
            Wa[ar[: r1 - r0], ar[r0:r1]] = 0.0
            grad[b, r0:r1] = W @ f[b] / tau
            absg[b, r0:r1] = Wa @ fa / tau
            if use_cross:
                S = f[b, r0:r1] @ t[b].t()
                X = torch.where(~same & (S > thr), lambda_cross / (cross_cnt + EPS) / (1.0 - S + EPS), torch.zeros_like(S))
                grad[b, r0:r1] += X @ t[b]
                absg[b, r0:r1] += X.abs() @ t[b].abs()
    return Fecl64(loss, student_sum, cross_num, cross_cnt, grad, grad_u, absg)


# ------------------------------------------------------------------------------------------------------------------ clustered inputs
MASK_KINDS = ("mixed", "oneclass", "singleton", "block_aligned")


def clustered(B, N, Dm, seed, K=12, s2=0.2, teacher_noise=0.03, masks=None):
    """Features as a trained projection head leaves them: K orthonormal centres, every row a noisy copy of one of them
    (same-cluster cosines near 1 / (1 + s2)), the teacher a slightly perturbed student; both rounded to bf16.  The mask is
    Bernoulli(rho_k) per cluster with rho_k in [0.05, 0.65], so every cluster holds both labels and the hard negatives of the
    cross branch are the different-label pairs of one cluster.  masks: one of MASK_KINDS per sample (default all 'mixed'), applied
    on top.  Returns CPU tensors (feat bf16, teacher bf16, mask fp32 (B, N)); generated on the CPU from `seed` alone, so the CPU and
    the GPU tests see the same values."""
    masks = list(masks) if masks is not None else ["mixed"] * B
    assert len(masks) == B and all(k in MASK_KINDS for k in masks)
    g = torch.Generator().manual_seed(seed)
    q, _ = torch.linalg.qr(torch.randn(Dm, K, generator=g, dtype=torch.float64))
    centres = q.t().contiguous()                                           # (K, Dm) orthonormal rows
    cid = torch.randint(0, K, (B, N), generator=g)
    fd = F.normalize(centres[cid] + (s2 / Dm) ** 0.5 * torch.randn(B, N, Dm, generator=g, dtype=torch.float64), dim=-1)
    td = F.normalize(fd + teacher_noise / Dm ** 0.5 * torch.randn(B, N, Dm, generator=g, dtype=torch.float64), dim=-1)
    rho = 0.05 + 0.6 * torch.rand(B, K, generator=g, dtype=torch.float64)
    mask = (torch.rand(B, N, generator=g, dtype=torch.float64) < torch.gather(rho, 1, cid)).float()
    one = torch.randint(0, N, (B,), generator=g)
    for b, kind in enumerate(masks):
        if kind == "oneclass":
            mask[b] = 0.0
        elif kind == "singleton":
            mask[b] = 0.0
            mask[b, one[b]] = 1.0
        elif kind == "block_aligned":
            assert N > 128
            mask[b] = 0.0
            mask[b, 128:256] = 1.0
    return fd.to(torch.bfloat16), td.to(torch.bfloat16), mask


class Gap(NamedTuple):
    margin: float      # min |S_ij - thr| over the different-label pairs (inf when there is none)
    smax: float        # max S_ij over the different-label pairs (-inf when there is none)
    share: list        # per sample: the share of its different-label pairs above thr (nan when it has none)


def threshold_gap(feat, teacher, mask, thr, block=512) -> Gap:
    """The conditions under which a fp32-accumulating kernel and the fp64 reference take the same cross branch for every pair:
    S = f.t^T in float64 on the (rounded) values given, over the different-label pairs of each sample."""
    B, N, _ = feat.shape
    f, t, m = feat.double(), teacher.double(), mask.reshape(B, N)
    margin, smax, share = float("inf"), float("-inf"), []
    for b in range(B):
        above = total = 0
        for r0, r1 in _blocks(N, block):
            S = f[b, r0:r1] @ t[b].t()
            diff = m[b, r0:r1, None] != m[b][None, :]
            if bool(diff.any()):
                Sd = S[diff]
                margin = min(margin, float((Sd - thr).abs().min()))
                smax = max(smax, float(Sd.max()))
                above += int((Sd > thr).sum())
                total += int(diff.sum())
        share.append(above / total if total else float("nan"))
    return Gap(margin, smax, share)


MIN_MARGIN, MAX_COS, MIN_SHARE = 0.02, 0.95, 0.05


def assert_gap(feat, teacher, mask, thr, masks, what="", expect_hard=True):
    """The three conditions every clustered GPU case must meet (asserted on the CPU for every case, and again on the GPU before the
    comparison): no different-label pair within MIN_MARGIN of thr, none above MAX_COS, and in every 'mixed' sample at least MIN_SHARE
    of the different-label pairs above thr -- or, for a case built to have an EMPTY cross branch (expect_hard=False), none at all."""
    gap = threshold_gap(feat, teacher, mask, thr)
    print(f"{what} thr {thr}: margin {gap.margin:.4f}, max different-label cosine {gap.smax:.4f}, "
          f"share above {[round(s, 4) for s in gap.share]}")
    assert gap.margin >= MIN_MARGIN, f"{what}: a different-label pair lies {gap.margin:.4f} from thr {thr}"
    assert gap.smax <= MAX_COS, f"{what}: different-label cosine {gap.smax:.4f} > {MAX_COS}"
    for kind, s in zip(masks, gap.share):
        if not expect_hard:
            assert not s > 0, f"{what}: {s:.4f} of the different-label pairs are above thr {thr}, the case needs none"
        elif kind == "mixed":
            assert s >= MIN_SHARE, f"{what}: only {s:.4f} of a mixed sample's different-label pairs are above thr {thr}"
    return gap


# ------------------------------------------------------------------------------------------------------------------ the GPU cases
# Shared by the CPU test of the gap conditions and the GPU test.
class Case(NamedTuple):
    id: str
    B: int
    N: int
    Dm: int
    focal: bool
    teacher: bool
    gambling: bool
    masks: list          # one of MASK_KINDS per sample
    thrs: tuple          # the hard-negative thresholds the case runs at
    seed: int = 0


CASES = [
    Case("headline_b2", 2, 1728, 256, True, True, False, ["mixed", "mixed"], (0.30, 0.50)),
    Case("headline_b8", 8, 1728, 256, True, True, False, ["mixed"] * 6 + ["oneclass", "singleton"], (0.30, 0.50)),
    Case("cs1_b40", 40, 1152, 128, True, True, False, ["mixed"] * 40, (0.30, 0.50)),
    Case("ragged_1025", 1, 1025, 256, True, True, False, ["mixed"], (0.30, 0.50)),
    # the cases with one threshold run at 0.50: `v >= thr + c` in place of `v > thr` stays inside the gap from 0.30 for c up to 0.4
    Case("min_1024", 2, 1024, 64, False, True, False, ["mixed", "block_aligned"], (0.50,)),
    Case("gambling", 2, 1728, 128, True, True, True, ["mixed", "singleton"], (0.50,)),
    Case("no_teacher", 2, 1728, 256, True, False, False, ["mixed", "oneclass"], (0.50,)),
    Case("cross_empty", 1, 1536, 256, True, True, False, ["oneclass"], (0.50,)),
    # not in the issue's table: a teacher, different labels, and a threshold above every cosine (MAX_COS + MIN_MARGIN): out[2] == 0
    # with a student term that is NOT zero (a one-class sample has P = 1, loss and gradient exactly 0)
    Case("cross_empty_mixed", 1, 1536, 256, True, True, False, ["mixed"], (0.97,)),
    Case("below_floor", 2, 1000, 256, True, True, False, ["mixed", "mixed"], (0.50,)),
    Case("ddp_parts", 2, 1728, 256, True, True, False, ["mixed", "mixed"], (0.50,)),
]
CASE_THR = [(c.id, thr) for c in CASES for thr in c.thrs]
CROSS_EMPTY = ("cross_empty", "cross_empty_mixed")          # cases whose cross branch must count no pair


def case(cid) -> Case:
    return next(c for c in CASES if c.id == cid)


def case_inputs(cid):
    """(feat, teacher, mask, u or None) of a case, CPU tensors; u uniform in [0.05, 1) from the case's seed"""
    c = case(cid)
    f, t, mask = clustered(c.B, c.N, c.Dm, c.seed, masks=c.masks)
    u = None
    if c.gambling:
        u = 0.05 + 0.95 * torch.rand(c.B, c.N, generator=torch.Generator().manual_seed(c.seed + 1))
    return f, t, mask, u
