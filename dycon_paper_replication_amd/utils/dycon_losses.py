"""UnCL / FeCL with the reference's call signatures (code/utils/dycon_losses.py), on HIP kernels.

Both are torch.autograd.Functions over the C ABI: the forward launches the fused reduction(s), the
backward one more pass.  Nothing of size (B,N,N) or (B,B,V) is ever materialised (the reference
builds ~12 N x N tensors for FeCL and a (B,B,H,W,D) broadcast for UnCL).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import _lib, ops


def adaptive_beta(epoch, total_epochs, max_beta=5.0, min_beta=0.5):
    """dycon_losses.py:8-12."""
    return max_beta * ((min_beta / max_beta) ** (epoch / total_epochs))


class _GamblingSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits):
        x = logits.movedim(1, -1).contiguous().float()
        y = ops.gambling_softmax(x)
        ctx.save_for_backward(y)
        ctx.in_dtype = logits.dtype
        return y.movedim(-1, 1).to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        gx = ops.gambling_softmax_bwd(y, g.movedim(1, -1).contiguous().float())
        return gx.movedim(-1, 1).to(ctx.in_dtype)


def gambling_softmax(logits):
    """dycon_losses.py:14-26: exp(logits) / (sum over dim 1 + 1e-18), NO max shift (logits above ~88.7 give NaN, as there).
    (B, C, ...) with C in 1..8, differentiable."""
    if logits.dim() < 2 or not 1 <= logits.shape[1] <= 8:
        raise ValueError(f"gambling_softmax: expected (B, C, ...) with C in 1..8, got {tuple(logits.shape)}")
    return _GamblingSoftmax.apply(logits)


def sigmoid_rampup(current_epoch, total_rampup_epochs, min_threshold, max_threshold, steepness=5.0):
    """dycon_losses.py:28-47 (threshold schedule of FeCL)."""
    if total_rampup_epochs == 0:
        return max_threshold
    e = max(0.0, min(float(current_epoch), total_rampup_epochs))
    phase = 1.0 - e / total_rampup_epochs
    return min_threshold + (max_threshold - min_threshold) * math.exp(-steepness * phase * phase)


def _ndhwc_logits(x):
    """(B,2,D,H,W) any strides -> contiguous fp32 (B,D,H,W,2); free for channels_last_3d fp32 inputs."""
    if x.dim() != 5 or x.shape[1] != 2:
        raise ValueError(f"expected 2-class logits (B,2,D,H,W), got {tuple(x.shape)}")
    return x.permute(0, 2, 3, 4, 1).contiguous().float()


class _UnCLFunction(torch.autograd.Function):
    """2 classes: the fused voxel-loss kernels of the DyCON step (csrc/losses.hip)."""

    @staticmethod
    def forward(ctx, s_logits, t_logits, beta):
        s, t = _ndhwc_logits(s_logits), _ndhwc_logits(t_logits)
        B = s.shape[0]
        V = s.numel() // (2 * B)
        dummy = torch.empty(1, dtype=torch.uint8, device=s.device)
        sums = ops.seg_losses_fwd(s, t, dummy, 0, beta)
        vals = ops.seg_losses_finalize(sums, B, 0, V, beta)
        ctx.save_for_backward(s, t, sums, dummy)
        ctx.beta = beta
        return vals[5]

    @staticmethod
    def backward(ctx, g):
        s, t, sums, dummy = ctx.saved_tensors
        coef = torch.zeros(5, dtype=torch.float32, device=s.device)
        coef[4:5] = g.reshape(1).float()
        gs = ops.seg_losses_bwd(s, t, dummy, 0, ctx.beta, sums, coef)
        return gs.permute(0, 4, 1, 2, 3), None, None


class _UnCLClassesFunction(torch.autograd.Function):
    """Any other class count in 1..8: dycon_uncl_fwd / _bwd (csrc/reflosses.hip) over strided (n, C, V) views -- an NCDHW tensor and
    the nets' channels-last views are read in place; the gradient is written in the student logits' own layout."""

    @staticmethod
    def forward(ctx, s_logits, t_logits, beta):
        from .losses import _f32, _ref, _scratch, _view_ncv
        s, vs, n, C, V = _view_ncv(_f32(s_logits))
        t, vt, _, _, _ = _view_ncv(_f32(t_logits))
        sum_, out = _scratch(s.device)
        _lib.call("dycon_uncl_fwd", _ref(vs), _ref(vt), n, C, V, beta, sum_.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(s, t)
        ctx.beta, ctx.in_dtype = beta, s_logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        from .losses import _f32, _ref, _view_ncv
        s, t = ctx.saved_tensors
        _, vs, n, C, V = _view_ncv(s)
        _, vt, _, _, _ = _view_ncv(t)
        gu = _f32(g).reshape(1).contiguous()
        gs = torch.empty_like(s)                  # preserves the strides of a dense (permuted) tensor
        gs, vg, _, _, _ = _view_ncv(gs)
        _lib.call("dycon_uncl_bwd", _ref(vs), _ref(vt), n, C, V, ctx.beta, gu.data_ptr(), _ref(vg), ops._s())
        return gs.to(ctx.in_dtype), None, None


class UnCLoss(nn.Module):
    """Uncertainty-weighted consistency (dycon_losses.py:50-118): forward(s_logits, t_logits, beta) -> 0-dim.
    (B, C, D, H, W) logits with C in 1..8; softmax and entropy over dim 1, as the reference."""

    def forward(self, s_logits, t_logits, beta):
        if s_logits.dim() != 5 or not 1 <= s_logits.shape[1] <= 8 or s_logits.shape != t_logits.shape:
            raise ValueError(f"UnCLoss: expected two (B,C,D,H,W) logit tensors with C in 1..8, got {tuple(s_logits.shape)} "
                             f"and {tuple(t_logits.shape)}")
        fn = _UnCLFunction if s_logits.shape[1] == 2 else _UnCLClassesFunction
        return fn.apply(s_logits, t_logits.detach(), float(beta))


class _FeCLFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feat, teacher, mask, gambling, temperature, gamma, use_focal, thr, lambda_cross):
        f = feat.contiguous()
        if f.dtype not in (torch.float32, torch.bfloat16):
            f = f.float()
        t = teacher.contiguous().to(f.dtype) if teacher is not None else None
        m = mask.reshape(f.shape[0], f.shape[1]).contiguous().float()
        gmb = gambling.reshape(f.shape[0], f.shape[1]).contiguous().float() if gambling is not None else None
        args = (f, t, m, gmb, float(temperature), float(gamma), bool(use_focal), float(thr), float(lambda_cross))
        loss, st = ops.fecl_fwd(*args)
        ctx.args, ctx.st, ctx.in_dtype = args, st, feat.dtype
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        gf = ops.fecl_bwd(*ctx.args, ctx.st, g.reshape(1).float().contiguous())
        return (gf.to(ctx.in_dtype),) + (None,) * 8


class _FeCLGamblingFunction(torch.autograd.Function):
    """FeCL with a differentiable uncertainty weight u (dycon_losses.py:209-211): the student term is mean(r * u) with
    r_i = sum_j ell_ij / (cnt_i - 1 + 1e-18) (the focal result is discarded), so d/du_i = g * r_i / (B*N)."""

    @staticmethod
    def forward(ctx, feat, teacher, mask, gambling, temperature, gamma, thr, lambda_cross):
        f = feat.contiguous()
        if f.dtype not in (torch.float32, torch.bfloat16):
            f = f.float()
        B, N = f.shape[0], f.shape[1]
        t = teacher.contiguous().to(f.dtype) if teacher is not None else None
        m = mask.reshape(B, N).contiguous().float()
        u = gambling.reshape(B, N).contiguous().float()
        st = ops.fecl_fwd_rows(f, t, m, float(temperature), float(thr))
        r, _ = ops.fecl_gambling_finalize(f, st, u, want_r=True)
        loss = ops.fecl_finalize(st, B * N, float(lambda_cross), t is not None)
        ctx.args = (f, t, m, None, float(temperature), float(gamma), False, float(thr), float(lambda_cross))
        ctx.st, ctx.r, ctx.in_dtype, ctx.u_meta = st, r, feat.dtype, (gambling.shape, gambling.dtype)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        coef = g.reshape(1).float().contiguous()
        gf = ops.fecl_bwd(*ctx.args, ctx.st, coef)
        gu = ops.fecl_gambling_grad(ctx.r, coef)
        shape, dtype = ctx.u_meta
        return gf.to(ctx.in_dtype), None, None, gu.reshape(shape).to(dtype), None, None, None, None


class FeCLoss(nn.Module):
    """Focal patch-contrastive loss (dycon_losses.py:120-235); same constructor and call signature."""

    def __init__(self, device=None, temperature=0.6, gamma=2.0, use_focal=False, rampup_epochs=2000, lambda_cross=1.0):
        super().__init__()
        self.device, self.temperature, self.gamma = device, temperature, gamma
        self.use_focal, self.rampup_epochs, self.lambda_cross = use_focal, rampup_epochs, lambda_cross

    def forward(self, feat, mask, teacher_feat=None, gambling_uncertainty=None, epoch=0):
        thr = sigmoid_rampup(epoch, self.rampup_epochs, min_threshold=0.3, max_threshold=0.5)
        if gambling_uncertainty is not None and gambling_uncertainty.requires_grad:   # u from the logits, not detached (Pancreas :242-246)
            return _FeCLGamblingFunction.apply(feat, teacher_feat.detach() if teacher_feat is not None else None, mask,
                                               gambling_uncertainty, self.temperature, self.gamma, thr, self.lambda_cross)
        return _FeCLFunction.apply(feat, teacher_feat.detach() if teacher_feat is not None else None, mask,
                                   gambling_uncertainty, self.temperature, self.gamma, self.use_focal, thr, self.lambda_cross)
