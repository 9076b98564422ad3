"""Supervised / consistency losses of the step with the reference's names (code/utils/losses.py).

Two families:

* the reference's OWN callables with the reference's argument meaning -- ``dice_loss(score, target)``,
  ``softmax_mse_loss(a, b, sigmoid=False)`` (element-wise result), ``softmax_kl_loss``,
  ``DiceLoss(n)(inputs, target, weight=None, softmax=False)`` -- on small streaming HIP kernels
  (csrc/reflosses.hip), so the reference's training-loop body (train_DyCON_BraTS19.py:298-372) runs on this
  package with only its imports changed; and the rest of the reference module's public names, which its scripts do not
  call but people vary the recipe with: ``dice_loss1``, ``softmax_dice_loss``, ``entropy_loss``, ``entropy_loss_map``,
  ``entropy_minmization``, ``entropy_map``, ``symmetric_mse_loss``, ``compute_kl_loss``, ``FocalLoss`` and the legacy
  ``FeCLoss(device, temperature)``, with the reference's quirks kept (plain sums in ``dice_loss1``, gradient to BOTH sides
  of ``softmax_dice_loss``, the last-dimension softmax of ``compute_kl_loss``, the detached ``pt`` of ``FocalLoss``);
* the fast forms the fused trainer uses: ONE pass over the logits for every voxel loss
  (``fused_voxel_losses`` and the ``*_from_logits`` / ``*_mean`` wrappers, 2..8 classes; the softmax is part of the kernel).
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from .. import ops
from .._lib import View, call
from .dycon_losses import _FeCLFunction, _ndhwc_logits

CE, DICE_FG, DICE_MC, CONS_MSE, CONS_KL, UNCL = range(6)


class _VoxelLossFunction(torch.autograd.Function):
    """vals[6] = ce, dice(class 1), dice(multi-class), consistency mse, consistency kl, uncl."""

    @staticmethod
    def forward(ctx, s_logits, t_logits, labels, labeled_bs, beta):
        s, t = _ndhwc_logits(s_logits), _ndhwc_logits(t_logits)
        B = s.shape[0]
        V = s.numel() // (2 * B)
        lab = labels.contiguous()
        sums = ops.seg_losses_fwd(s, t, lab, labeled_bs, beta)
        vals = ops.seg_losses_finalize(sums, B, labeled_bs, V, beta)
        ctx.save_for_backward(s, t, sums, lab)
        ctx.meta = (labeled_bs, beta)
        return vals[:6]

    @staticmethod
    def backward(ctx, g):
        s, t, sums, lab = ctx.saved_tensors
        LB, beta = ctx.meta
        g = g.float()
        # kernel coefficient slots: ce, dice_fg, dice_mc, consistency, uncl ; mse and kl need separate passes
        out = None
        for kind, cons_g in ((0, g[CONS_MSE:CONS_MSE + 1]), (1, g[CONS_KL:CONS_KL + 1])):
            coef = torch.zeros(5, dtype=torch.float32, device=s.device)
            if kind == 0:
                coef[0:3] = g[0:3]
                coef[4:5] = g[UNCL:UNCL + 1]
            coef[3:4] = cons_g
            part = ops.seg_losses_bwd(s, t, lab, LB, beta, sums, coef, kind)
            out = part if out is None else ops.add(out, part)
        return out.permute(0, 4, 1, 2, 3), None, None, None, None


class _VoxelLossClassesFunction(torch.autograd.Function):
    """_VoxelLossFunction for 3..8 classes: the C-class pass (dycon_seg_lossesc_*), both consistency kinds accumulated."""

    @staticmethod
    def forward(ctx, s_logits, t_logits, labels, labeled_bs, beta):
        s, t = _ndhwc_logits_c(s_logits), _ndhwc_logits_c(t_logits)
        B, C = s.shape[0], s.shape[-1]
        V = s.numel() // (C * B)
        lab = labels.contiguous()
        sums = ops.seg_lossesc_fwd(s, t, lab, labeled_bs, beta, cons_kind=2)
        vals = ops.seg_lossesc_finalize(sums, B, labeled_bs, V, C, beta)
        ctx.save_for_backward(s, t, sums, lab)
        ctx.meta = (labeled_bs, beta)
        return vals[:6]

    @staticmethod
    def backward(ctx, g):
        s, t, sums, lab = ctx.saved_tensors
        LB, beta = ctx.meta
        g = g.float()
        out = None
        for kind, cons_g in ((0, g[CONS_MSE:CONS_MSE + 1]), (1, g[CONS_KL:CONS_KL + 1])):
            coef = torch.zeros(5, dtype=torch.float32, device=s.device)
            if kind == 0:
                coef[0:3] = g[0:3]
                coef[4:5] = g[UNCL:UNCL + 1]
            coef[3:4] = cons_g
            part = ops.seg_lossesc_bwd(s, t, lab, LB, beta, sums, coef, kind)
            out = part if out is None else ops.add(out, part)
        return out.permute(0, 4, 1, 2, 3), None, None, None, None


def _ndhwc_logits_c(x):
    """(B,C,D,H,W) any strides -> contiguous fp32 (B,D,H,W,C), C in 2..8"""
    if x.dim() != 5 or not 2 <= x.shape[1] <= 8:
        raise ValueError(f"expected logits (B,C,D,H,W) with C in 2..8, got {tuple(x.shape)}")
    return x.permute(0, 2, 3, 4, 1).contiguous().float()


def fused_voxel_losses(s_logits, t_logits, labels, labeled_bs, beta=1.0):
    """One pass over student/teacher logits (B,C,D,H,W), C in 2..8, and labels (B,D,H,W): returns the 6 scalars
    (ce, dice_fg, dice_multiclass, cons_mse, cons_kl, uncl) as a differentiable tensor (train_DyCON_BraTS19.py:308-352).
    Two classes run the 2-class kernels, any other count the C-class ones; dice_fg scores class 1 either way."""
    if s_logits.dim() != 5 or not 2 <= s_logits.shape[1] <= 8 or s_logits.shape != t_logits.shape:
        raise ValueError(f"fused_voxel_losses: expected two (B,C,D,H,W) logit tensors with C in 2..8, got {tuple(s_logits.shape)} "
                         f"and {tuple(t_logits.shape)}")
    fn = _VoxelLossFunction if s_logits.shape[1] == 2 else _VoxelLossClassesFunction
    return fn.apply(s_logits, t_logits.detach(), labels, int(labeled_bs), float(beta))


def dice_loss_from_logits(logits, target):
    """losses.dice_loss(softmax(logits)[:,1], target) (losses.py:8-16) -- fused: takes the LOGITS."""
    lab = target.to(torch.uint8) if target.dtype == torch.bool else target
    return fused_voxel_losses(logits, logits, lab, logits.shape[0])[DICE_FG]


def cross_entropy_from_logits(logits, target):
    """F.cross_entropy(logits, target) for 2..8 classes (train_DyCON_BraTS19.py:313)."""
    return fused_voxel_losses(logits, logits, target, logits.shape[0])[CE]


def softmax_mse_loss_mean(input_probs_logits, target_probs_logits):
    """mean of losses.softmax_mse_loss(softmax(a), softmax(b)) as the step uses it (train_DyCON_BraTS19.py:352):
    pass the LOGITS; both softmaxes of the reference's double application are inside the kernel."""
    dummy = torch.empty(1, dtype=torch.uint8, device=input_probs_logits.device)
    return fused_voxel_losses(input_probs_logits, target_probs_logits, dummy, 0)[CONS_MSE]


def softmax_kl_loss_mean(input_probs_logits, target_probs_logits):
    """losses.softmax_kl_loss(softmax(a), softmax(b)) (losses.py:85-104) from LOGITS."""
    dummy = torch.empty(1, dtype=torch.uint8, device=input_probs_logits.device)
    return fused_voxel_losses(input_probs_logits, target_probs_logits, dummy, 0)[CONS_KL]


# ------------------------------------------------------------------ the reference's callables, reference semantics
_TKIND = {torch.float32: 0, torch.uint8: 1, torch.bool: 1, torch.int64: 2}


def _f32(t):
    if not t.is_cuda:
        raise RuntimeError("the loss kernels run on the MI355X only (no CPU fallback): pass CUDA tensors")
    return t if t.dtype == torch.float32 else t.float()


def _collapse(shape, strides):
    """one (count, element stride) for a run of dims visited in natural order, or None if they do not collapse"""
    dims = [(n, s) for n, s in zip(shape, strides) if n != 1]
    if not dims:
        return 1, 1
    for (_, s0), (n1, s1) in zip(dims[:-1], dims[1:]):
        if s0 != s1 * n1:
            return None
    cnt = 1
    for n, _ in dims:
        cnt *= n
    return cnt, dims[-1][1]


def _view_ncv(t):
    """(tensor, View, n, C, V) of a (n, C, *spatial) tensor; copies only when the spatial dims do not collapse to one stride."""
    sp = _collapse(t.shape[2:], t.stride()[2:])
    if sp is None:
        t = t.contiguous()
        sp = _collapse(t.shape[2:], t.stride()[2:])
    V, sv = sp
    return t, View(t.data_ptr(), t.stride(0), t.stride(1), sv), t.shape[0], t.shape[1], V


def _view_flat(t):
    """(tensor, View, numel) of any tensor visited in natural order as (1, 1, numel)."""
    fl = _collapse(t.shape, t.stride())
    if fl is None:
        t = t.contiguous()
        fl = _collapse(t.shape, t.stride())
    return t, View(t.data_ptr(), 0, 0, fl[1]), fl[0]


def _ref(v):
    import ctypes
    return ctypes.byref(v)


class _SoftmaxMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, sigmoid):
        a, b = _f32(a), _f32(b)
        a, va, n, C, V = _view_ncv(a)
        b, vb, _, _, _ = _view_ncv(b)
        out = torch.empty_like(a)
        out, vo, _, _, _ = _view_ncv(out)
        call("dycon_softmax_mse_fwd", _ref(va), _ref(vb), _ref(vo), n, C, V, int(sigmoid), ops._s())
        ctx.save_for_backward(a, b)
        ctx.sigmoid = sigmoid
        return out

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g, vg, n, C, V = _view_ncv(_f32(g))
        grads = []
        for need, (x, y) in zip(ctx.needs_input_grad[:2], ((a, b), (b, a))):     # symmetric loss: swap for the second argument
            if not need:
                grads.append(None)
                continue
            _, vx, _, _, _ = _view_ncv(x)
            _, vy, _, _, _ = _view_ncv(y)
            gx = torch.empty_like(x)
            gx, vgx, _, _, _ = _view_ncv(gx)
            call("dycon_softmax_mse_bwd", _ref(vx), _ref(vy), _ref(vg), _ref(vgx), n, C, V, int(ctx.sigmoid), ops._s())
            grads.append(gx)
        return grads[0], grads[1], None


def softmax_mse_loss(input_logits, target_logits, sigmoid=False):
    """losses.py:65-82: (softmax(input, 1) - softmax(target, 1))**2, ELEMENT-WISE (the caller takes .mean(),
    train_DyCON_BraTS19.py:352).  The reference passes probabilities here, so its softmax is applied twice -- so is this one."""
    assert input_logits.size() == target_logits.size()
    return _SoftmaxMSE.apply(input_logits, target_logits, bool(sigmoid))


class _SoftmaxKL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, sigmoid):
        a, b = _f32(a), _f32(b)
        a, va, n, C, V = _view_ncv(a)
        b, vb, _, _, _ = _view_ncv(b)
        scratch = torch.empty(1, dtype=torch.float64, device=a.device)
        out = torch.empty(1, dtype=torch.float32, device=a.device)
        call("dycon_softmax_kl_fwd", _ref(va), _ref(vb), n, C, V, int(sigmoid), scratch.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(a, b)
        ctx.sigmoid = sigmoid
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        _, va, n, C, V = _view_ncv(a)
        _, vb, _, _, _ = _view_ncv(b)
        gu = _f32(g).reshape(1).contiguous()
        grads = []
        for which, (need, x) in enumerate(zip(ctx.needs_input_grad[:2], (a, b))):
            if not need:
                grads.append(None)
                continue
            gx = torch.empty_like(x)
            gx, vgx, _, _, _ = _view_ncv(gx)
            call("dycon_softmax_kl_bwd", _ref(va), _ref(vb), n, C, V, int(ctx.sigmoid), which, gu.data_ptr(), _ref(vgx), ops._s())
            grads.append(gx)
        return grads[0], grads[1], None


def softmax_kl_loss(input_logits, target_logits, sigmoid=False):
    """losses.py:85-104: F.kl_div(log_softmax(input, 1), softmax(target, 1), reduction='mean') -> 0-dim tensor."""
    assert input_logits.size() == target_logits.size()
    return _SoftmaxKL.apply(input_logits, target_logits, bool(sigmoid))


class _Dice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, score, target, onehot, softmax, weights, n_div):
        score = _f32(score)
        if target.dtype not in _TKIND:
            target = target.float()
        if onehot:
            score, vs, n, C, V = _view_ncv(score)
            target, vt_, tn, tC, tV = _view_ncv(target)          # (n, 1, *spatial) label map
            if (tn, tC, tV) != (n, 1, V):
                raise ValueError(f"DiceLoss: target {tuple(target.shape)} does not match inputs {tuple(score.shape)}")
            vt = View(target.data_ptr(), target.stride(0), 0, vt_.sv)
        else:
            if score.shape != target.shape:
                raise ValueError(f"dice_loss: score {tuple(score.shape)} vs target {tuple(target.shape)}")
            score, vs, V = _view_flat(score)
            target, vt, _ = _view_flat(target)
            n, C = 1, 1
        import ctypes
        w = (ctypes.c_float * C)(*[float(x) for x in weights]) if weights is not None else None
        sums = torch.empty(24, dtype=torch.float64, device=score.device)
        out = torch.empty(1, dtype=torch.float32, device=score.device)
        args = (_ref(vs), _ref(vt), _TKIND[target.dtype], int(onehot), n, C, V, int(softmax), w, float(n_div))
        call("dycon_dice_fwd", *args, sums.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(score, target, sums)
        ctx.args = args
        return out[0]

    @staticmethod
    def backward(ctx, g):
        score, target, sums = ctx.saved_tensors
        gu = _f32(g).reshape(1).contiguous()
        gs = torch.empty(score.shape, dtype=torch.float32, device=score.device)     # contiguous, natural order
        if ctx.args[3]:
            _, vg, _, _, _ = _view_ncv(gs)
        else:
            _, vg, _ = _view_flat(gs)
        call("dycon_dice_bwd", *ctx.args, sums.data_ptr(), gu.data_ptr(), _ref(vg), ops._s())
        return gs, None, None, None, None, None


def dice_loss(score, target):
    """losses.py:8-16: 1 - (2 sum(score*target) + 1e-5) / (sum(score^2) + sum(target^2) + 1e-5), sums over the whole tensors
    (call site train_DyCON_BraTS19.py:314: score = probs[:LB, 1], target = label[:LB] == 1)."""
    return _Dice.apply(score, target, False, False, None, 1.0)


class DiceLoss(nn.Module):
    """losses.DiceLoss(n_classes) (losses.py:156-192): forward(inputs, target, weight=None, softmax=False) with the reference's
    argument meaning -- ``inputs`` (B, n, ...) probabilities (or logits with softmax=True), ``target`` (B, 1, ...) label map
    (train_DyCON_ISLES22.py:194,247).  (The reference also reads every class's dice back to the host -- ``.item()`` per class --
    into a list it never uses; that synchronisation is not reproduced.)"""

    def __init__(self, n_classes):
        super().__init__()
        if not 1 <= n_classes <= 8:
            raise NotImplementedError("1..8 classes")
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        if target.dim() == inputs.dim() - 1:
            target = target.unsqueeze(1)
        assert inputs.shape[1] == self.n_classes and inputs.shape[0] == target.shape[0] and inputs.shape[2:] == target.shape[2:], \
            "predict & target shape do not match"
        return _Dice.apply(inputs, target, True, bool(softmax), weight, float(self.n_classes))


# ------------------------------------------------------------------ the rest of the reference module (csrc/reflosses.hip, second half)
def _scratch(dev, doubles=1):
    return torch.empty(doubles, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float32, device=dev)


def _grad_like(x, view):
    """(fp32 gradient buffer of x's shape in natural order, its view)"""
    g = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    return g, view(g)[1]


class _Dice1(torch.autograd.Function):
    """softmax=False: dice_loss1 on flat views (C = 1); softmax=True: softmax_dice_loss on (n, C, V) logits."""

    @staticmethod
    def forward(ctx, a, b, softmax):
        a = _f32(a)
        if softmax or b.dtype not in _TKIND:
            b = _f32(b)
        if a.shape != b.shape:
            raise ValueError(f"dice_loss1: score {tuple(a.shape)} vs target {tuple(b.shape)}")
        if softmax:
            a, va, n, C, V = _view_ncv(a)
            b, vb, _, _, _ = _view_ncv(b)
        else:
            a, va, V = _view_flat(a)
            b, vb, _ = _view_flat(b)
            n, C = 1, 1
        sums, out = _scratch(a.device, 24)
        call("dycon_dice1_fwd", _ref(va), _ref(vb), _TKIND[b.dtype], n, C, V, int(softmax), sums.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(a, b, sums)
        ctx.meta = (n, C, V, softmax)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a, b, sums = ctx.saved_tensors
        n, C, V, softmax = ctx.meta
        gu = _f32(g).reshape(1).contiguous()
        view = (lambda t: (t, _view_ncv(t)[1])) if softmax else (lambda t: (t, _view_flat(t)[1]))
        grads = []
        for need, (x, y) in zip(ctx.needs_input_grad[:2], ((a, b), (b, a))):        # symmetric denominators: swap for the target
            if not need:
                grads.append(None)
                continue
            gx, vgx = _grad_like(x, view)
            call("dycon_dice1_bwd", _ref(view(x)[1]), _ref(view(y)[1]), _TKIND[y.dtype], n, C, V, int(softmax), sums.data_ptr(),
                 gu.data_ptr(), _ref(vgx), ops._s())
            grads.append(gx)
        return grads[0], grads[1], None


def dice_loss1(score, target):
    """losses.py:19-27: 1 - (2 sum(score*target) + 1e-5) / (sum(score) + sum(target) + 1e-5) -- PLAIN sums, unlike dice_loss.
    Differentiable in ``score`` and, when it is a float tensor that requires grad, in ``target``."""
    return _Dice1.apply(score, target, False)


def softmax_dice_loss(input_logits, target_logits):
    """losses.py:39-56: mean over the classes i of dice_loss1(softmax(input, 1)[:, i], softmax(target, 1)[:, i]); both softmaxes
    are inside the kernel.  Gradients go to BOTH arguments: the reference does not detach the target, whatever its docstring says."""
    assert input_logits.size() == target_logits.size()
    return _Dice1.apply(input_logits, target_logits, True)


class _Entropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, scale, as_map):
        p = _f32(p)
        p, vp, n, C, V = _view_ncv(p)
        ctx.save_for_backward(p)
        ctx.meta = (n, C, V, scale, as_map)
        if as_map:
            out = torch.empty((n, 1) + tuple(p.shape[2:]), dtype=torch.float32, device=p.device)
            call("dycon_entropy_fwd", _ref(vp), n, C, V, scale, out.data_ptr(), None, None, ops._s())
            return out
        sum_, out = _scratch(p.device)
        call("dycon_entropy_fwd", _ref(vp), n, C, V, scale, None, sum_.data_ptr(), out.data_ptr(), ops._s())
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        n, C, V, scale, as_map = ctx.meta
        g = _f32(g).contiguous() if as_map else _f32(g).reshape(1).contiguous()
        gp, vgp = _grad_like(p, lambda t: (t, _view_ncv(t)[1]))
        call("dycon_entropy_bwd", _ref(_view_ncv(p)[1]), n, C, V, scale, g.data_ptr() if as_map else None,
             None if as_map else g.data_ptr(), _ref(vgp), ops._s())
        return gp, None, None


def _entropy(p, scale, as_map):
    if p.dim() < 2 or not 1 <= p.shape[1] <= 8:
        raise ValueError(f"entropy: expected (N, C, ...) with C in 1..8, got {tuple(p.shape)}")
    return _Entropy.apply(p, float(scale), as_map)


def entropy_loss(p, C=2):
    """losses.py:30-36: mean over the voxels of -sum_c p log(p + 1e-6) / log(C); ``p`` is probabilities (any float tensor), fp32 out."""
    return _entropy(p, 1.0 / math.log(C), False)


def entropy_loss_map(p, C=2):
    """losses.py:59-62: the (N, 1, *spatial) map of -sum_c p log(p + 1e-6) / log(C)."""
    return _entropy(p, 1.0 / math.log(C), True)


def entropy_minmization(p):
    """losses.py:195-199 (the reference's spelling): mean over the voxels of -sum_c p log(p + 1e-6)."""
    return _entropy(p, 1.0, False)


def entropy_map(p):
    """losses.py:202-205: the (N, 1, *spatial) map of -sum_c p log(p + 1e-6)."""
    return _entropy(p, 1.0, True)


class _SymMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, va, count = _view_flat(_f32(a))
        b, vb, _ = _view_flat(_f32(b))
        sum_, out = _scratch(a.device)
        call("dycon_sym_mse_fwd", _ref(va), _ref(vb), count, sum_.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(a, b)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        gu = _f32(g).reshape(1).contiguous()
        view = lambda t: (t, _view_flat(t)[1])      # noqa: E731
        grads = []
        for need, (x, y) in zip(ctx.needs_input_grad, ((a, b), (b, a))):
            if not need:
                grads.append(None)
                continue
            gx, vgx = _grad_like(x, view)
            call("dycon_sym_mse_bwd", _ref(view(x)[1]), _ref(view(y)[1]), x.numel(), gu.data_ptr(), _ref(vgx), ops._s())
            grads.append(gx)
        return grads[0], grads[1]


def symmetric_mse_loss(input1, input2):
    """losses.py:107-116: mean((input1 - input2)**2) over any shape, gradients to both arguments."""
    assert input1.size() == input2.size()
    return _SymMSE.apply(input1, input2)


def _view_rows(t):
    """(tensor, View of the rows, n, C, V, L, element stride) of a tensor of 3 or more dimensions seen as rows along its LAST one:
    the leading dimensions are addressed like an (n, C, V) view; copies only when they do not collapse."""
    if _collapse(t.shape[2:-1], t.stride()[2:-1]) is None:
        t = t.contiguous()
    V, sv = _collapse(t.shape[2:-1], t.stride()[2:-1])
    return t, View(t.data_ptr(), t.stride(0), t.stride(1), sv), t.shape[0], t.shape[1], V, t.shape[-1], t.stride(-1)


class _KLRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, q):
        p, vp, n, C, V, L, slp = _view_rows(_f32(p))
        q, vq, _, _, _, _, slq = _view_rows(_f32(q))
        sum_, out = _scratch(p.device)
        call("dycon_kl_rows_fwd", _ref(vp), slp, _ref(vq), slq, n, C, V, L, sum_.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(p, q)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        p, q = ctx.saved_tensors
        gu = _f32(g).reshape(1).contiguous()
        grads = []
        for need, (x, y) in zip(ctx.needs_input_grad, ((p, q), (q, p))):            # symmetric loss: swap for the second argument
            if not need:
                grads.append(None)
                continue
            _, vx, n, C, V, L, slx = _view_rows(x)
            _, vy, _, _, _, _, sly = _view_rows(y)
            gx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
            _, vg, _, _, _, _, slg = _view_rows(gx)
            call("dycon_kl_rows_bwd", _ref(vx), slx, _ref(vy), sly, n, C, V, L, gu.data_ptr(), _ref(vg), slg, ops._s())
            grads.append(gx)
        return grads[0], grads[1]


def compute_kl_loss(p, q):
    """losses.py:208-219: (kl_div(log_softmax(p, -1), softmax(q, -1), 'none').mean() + the same with p and q exchanged) / 2.
    Both softmaxes run over the LAST dimension (not the channels), as in the reference; last dimension 1..1024; gradients to both."""
    if p.size() != q.size():
        raise ValueError(f"compute_kl_loss: {tuple(p.shape)} vs {tuple(q.shape)}")
    if p.dim() < 3:
        p, q = (t.reshape((1,) * (3 - t.dim()) + tuple(t.shape)) for t in (p, q))
    return _KLRows.apply(p, q)


class _Focal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, gamma, alpha, size_average):
        x = _f32(x)
        x, vx, n, C, V = _view_ncv(x)
        if not target.is_cuda:
            raise RuntimeError("the loss kernels run on the MI355X only (no CPU fallback): pass CUDA tensors")
        if target.dtype not in (torch.uint8, torch.int64):
            target = target.long()
        target = target.reshape(-1).contiguous()
        if target.numel() != n * V:
            raise ValueError(f"FocalLoss: target has {target.numel()} elements, input {tuple(x.shape)} needs {n * V}")
        # classes the alpha table does not cover are NaN (the reference's gather raises there)
        w = (ctypes.c_float * C)(*[float(alpha[c]) if c < len(alpha) else math.nan for c in range(C)]) if alpha is not None else None
        sum_, out = _scratch(x.device)
        args = (_ref(vx), target.data_ptr(), _TKIND[target.dtype], n, C, V, float(gamma), w, int(size_average))
        call("dycon_focal_fwd", *args, sum_.data_ptr(), out.data_ptr(), ops._s())
        ctx.save_for_backward(x, target)
        ctx.args = args
        return out[0]

    @staticmethod
    def backward(ctx, g):
        x, _ = ctx.saved_tensors
        gu = _f32(g).reshape(1).contiguous()
        gx, vgx = _grad_like(x, lambda t: (t, _view_ncv(t)[1]))
        call("dycon_focal_bwd", *ctx.args, gu.data_ptr(), _ref(vgx), ops._s())
        return gx, None, None, None, None


class FocalLoss(nn.Module):
    """losses.FocalLoss (losses.py:119-153): forward(input, target) with ``input`` logits (N, C, *spatial) or (M, C), C in 1..8, and
    ``target`` the int64 (or uint8) labels, N*prod(spatial) of them in any shape: mean (``size_average``) or sum of
    -(1 - pt)**gamma * alpha[target] * log(pt), pt = softmax(input, 1)[target].  ``alpha``: None, a list of per-class weights, or a
    number a meaning [a, 1 - a].  As in the reference pt is detached: the gradient flows through log(pt) only.  A superset of the
    reference in one respect: its ``view`` needs a contiguous input, this accepts any strides (channels-last, slices)."""

    def __init__(self, gamma=2, alpha=None, size_average=True):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)):
            self.alpha = torch.Tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.Tensor(alpha)
        self.size_average = size_average

    def forward(self, input, target):
        if input.dim() < 2 or not 1 <= input.shape[1] <= 8:
            raise ValueError(f"FocalLoss: expected (N, C, ...) logits with C in 1..8, got {tuple(input.shape)}")
        alpha = None if self.alpha is None else [float(v) for v in self.alpha.reshape(-1).tolist()]
        return _Focal.apply(input, target, float(self.gamma), alpha, bool(self.size_average))


class FeCLoss(nn.Module):
    """The legacy student-only contrastive loss losses.FeCLoss(device, temperature=0.6) (losses.py:221-251): forward(feat, mask) with
    ``feat`` (B, N, D) normalised rows and ``mask`` (B, 1, N).  Arithmetically dycon_losses.FeCLoss(use_focal=False) without a
    teacher, so it runs on the same kernels."""

    def __init__(self, device, temperature=0.6):
        super().__init__()
        self.device = device
        self.temperature = temperature

    def forward(self, feat, mask):
        if not feat.is_cuda:
            raise RuntimeError("the loss kernels run on the MI355X only (no CPU fallback): pass CUDA tensors")
        return _FeCLFunction.apply(feat, None, mask, None, self.temperature, 2.0, False, 0.0, 1.0)
