"""The V-Net's building blocks as layer modules over the HIP launches of ops.py.

``ConvBlock``, ``ResidualConvBlock``, ``DownsamplingConvBlock``, ``UpsamplingDeconvBlock`` and ``Upsampling`` keep the
constructor signatures, the parameter initialisation (torch's defaults) and the ``state_dict`` keys of code/networks/VNet.py:5-142
(plus a keyword ``dtype``: the storage type of the activations, fp32 or bf16, as on HipSegNet), so a net assembled from them
exchanges checkpoints with one assembled from the reference's classes.  ``self.conv`` is an ``nn.Sequential`` of the same torch
modules at the same indices, used as the parameter container only: it is never called.  Every block is one autograd node whose
forward and backward are explicit launch sequences, the ones engine.Engine issues for the same layer kinds.

Input: (B, C, D, H, W) on the GPU, fp32 or the module's dtype; a ``channels_last_3d`` tensor of the module's dtype is used in
place (its memory is the NDHWC the kernels work in), anything else is converted once.  Output: (B, C', D', H', W') with
``channels_last_3d`` strides in the module's dtype, so a chain of blocks moves no data between layers.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .._lib import CONV_1X1, CONV_K2S2, CONV_K3

NORMS = ("none", "batchnorm", "groupnorm", "instancenorm")      # VNet.py:17-24


def _norm_module(normalization, c):
    if normalization == "batchnorm":
        return nn.BatchNorm3d(c)
    if normalization == "groupnorm":
        if c % 16:
            raise ValueError(f"GroupNorm(16, {c}): the channel count must be divisible by 16 (VNet.py:20)")
        return nn.GroupNorm(num_groups=16, num_channels=c)
    if normalization == "instancenorm":
        return nn.InstanceNorm3d(c)
    return None


def _ndhwc(x, dtype):
    """(B, C, D, H, W) -> contiguous (B, D, H, W, C) of `dtype`: a view when x is channels_last_3d of that dtype already, otherwise
    ONE pass that changes layout and type together"""
    v = x.permute(0, 2, 3, 4, 1)
    if v.is_contiguous():
        return v if v.dtype == dtype else ops.cast(v, dtype)
    return torch.empty(v.shape, dtype=dtype, device=x.device).copy_(v)


class _BlockFunction(torch.autograd.Function):
    """One autograd node per block: stage i is conv_i -> [norm_i] -> ReLU; the residual block adds its input before the last ReLU.
    Saved per stage: the stage input, the pre-norm tensor and the statistics (what Engine's tape keeps)."""

    @staticmethod
    def forward(ctx, x, block, *params):
        dtype = block.compute_dtype
        h = _ndhwc(x.detach(), dtype)
        x0 = h
        tape = []
        last = len(block._stages) - 1
        for i, st in enumerate(block._stages):
            res = x0 if (block._residual and i == last) else None
            z = block._conv_fwd(st, h)
            y, saved = block._norm_fwd(st, z, res)
            tape.append((h, z) + saved)
            h = y
        flat = [t for entry in tape for t in entry]
        ctx.save_for_backward(*[t for t in flat if t is not None])      # version-checked: an in-place change before backward raises
        ctx.block, ctx.present, ctx.x_dtype = block, [t is not None for t in flat], x.dtype
        return h.permute(0, 4, 1, 2, 3)

    @staticmethod
    def backward(ctx, gy):
        block = ctx.block
        it = iter(ctx.saved_tensors)
        flat = [next(it) if has else None for has in ctx.present]
        tape = [tuple(flat[i:i + 4]) for i in range(0, len(flat), 4)]
        g = _ndhwc(gy, block.compute_dtype)
        grads = {}
        g_res = None
        for si in range(len(tape) - 1, -1, -1):
            st, (h, z, stats, n) = block._stages[si], tape[si]
            g, gr = block._norm_bwd(st, z, stats, n, g, grads)
            if gr is not None:
                g_res = gr
            # the first stage's data gradient (for Upsampling: k=3 dgrad + trilinear_bwd) only when the input asks for one
            g = block._conv_bwd(st, h, g, grads, need_gx=si > 0 or ctx.needs_input_grad[0])
        if not ctx.needs_input_grad[0]:
            g = None
        else:
            if g_res is not None:
                g = ops.add(g, g_res)
            if g.dtype != ctx.x_dtype:
                g = ops.cast(g, ctx.x_dtype)
            g = g.permute(0, 4, 1, 2, 3)
        return (g, None) + tuple(grads.get(id(p)) for p in block._plist)


class _Block(nn.Module):
    _residual = False

    def __init__(self, normalization, dtype):
        super().__init__()
        if normalization not in NORMS:
            raise ValueError(f"normalization must be one of {NORMS}, got {normalization!r}")
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"dtype must be torch.float32 or torch.bfloat16, got {dtype}")
        self.normalization, self.compute_dtype = normalization, dtype
        self._stages = []        # (kind, conv index, norm index or None) into self.conv
        self._packs = {}         # (conv index, tag) -> (parameter version, packed operand)

    def _build(self, layers):
        """layers: [(kind, conv module, norm module or None, relu?)] with an optional leading parameter-less module"""
        mods, stages = [], []
        for kind, conv, norm, relu, lead in layers:
            if lead is not None:
                mods.append(lead)
            stages.append((kind, len(mods), len(mods) + 1 if norm is not None else None))
            mods.append(conv)
            if norm is not None:
                mods.append(norm)
            if relu:
                mods.append(nn.ReLU(inplace=True))
        self.conv = nn.Sequential(*mods)
        self._stages = stages
        gq = 8 if self.compute_dtype == torch.bfloat16 else 4
        for kind, ci, _ in stages:
            cin, cout = self._channels(kind, self.conv[ci].weight)
            skinny = cin % gq != 0 or cout % 16 != 0
            if skinny and (kind != "k3" or cout % 16 != 0):
                raise ValueError(f"{type(self).__name__}: {cin} -> {cout} channels are not served by the HIP convolutions (input channels "
                                 f"a multiple of {gq}, output channels a multiple of 16; a k=3 convolution takes any input count)")

    @staticmethod
    def _channels(kind, w):
        return (w.shape[0], w.shape[1]) if kind == "deconv" else (w.shape[1], w.shape[0])

    @property
    def _plist(self):
        return list(self.parameters())

    def forward(self, x):
        if not x.is_cuda or not self.conv[self._stages[0][1]].weight.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the MI355X only (no CPU fallback): move the module and input to 'cuda'")
        cin = self._channels(self._stages[0][0], self.conv[self._stages[0][1]].weight)[0]
        if x.dim() != 5 or x.shape[1] != cin:
            raise ValueError(f"expected (B,{cin},D,H,W), got {tuple(x.shape)}")
        if any(p.dtype != torch.float32 for p in self.parameters()):
            raise TypeError(f"{type(self).__name__} keeps its parameters in fp32 (the kernels pack them into the compute dtype); choose "
                            "bf16 storage with the constructor's dtype=torch.bfloat16, not with .bfloat16() / .half()")
        if x.dtype not in (torch.float32, self.compute_dtype):
            raise TypeError(f"input must be fp32 or {self.compute_dtype}, got {x.dtype}")
        if self._stages[0][0] == "k2s2" and any(s % 2 for s in x.shape[2:]):
            raise ValueError("D, H, W must be even for the stride-2 convolution")
        return _BlockFunction.apply(x, self, *self._plist)

    # ---------------------------------------------------------------- packed operands, refreshed when the weight's version changes
    def _pack(self, ci, tag, kind, *spec, flip=False):
        w = self.conv[ci].weight
        hit = self._packs.get((ci, tag))
        if hit is not None and hit[0] == (w._version, w.data_ptr()):
            return hit[1]
        buf = hit[1] if hit is not None and hit[1].device == w.device else None
        wd = w.detach()
        if kind == "frag":
            buf = ops.pack_bfrag(wd, self.compute_dtype, *spec, flip, out=buf)
        else:
            buf = ops.pack_tcn(wd, *spec, flip, out=buf)
        self._packs[(ci, tag)] = ((w._version, w.data_ptr()), buf)
        return buf

    # ---------------------------------------------------------------- convolutions (chosen as Engine._conv chooses them)
    def _skinny(self, cin, cout):
        return cin % (8 if self.compute_dtype == torch.bfloat16 else 4) != 0 or cout % 16 != 0

    def _conv_fwd(self, st, x):
        kind, ci, _ = st
        w, b = self.conv[ci].weight, self.conv[ci].bias.detach()
        cin, cout = self._channels(kind, w)
        if kind == "deconv":
            wf = self._pack(ci, "f", "frag", 1, cin, 8 * cout, cout, 0, cout * 8, 1, 8)
            return ops.conv_gemm(x, wf, b, CONV_1X1, 8 * cout, cout, scatter=True)
        T, mode = (8, CONV_K2S2) if kind == "k2s2" else (27, CONV_K3)
        if self._skinny(cin, cout):
            wt = self._pack(ci, "tcn", "tcn", T, cin, cout, cout, 1, T, 0, cin * T)
            return ops.conv_direct(x, wt, b, mode, cout, self.compute_dtype)
        wf = self._pack(ci, "f", "frag", T, cin, cout, cout, 1, T, 0, cin * T)
        if kind == "upk3":
            if self._fused_upconv(x, cin, cout):
                return ops.upconv_k3(x, wf, b, cout)
            B, D, H, W, _ = x.shape
            return ops.conv_gemm(ops.trilinear_fwd(x, (2 * D, 2 * H, 2 * W), False), wf, b, CONV_K3, cout, cout)
        return ops.conv_gemm(x, wf, b, mode, cout, cout)

    # Upsampling's forward form.  Measured (profiles/upconv_micro.txt, bf16, B = 4): the fused kernel takes 2.0x / 1.7x / 4.2x the time
    # of resize -> convolution at 48^3 / 24^3 / 6^3 low-resolution grids, so every shape class runs the composition; the fused
    # kernel stays reachable (ops.upconv_k3, or this attribute on a module) for the work DESIGN.md section 7 lists.
    fused_upconv = False

    def _fused_upconv(self, x, cin, cout):
        return self.fused_upconv

    def _conv_bwd(self, st, x, gy, grads, need_gx=True):
        kind, ci, _ = st
        w, b = self.conv[ci].weight, self.conv[ci].bias
        cin, cout = self._channels(kind, w)
        gw, gb = torch.empty_like(w, dtype=torch.float32), torch.empty_like(b, dtype=torch.float32)
        grads[id(w)], grads[id(b)] = gw, gb
        if kind == "deconv":       # dW[ci][co][t] = sum_m x[m, ci] * gy[2m + t, co]: the roles of x and gy swapped
            ops.colsum(gy, gb)
            ops.conv_wgrad(gy, x, gw, CONV_K2S2, 1, 8, cout * 8)
            if not need_gx:
                return None
            wd = self._pack(ci, "d", "frag", 8, cout, cin, cin, 1, 8, 0, cout * 8)
            return ops.conv_gemm(gy, wd, None, CONV_K2S2, cin, cin)
        if kind == "k2s2":         # scatter: gx[2m + t, ci] = sum_co gy[m, co] W[co][ci][t]
            ops.conv_wgrad(x, gy, gw, CONV_K2S2, 1, 8, cin * 8, dbias=gb)
            if not need_gx:
                return None
            wd = self._pack(ci, "d", "frag", 1, cout, 8 * cin, cin, 0, cin * 8, 1, 8)
            return ops.conv_gemm(gy, wd, None, CONV_1X1, 8 * cin, cin, scatter=True)
        src = x
        if kind == "upk3":         # only the low-resolution input was kept: the up-sampled operand is recomputed
            B, D, H, W, _ = x.shape
            src = ops.trilinear_fwd(x, (2 * D, 2 * H, 2 * W), False)
        ops.conv_wgrad(src, gy, gw, CONV_K3, 1, 27, cin * 27, dbias=gb)
        if not need_gx:
            return None
        if self._skinny(cin, cout):    # conv with flipped taps and transposed channels, plain fp32 weights
            wd = self._pack(ci, "tcn_d", "tcn", 27, cout, cin, cin, 1, cin * 27, 0, 27, flip=True)
            gx = ops.conv_direct(gy, wd, None, CONV_K3, cin, self.compute_dtype)
        else:
            wd = self._pack(ci, "d", "frag", 27, cout, cin, cin, 1, cin * 27, 0, 27, flip=True)
            gx = ops.conv_gemm(gy, wd, None, CONV_K3, cin, cin)
        return ops.trilinear_bwd(gx, tuple(x.shape), False) if kind == "upk3" else gx

    # ---------------------------------------------------------------- [norm ->] (+ residual) -> ReLU
    def _norm_geometry(self, z):
        B, C = z.shape[0], z.shape[-1]
        V = z.numel() // (B * C)
        if self.normalization == "groupnorm":
            return B, V, C, 16
        if self.normalization == "instancenorm":
            return B, V, C, C
        return 1, B * V, C, C      # BatchNorm: one sample of B*V voxels

    def _norm_fwd(self, st, z, res):
        """returns (y, (stats, n)): n = the pre-ReLU tensor of the residual stage (None elsewhere).  The apply pass of the kernels
        adds its `skip` AFTER the ReLU (the V-Net's decoder adds), the residual block adds BEFORE it (VNet.py:62-63): there the
        normalisation runs without ReLU with the block input as skip, and the ReLU is its own pass."""
        nm = self.conv[st[2]] if st[2] is not None else None
        if nm is None:
            if res is None:
                return ops.relu_fwd(z), (None, None)
            n = ops.add(z, res)
            return ops.relu_fwd(n), (None, n)
        Nb, V, C, G = self._norm_geometry(z)
        bn = self.normalization == "batchnorm"
        gamma = nm.weight.detach() if nm.weight is not None else None
        beta = nm.bias.detach() if nm.bias is not None else None
        relu = res is None
        if bn and not self.training:      # running statistics (no gradient flows through them)
            stats = torch.stack([nm.running_mean, torch.rsqrt(nm.running_var + nm.eps)], 1).reshape(-1).contiguous()
            y = ops.norm_apply(z, stats, Nb, V, C, G, gamma, beta, relu, res)
            stats = None
        else:
            y, stats = ops.norm_fwd(z, Nb, V, C, G, gamma, beta, relu, res, None, nm.eps, nm.running_mean if bn else None,
                                    nm.running_var if bn else None, nm.momentum if bn else 0.1)
            if bn:
                nm.num_batches_tracked.add_(1)
        if res is None:
            return y, (stats, None)
        return ops.relu_fwd(y), (stats, y)

    def _norm_bwd(self, st, z, stats, n, gy, grads):
        """returns (gz, gradient of the residual input or None)"""
        nm = self.conv[st[2]] if st[2] is not None else None
        g_res = None
        if n is not None:                 # the residual stage's own ReLU pass
            gy = ops.relu_bwd(n, gy)
            g_res = gy
        if nm is None:
            return (gy if n is not None else ops.relu_bwd(z, gy)), g_res
        if stats is None:
            raise RuntimeError("backward through an eval-mode BatchNorm3d block is not implemented: call .train() to differentiate")
        Nb, V, C, G = self._norm_geometry(z)
        gamma = beta = dg = db = None
        if nm.weight is not None:
            gamma, beta = nm.weight.detach(), nm.bias.detach()
            dg, db = torch.empty_like(gamma), torch.empty_like(beta)
            grads[id(nm.weight)], grads[id(nm.bias)] = dg, db
        return ops.norm_bwd(z, False, gy, stats, Nb, V, C, G, gamma, beta, n is None, dg, db), g_res


def _check_stride(stride):
    if stride != 2:
        raise ValueError(f"stride must be 2 (the HIP kernels are the k=2, s=2 and the x2 up-sampling ones), got {stride}")


class ConvBlock(_Block):
    """n_stages x (Conv3d k=3 -> [norm] -> ReLU)   (VNet.py:5-31)"""

    def __init__(self, n_stages, n_filters_in, n_filters_out, normalization="none", dtype=torch.float32):
        super().__init__(normalization, dtype)
        self._build([("k3", nn.Conv3d(n_filters_in if i == 0 else n_filters_out, n_filters_out, 3, padding=1),
                      _norm_module(normalization, n_filters_out), True, None) for i in range(n_stages)])


class ResidualConvBlock(_Block):
    """ConvBlock without the last ReLU, then relu(conv(x) + x)   (VNet.py:34-64)"""
    _residual = True

    def __init__(self, n_stages, n_filters_in, n_filters_out, normalization="none", dtype=torch.float32):
        super().__init__(normalization, dtype)
        if n_filters_in != n_filters_out:
            raise ValueError(f"ResidualConvBlock adds its input to its output: n_filters_in ({n_filters_in}) must equal "
                             f"n_filters_out ({n_filters_out})")
        self._build([("k3", nn.Conv3d(n_filters_in if i == 0 else n_filters_out, n_filters_out, 3, padding=1),
                      _norm_module(normalization, n_filters_out), i != n_stages - 1, None) for i in range(n_stages)])
        self.relu = nn.ReLU(inplace=True)


class DownsamplingConvBlock(_Block):
    """Conv3d k=2, s=2 -> [norm] -> ReLU   (VNet.py:67-91)"""

    def __init__(self, n_filters_in, n_filters_out, stride=2, normalization="none", dtype=torch.float32):
        super().__init__(normalization, dtype)
        _check_stride(stride)
        self._build([("k2s2", nn.Conv3d(n_filters_in, n_filters_out, stride, padding=0, stride=stride),
                      _norm_module(normalization, n_filters_out), True, None)])


class UpsamplingDeconvBlock(_Block):
    """ConvTranspose3d k=2, s=2 -> [norm] -> ReLU   (VNet.py:94-118)"""

    def __init__(self, n_filters_in, n_filters_out, stride=2, normalization="none", dtype=torch.float32):
        super().__init__(normalization, dtype)
        _check_stride(stride)
        self._build([("deconv", nn.ConvTranspose3d(n_filters_in, n_filters_out, stride, padding=0, stride=stride),
                      _norm_module(normalization, n_filters_out), True, None)])


class Upsampling(_Block):
    """trilinear x2 (align_corners=False) -> Conv3d k=3 -> [norm] -> ReLU   (VNet.py:121-142).  Forward: resize -> convolution, or
    with `fused_upconv` the one-kernel form (ops.upconv_k3), measured slower so far; either way only the low-resolution input is
    saved and the backward recomputes the up-sampled operand from it."""

    def __init__(self, n_filters_in, n_filters_out, stride=2, normalization="none", dtype=torch.float32):
        super().__init__(normalization, dtype)
        _check_stride(stride)
        if not (n_filters_in in (16, 48) or n_filters_in % 32 == 0) or n_filters_out % 16:
            raise ValueError(f"Upsampling: {n_filters_in} -> {n_filters_out} channels are not served by the fused kernel (input 16, 48 "
                             "or a multiple of 32; output a multiple of 16)")
        self._build([("upk3", nn.Conv3d(n_filters_in, n_filters_out, kernel_size=3, padding=1),
                      _norm_module(normalization, n_filters_out), True,
                      nn.Upsample(scale_factor=stride, mode="trilinear", align_corners=False))])
