"""Tap planning and the stand-alone dilated convolution of the 3-D ASPP (networks/assp.py:28-82).

A k=3 convolution with dilation = padding = d on a grid of extents (D, H, W) reads real data through an off-centre offset +-d of
an axis only if d < that extent; every other tap multiplies zero padding.  The live taps are therefore the product over the axes
of {0} u {+-d : d < n}, derived from the shape alone.  At the bottleneck grids the project trains on:

    6 x 6 x 6, 6 x 6 x 4   every dilated branch (d = 6, 12, 18) is its centre tap: a 1x1 convolution
    7 x 7 x 5, 7 x 7 x 6   d = 6 keeps 9 taps (3 x 3 in the D-H plane), d = 12 and 18 are centre-only

A TapPlan lays the branches that read one input out as ONE GEMM on the 1x1 MFMA path (ops.conv_gemm): the K axis is a list of
blocks, each the input shifted by one live offset (block 0: the input itself, shared by every branch's centre tap), and the N
axis has one block per branch.  Block (k, n) holds branch n's weights at the tap of offset k, or zeros.  The data gradient is
the same construction on the output gradient shifted by the negated offsets, with the transposed taps.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import torch

from . import ops
from ._lib import CONV_1X1

ASPP_DILATIONS = (1, 6, 12, 18)              # ASPP3D(output_stride=16), assp.py:31-32
ASPP_BRANCHES = ((1, 1), (3, 6), (3, 12), (3, 18))   # (kernel size, dilation) of aspp1..aspp4


def live_taps(dhw: Sequence[int], d: int) -> List[Tuple[int, int, int, int]]:
    """[(torch tap index, dz, dy, dx)] of a k=3 convolution with dilation = padding = d on a (D, H, W) grid that can touch data:
    the centre first, then the others in torch's tap order."""
    if int(d) < 1:
        raise ValueError(f"dilation must be >= 1, got {d}")
    d = int(d)
    axes = [{0} | ({-d, d} if d < int(n) else set()) for n in dhw]
    taps = []
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                o = ((kz - 1) * d, (ky - 1) * d, (kx - 1) * d)
                if all(o[a] in axes[a] for a in range(3)):
                    taps.append((kz * 9 + ky * 3 + kx,) + o)
    return sorted(taps, key=lambda t: (t[0] != 13, t[0]))


class TapPlan:
    """K-block layout of the branches (kernel size 1 or 3, dilation) that read one (B, D, H, W, Ci) input (module docstring)."""

    def __init__(self, dhw: Sequence[int], branches: Sequence[Tuple[int, int]]):
        self.dhw = tuple(int(n) for n in dhw)
        self.branches = tuple((int(k), int(d)) for k, d in branches)
        self.offsets = [(0, 0, 0)]
        self.kb = []                     # per branch: {tap index in its weight: k block}
        for k, d in self.branches:
            if k == 1:
                self.kb.append({0: 0})
                continue
            if k != 3:
                raise ValueError("branches are 1x1x1 or 3x3x3 convolutions")
            m = {}
            for tap, dz, dy, dx in live_taps(self.dhw, d):
                if (dz, dy, dx) == (0, 0, 0):
                    m[tap] = 0
                else:
                    m[tap] = len(self.offsets)
                    self.offsets.append((dz, dy, dx))
            self.kb.append(m)
        self.KB, self.NB = len(self.offsets), len(self.branches)
        self.T = [1 if k == 1 else 27 for k, _ in self.branches]
        self.taps_host = ops.host_array(C.c_int, [v for o in self.offsets for v in o])
        self.neg_taps_host = ops.host_array(C.c_int, [-v for o in self.offsets for v in o])

    def live(self, j):
        """sorted torch tap indices that branch j keeps"""
        return sorted(self.kb[j])

    def _blk(self):
        """block (kb, j) = branch j's tap at offset kb, or -1: the forward's (offset x branch) grid, and the data gradient's K blocks
        ([offset][branch] channels of the gathered output gradient)"""
        blk = [-1] * (self.KB * self.NB)
        for j, m in enumerate(self.kb):
            for tap, kb in m.items():
                blk[kb * self.NB + j] = j * 32 + tap
        return ops.host_array(C.c_short, blk)

    def fwd_tables(self, ws, Ci):
        """ops.pack_wblocks tables of B (KB*Ci x NB*Co): element (kb*Ci + ci, j*Co + co) = w_j[co][ci][tap]"""
        w_host = ops.host_array(C.c_void_p, [w.data_ptr() for w in ws])
        strides = ops.host_array(C.c_longlong, [v for T in self.T for v in (T, Ci * T)])
        return (w_host, strides, self.NB, self._blk())

    def dgrad_tables(self, ws, Ci):
        """ops.pack_wblocks tables of the data gradient's B (KB*NB*Co x Ci): the output gradient gathered at the NEGATED offsets
        ([offset][branch][co] columns) times each branch's transposed tap -- one fp32 accumulation, one rounding"""
        w_host = ops.host_array(C.c_void_p, [w.data_ptr() for w in ws])
        strides = ops.host_array(C.c_longlong, [v for T in self.T for v in (Ci * T, T)])
        return (w_host, strides, self.NB, self._blk())

    def unpack_tables(self, gs):
        g_host = ops.host_array(C.c_void_p, [g.data_ptr() for g in gs])
        taps = ops.host_array(C.c_int, list(self.T))
        kb = [-1] * (27 * self.NB)
        for j, m in enumerate(self.kb):
            for tap, b in m.items():
                kb[j * 27 + tap] = b
        return (g_host, taps, ops.host_array(C.c_short, kb), self.NB)


def _check(x, w):
    if x.dim() != 5 or not x.is_contiguous():
        raise ValueError("x must be a contiguous (B, D, H, W, Ci) tensor")
    if tuple(w.shape[1:]) != (x.shape[-1], 3, 3, 3) or w.dtype != torch.float32 or not w.is_contiguous():
        raise ValueError(f"w must be a contiguous fp32 (Co, {x.shape[-1]}, 3, 3, 3) tensor, got {tuple(w.shape)}")


def dilated_conv3d(x, w, d):
    """F.conv3d(x, w, dilation=d, padding=d) without bias on NDHWC activations (fp32 / bf16 storage, fp32 weights)."""
    _check(x, w)
    Co, Ci = w.shape[:2]
    plan = TapPlan(x.shape[1:4], [(3, d)])
    wf = ops.pack_wblocks(plan.fwd_tables([w], Ci), plan.KB, 1, Ci, Co, x.dtype, x.device)
    a = x if plan.KB == 1 else ops.tap_gather(x, plan.taps_host, plan.KB)
    return ops.conv_gemm(a, wf, None, CONV_1X1, Co, Co)


def dilated_conv3d_bwd_data(gy, w, d):
    """data gradient of dilated_conv3d: (B, D, H, W, Co) -> (B, D, H, W, Ci)"""
    Co, Ci = w.shape[:2]
    if gy.dim() != 5 or gy.shape[-1] != Co:
        raise ValueError("gy must be (B, D, H, W, Co)")
    plan = TapPlan(gy.shape[1:4], [(3, d)])
    wd = ops.pack_wblocks(plan.dgrad_tables([w], Ci), plan.KB, 1, Co, Ci, gy.dtype, gy.device)
    a = gy if plan.KB == 1 else ops.tap_gather(gy, plan.neg_taps_host, plan.KB)
    return ops.conv_gemm(a, wd, None, CONV_1X1, Ci, Ci)


def dilated_conv3d_bwd_weight(x, gy, d, gw=None):
    """weight gradient of dilated_conv3d into gw (Co, Ci, 3, 3, 3) fp32 (written, zeros on the pruned taps)"""
    Ci, Co = x.shape[-1], gy.shape[-1]
    if gw is None:
        gw = torch.empty((Co, Ci, 3, 3, 3), dtype=torch.float32, device=x.device)
    plan = TapPlan(x.shape[1:4], [(3, d)])
    a = x if plan.KB == 1 else ops.tap_gather(x, plan.taps_host, plan.KB)
    dense = torch.empty(plan.KB * Ci * Co, dtype=torch.float32, device=x.device)
    ops.conv_wgrad(a, gy, dense, CONV_1X1, 0, Co, 1)
    ops.unpack_wgrad(dense, Co, plan.KB, plan.unpack_tables([gw]), Ci, Co)
    return gw
