"""bf16 parity of the convolution and normalisation kernels at the shapes and batch sizes the package really runs, element-wise
against float64 references computed on the GPU (tests/ref64.py).

csrc/conv.hip picks the kernel, the per-XCD tile remap and the split-K count from B x D x H x W, and csrc/norm.hip picks the
one-launch register-resident form or the three-launch form from the voxel count and the channels per group.  Each row below names
the shape of a real configuration (TrainConfig() default B = 8, the evaluator's 96 x 96 x 64 windows in chunks of 1 to 4, ragged
tile counts of the persistent kernels, the boundaries of the norm forms) and the kernels it exists to cover; the kernel names are
captured from the launches (csrc/ktimer.cpp) so a change of the dispatch that moves a row onto another kernel fails the row.

Every case runs with torch's deterministic fill on: each torch.empty -- outputs, workspaces, split-K slabs -- starts as NaN, so a
partial row or a slab a kernel fails to write poisons the result instead of adding zero.

test_ledger runs one eager step of each configuration the package runs (and the evaluator) with the launches captured: every
kernel of csrc/conv.hip and csrc/norm.hip it launches must be named by a row here or map to an existing test that compares it with a
non-HIP reference (COVERED_ELSEWHERE).
"""
import contextlib
import importlib
import os
import re
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ref64 import conv_ref64, norm_ref64
from test_fullsize_gpu import assert_bf16_elementwise

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import ops
    from dycon_paper_replication_amd._lib import DyconLibraryError
    from test_ops_gpu import mini_engine

DEV = "cuda:0"
BF = torch.bfloat16
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dycon_paper_replication_amd", "csrc")


# ------------------------------------------------------------------------------------------------------------------- fixtures
@pytest.fixture
def poisoned():
    """every torch.empty of the case starts as NaN (torch.utils.deterministic.fill_uninitialized_memory); settings restored after"""
    prev = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled(),
            torch.utils.deterministic.fill_uninitialized_memory)
    torch.use_deterministic_algorithms(True, warn_only=True)
    torch.utils.deterministic.fill_uninitialized_memory = True
    try:
        probe = (torch.empty(4099, device=DEV), torch.empty(4099, dtype=BF, device=DEV), torch.empty(3, 5, dtype=torch.float64, device=DEV))
        assert all(bool(torch.isnan(t).all()) for t in probe), "torch.empty on the GPU does not come back as NaN"
        yield
    finally:
        torch.use_deterministic_algorithms(prev[0], warn_only=prev[1])
        torch.utils.deterministic.fill_uninitialized_memory = prev[2]


@contextlib.contextmanager
def launched(names):
    """kernel timing on for the HIP calls inside the block only; adds the names of the kernels they launched to `names`"""
    prof = ops.KernelProfiler()
    try:
        yield names
        torch.cuda.synchronize()
        names.update(prof.summary())
    finally:
        prof.close()


def _gen(key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, gen, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=gen, device=DEV) * scale + shift


def _nc(t):
    """channels-last -> NCDHW view (assert_bf16_elementwise reports its worst tile in NCDHW coordinates)"""
    return t.permute(0, 4, 1, 2, 3)


def _close_max(got, ref, what, tol=1e-3):
    got, ref = got.double(), ref.double()
    assert bool(torch.isfinite(got).all()), f"{what}: holds NaN / Inf"
    err, scale = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _expect(names, expect, what):
    print(f"{what}: launched {sorted(names)}")
    missing = [k for k in expect if k not in names]
    assert not missing, f"{what}: expected kernels not launched: {missing}; launched {sorted(names)}"


# ------------------------------------------------------------------------------------------------------------------- conv table
# id, kind, B, cin, cout, spatial (input), kernels the row exists to cover (forward, data gradient, weight gradient)
CONV_TABLE = [
    ("c1_ragged_b1", "k3", 1, 1, 16, (50, 44, 46),
     ['conv_k3_c1_kernel<1, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_c1_kernel<false>']),
    ("p16_ragged_b1", "k3", 1, 16, 16, (50, 44, 46),
     ['conv_k3_p16_kernel<2, false, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_bf16_kernel<1, false, 4>']),
    ("p32_b3_remainder", "k3", 3, 32, 32, (56, 56, 40),
     ['conv_k3_p32_kernel<8, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_bf16_kernel<2, false, 4>']),
    ("lds32_b1", "k3", 1, 32, 32, (48, 48, 32),
     ['conv_k3_lds_kernel<32, 2, 4, 4>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_bf16_kernel<2, false, 4>']),
    ("gemm64_b1", "k3", 1, 64, 64, (24, 24, 16),
     ['conv_gemm_kernel<__hip_bfloat16, 1, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("gemm64_b3", "k3", 3, 64, 64, (24, 24, 16),
     ['conv_gemm_kernel<__hip_bfloat16, 1, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("tile128_b1", "k3", 1, 128, 128, (12, 12, 8),
     ['conv_k3_tile_kernel<2>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("tile256_b1", "k3", 1, 256, 256, (6, 6, 4),
     ['conv_k3_tile_kernel<2>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("tile256_b8", "k3", 8, 256, 256, (6, 6, 6),
     ['conv_k3_tile_kernel<2>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("lds64_b8", "k3", 8, 64, 64, (24, 24, 24),
     ['conv_k3_lds_kernel<32, 4, 2, 4>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_bf16_kernel<4, false, 8>']),
    ("p16_96_b8", "k3", 8, 16, 16, (96, 96, 96),
     ['conv_k3_p16_kernel<2, false, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_bf16_kernel<1, false, 4>']),
    ("k2s2_16_b1", "k2s2", 1, 16, 32, (96, 96, 64),
     ['conv_gemm_kernel<__hip_bfloat16, 0, true>', 'conv_gemm_kernel<__hip_bfloat16, 2, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k2s2_bf16_kernel<2>']),
    ("k2s2_128_b1", "k2s2", 1, 128, 256, (12, 12, 8),
     ['conv_gemm_kernel<__hip_bfloat16, 0, true>', 'conv_gemm_kernel<__hip_bfloat16, 2, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k2s2_bf16_kernel<4>']),
    ("deconv256_b1", "deconv", 1, 256, 128, (6, 6, 4),
     ['colsum_kernel<__hip_bfloat16>', 'conv_gemm_kernel<__hip_bfloat16, 0, true>', 'conv_gemm_kernel<__hip_bfloat16, 2, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_k2s2_bf16_kernel<4>']),
    ("deconv32_b3", "deconv", 3, 32, 16, (48, 48, 32),
     ['colsum_kernel<__hip_bfloat16>', 'conv_gemm_kernel<__hip_bfloat16, 0, true>', 'conv_gemm_kernel<__hip_bfloat16, 2, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'reduce_partials_small_kernel', 'wgrad_k2s2_bf16_kernel<2>']),
    ("1x1_256_b1", "1x1", 1, 256, 512, (12, 12, 8),
     ['conv_gemm_kernel<__hip_bfloat16, 0, false>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>', 'wgrad_1x1_bf16_kernel<4>']),
]


@pytest.mark.parametrize("cid,kind,B,cin,cout,sp,expect", CONV_TABLE, ids=[r[0] for r in CONV_TABLE])
def test_conv_dispatch_bf16(poisoned, cid, kind, B, cin, cout, sp, expect):
    gen = _gen(("conv", cid))
    k = {"k3": 3, "k2s2": 2, "deconv": 2, "1x1": 1}[kind]
    wshape = (cin, cout, k, k, k) if kind == "deconv" else (cout, cin, k, k, k)
    w = (_randn(wshape, gen) / float(np.sqrt(cin * k ** 3))).to(BF).float()      # the kernels multiply bf16-rounded weights
    b = _randn((cout,), gen)
    x = _randn((B,) + sp + (cin,), gen).to(BF)
    e = mini_engine({"l.weight": w, "l.bias": b}, BF)
    names = set()
    with launched(names):
        y = e._conv("l", x, kind, need_gx=cin > 1)
        gy = _randn(tuple(y.shape), gen).to(BF)
        e.G[id(y)] = gy
        for fn in reversed(e.tape):
            fn()
    print(f"conv {cid}: launched {sorted(names)}")
    yr, gxr, gwr, gbr = conv_ref64(kind, x, w, b, gy)
    what = f"{kind} {cin}->{cout} @ {sp} B={B}"
    assert_bf16_elementwise(_nc(y), _nc(yr), f"y {what}")
    del yr
    if cin > 1:
        assert_bf16_elementwise(_nc(e.G[id(x)]), _nc(gxr), f"gx {what}")
    del gxr
    _close_max(e.g["l.weight"], gwr, f"gw {what}")
    _close_max(e.g["l.bias"], gbr, f"gb {what}")
    _expect(names, expect, f"conv {cid}")


# ------------------------------------------------------------------------------------------------------------------- norm table
# id, kind, C, spatial, B, mode (relu | skip | norelu | scale | eval), kernels the row exists to cover
NORM_TABLE = [
    # GroupNorm(16), 16 channels per group, across ROWS = 1 / 8 (V = 144, 245, 256 | 257, 294)
    ("gn256_v144_b1", "gn", 256, (6, 6, 4), 1, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 1>', 'norm_sum_dparams_kernel']),
    ("gn256_v245_b3", "gn", 256, (7, 7, 5), 3, "skip",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 1>', 'norm_sum_dparams_kernel']),
    ("gn256_v256_b8", "gn", 256, (8, 8, 4), 8, "norelu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 1>', 'norm_sum_dparams_kernel']),
    ("gn256_v257_b1", "gn", 256, (1, 1, 257), 1, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn128_v294_b3", "gn", 128, (7, 7, 6), 3, "scale",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 8, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 8, false, 8>', 'norm_sum_dparams_kernel']),
    # 8 channels per group, up to and past the one-launch limit (V = 1152, 1960, 2048 | 2049, 2197)
    ("gn128_v1152_b1", "gn", 128, (12, 12, 8), 1, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 8, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 8, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn128_v1960_b3", "gn", 128, (14, 14, 10), 3, "skip",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 8, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 8, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn64_v2048_b8", "gn", 64, (16, 16, 8), 8, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 4, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 4, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn64_v2049_b1", "gn", 64, (3, 683, 1), 1, "relu",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("gn64_v2197_b3", "gn", 64, (13, 13, 13), 3, "norelu",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("gn32_v1152_b8", "gn", 32, (12, 12, 8), 8, "scale",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 2, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 2, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn32_v9216_b1", "gn", 32, (24, 24, 16), 1, "skip",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("gn16_v1960_b1", "gn", 16, (14, 14, 10), 1, "scale",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 8>', 'norm_sum_dparams_kernel']),
    # InstanceNorm (one channel per group)
    ("in256_v144_b8", "in", 256, (6, 6, 4), 8, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 1>']),
    ("in128_v1152_b3", "in", 128, (12, 12, 8), 3, "skip",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 8>']),
    ("in64_v2197_b1", "in", 64, (13, 13, 13), 1, "scale",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("in32_v9216_b1", "in", 32, (24, 24, 16), 1, "relu",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("in16_v245_b3", "in", 16, (7, 7, 5), 3, "norelu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 1>']),
    # BatchNorm: one sample of B x V voxels, on both sides of 2048 through B (6^3 x 8 = 1728 | 6^3 x 10 = 2160)
    ("bn256_b8", "bn", 256, (6, 6, 6), 8, "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 8>', 'norm_sum_dparams_kernel']),
    ("bn256_b10", "bn", 256, (6, 6, 6), 10, "relu",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("bn128_b8_scale", "bn", 128, (6, 6, 6), 8, "scale",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 8>', 'norm_sum_dparams_kernel', 'scale_channels_kernel<__hip_bfloat16>']),
    ("bn64_b10_skip", "bn", 64, (6, 6, 6), 10, "skip",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("bn128_v245_b1", "bn", 128, (7, 7, 5), 1, "norelu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 1>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 1>', 'norm_sum_dparams_kernel']),
    ("bn32_v9216_b1", "bn", 32, (24, 24, 16), 1, "relu",
     ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']),
    ("bn256_eval_b3", "bn", 256, (6, 6, 4), 3, "eval",
     ['norm_apply_kernel<__hip_bfloat16, false>']),
]


@pytest.mark.parametrize("nid,kind,C,sp,B,mode,expect", NORM_TABLE, ids=[r[0] for r in NORM_TABLE])
def test_norm_dispatch_bf16(poisoned, nid, kind, C, sp, B, mode, expect):
    gen = _gen(("norm", nid))
    z = _randn((B,) + sp + (C,), gen, 1.5, 0.3).to(BF)
    affine = kind != "in"
    gamma = _randn((C,), gen, 0.2, 1.0) if affine else None
    beta = _randn((C,), gen, 0.2) if affine else None
    skip = _randn((B,) + sp + (C,), gen).to(BF) if mode == "skip" else None
    cs = (torch.rand(B * C, generator=gen, device=DEV) > 0.5).float() * 2.0 if mode == "scale" else None
    training = mode != "eval"
    e = mini_engine({"n.weight": gamma, "n.bias": beta} if affine else {}, BF)
    run64 = None
    if kind == "bn":
        rm0, rv0 = _randn((C,), gen, 0.1), 1.0 + torch.rand(C, generator=gen, device=DEV)
        e.buf = {"n.running_mean": rm0.clone(), "n.running_var": rv0.clone()}
        run64 = (rm0.double(), rv0.double())
    e.recording = training           # eval-mode BatchNorm (the ISLES teacher) has no backward
    names = set()
    with launched(names):
        y = e._norm("n" if affine else None, z, kind, relu=mode != "norelu", skip=skip, training=training, chan_scale=cs)
        ycopy = y.clone()
        gy = _randn(tuple(y.shape), gen).to(BF)
        if training:
            e.G[id(y)] = gy
            for fn in reversed(e.tape):
                fn()
    print(f"norm {nid}: launched {sorted(names)}")
    yr, gzr, dgr, dbr, _ = norm_ref64(kind, z, gy, gamma, beta, relu=mode != "norelu", skip=skip, chan_scale=cs, running=run64,
                                      training=training)
    what = f"{kind} C={C} @ {sp} B={B} {mode}"
    assert_bf16_elementwise(_nc(ycopy), _nc(yr), f"y {what}")
    if kind == "bn":                 # running statistics: updated in training (unbiased variance), untouched in eval
        for got, ref, nm in ((e.buf["n.running_mean"], run64[0], "running_mean"), (e.buf["n.running_var"], run64[1], "running_var")):
            np.testing.assert_allclose(got.cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=f"{nm} {what}")
    if training:
        assert_bf16_elementwise(_nc(e.G[id(z)]), _nc(gzr), f"gz {what}", acc_noise=2e-3)
        if skip is not None:
            assert torch.equal(e.G[id(skip)], gy), f"gskip {what}: not gy exactly"
        if affine:
            _close_max(e.g["n.weight"], dgr, f"dgamma {what}")
            _close_max(e.g["n.bias"], dbr, f"dbeta {what}")
    _expect(names, expect, f"norm {nid}")


# ------------------------------------------------------------------------------------------------------------------- fused head
# id, spatial, B, with the Dropout3d factor, kernels
HEAD_TABLE = [
    ("head_eval_patch_b1", (96, 96, 64), 1, False,
     ['norm_apply_head_kernel<__hip_bfloat16>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_head_bwd_apply_kernel<__hip_bfloat16>', 'norm_head_finalize_kernel', 'norm_head_partial_kernel<__hip_bfloat16>', 'norm_partial_kernel<__hip_bfloat16, 0>']),
    ("head_96_b8_drop", (96, 96, 96), 8, True,
     ['norm_apply_head_kernel<__hip_bfloat16>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_head_bwd_apply_kernel<__hip_bfloat16>', 'norm_head_finalize_kernel', 'norm_head_partial_kernel<__hip_bfloat16>', 'norm_partial_kernel<__hip_bfloat16, 0>']),
]


@pytest.mark.parametrize("hid,sp,B,drop,expect", HEAD_TABLE, ids=[r[0] for r in HEAD_TABLE])
def test_norm_head_dispatch_bf16(poisoned, hid, sp, B, drop, expect):
    """block_nine's GroupNorm(16) -> ReLU [-> Dropout3d] -> out_conv (16 -> 2) through Engine._norm_head against fp64 autograd"""
    gen = _gen(("head", hid))
    C = 16
    z = _randn((B,) + sp + (C,), gen, 1.5, 0.3).to(BF)
    gamma, beta = _randn((C,), gen, 0.2, 1.0), _randn((C,), gen, 0.2)
    hw, hb = _randn((2, C, 1, 1, 1), gen, 0.4), _randn((2,), gen)
    cs = (torch.rand(B * C, generator=gen, device=DEV) > 0.5).float() * 2.0 if drop else None
    e = mini_engine({"n.weight": gamma, "n.bias": beta, "h.weight": hw, "h.bias": hb}, BF)
    names = set()
    with launched(names):
        logits = e._norm_head("n", z, "gn", "h", training=True, chan_scale=cs)
        lcopy = logits.clone()
        gl = _randn(tuple(logits.shape), gen)
        e.G[id(logits)] = gl
        for fn in reversed(e.tape):
            fn()
    print(f"head {hid}: launched {sorted(names)}")
    zr = z.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    w64, hb64 = hw.double().requires_grad_(True), hb.double().requires_grad_(True)
    a = F.relu(F.group_norm(zr, 16, g64, b64, 1e-5))
    if cs is not None:
        a = a * cs.double().reshape(B, C, 1, 1, 1)
    ref = F.conv3d(a, w64.detach(), hb64.detach())
    # the head's operands are bf16 as in the unfused launches (test_norm_head_fused_equals_norm_then_head: same results): its weight
    # gradient reads the activations rounded to bf16, and dgamma / dbeta read the head's data gradient rounded to bf16.  Those are
    # sums of 1e6 - 1e7 products that each carry one independent rounding (~1e-3 of the sum), so their fp64 reference takes the
    # same two roundings and the bound stays at summation order.  gz is held to the unrounded gradient (element-wise bf16 bound).
    gl64 = gl.double().permute(0, 4, 1, 2, 3)
    aq = a.detach().to(BF).double()
    w64.grad = torch.einsum("bodhw,bcdhw->oc", gl64, aq).reshape(w64.shape)
    hb64.grad = gl64.sum((0, 2, 3, 4))
    gy64 = F.conv3d(gl64, w64.detach().reshape(2, C).t().reshape(C, 2, 1, 1, 1))
    (gz64,) = torch.autograd.grad(a, zr, gy64, retain_graph=True)
    a.backward(gy64.to(BF).double())
    what = f"head @ {sp} B={B}"
    assert lcopy.dtype == torch.float32
    # the logits are fp32, formed from the normalised activations rounded to bf16 (the fused pass rounds them as the stored
    # activation of the unfused launches is rounded): each of the 16 products may carry one bf16 rounding (2^-9, doubled)
    got, r = _nc(lcopy).double(), ref.detach()
    assert bool(torch.isfinite(got).all()), f"logits {what}: holds NaN / Inf"
    bound = 2.0 ** -8 * F.conv3d(a.detach().abs(), w64.detach().abs()) + 2.0 ** -7 * r.abs() + 1e-3 * float(r.pow(2).mean().sqrt())
    excess = (got - r).abs() - bound
    assert float(excess.max()) <= 0, f"logits {what}: {int((excess > 0).sum())} elements off, worst excess {float(excess.max()):.3e}"
    fails = []
    checks = [lambda: assert_bf16_elementwise(_nc(e.G[id(z)]), gz64, f"gz {what}", acc_noise=2e-3)]
    for nm, gt, rf in (("dgamma", e.g["n.weight"], g64.grad), ("dbeta", e.g["n.bias"], b64.grad),
                       ("head gw", e.g["h.weight"], w64.grad), ("head gb", e.g["h.bias"], hb64.grad)):
        checks.append(lambda gt=gt, rf=rf, nm=nm: _close_max(gt, rf, f"{nm} {what}"))
    for c in checks:                 # (every gradient reported, not only the first that fails)
        try:
            c()
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "; ".join(fails)
    _expect(names, expect, f"head {hid}")


# ------------------------------------------------------------------------------------------------------------------- first block
FIRST_BLOCK = [(16, ['conv_k3_c1_kernel<1, false>', 'first_block_bwd_kernel', 'first_block_finalize_kernel', 'first_block_reduce_kernel', 'norm_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'pack_bfrag_kernel<__hip_bfloat16>']),
               (17, ['conv_k3_c1_kernel<1, false>', 'norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel', 'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>', 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'wgrad_k3_c1_kernel<false>'])]


@pytest.mark.parametrize("B,expect", FIRST_BLOCK, ids=["b16_one_pass", "b17_unfused"])
def test_first_block_dispatch_bf16(poisoned, B, expect):
    """V-Net block_one (conv 1 -> 16, GroupNorm(16), ReLU) at 24 x 24 x 28: B = 16, the limit of dycon_first_block_bwd, runs
    Engine._first_block; at B = 17 the engine's guard must take the unfused path (conv, norm, stored data gradient, weight gradient).
    Both against fp64 on the same bf16 convolution output."""
    gen = _gen(("first", B))
    sp, C = (24, 24, 28), 16
    w = (_randn((C, 1, 3, 3, 3), gen) / float(np.sqrt(27))).to(BF).float()
    b = _randn((C,), gen, 0.1)
    gamma, beta = _randn((C,), gen, 0.2, 1.0), _randn((C,), gen, 0.2)
    e = mini_engine({"block_one.conv.0.weight": w, "block_one.conv.0.bias": b,
                     "block_one.conv.1.weight": gamma, "block_one.conv.1.bias": beta}, BF)
    x = _randn((B,) + sp + (1,), gen).to(BF)
    fused = e._fuses_first_block(x, "gn", True)
    assert fused == (B <= 16)
    names = set()
    with launched(names):
        if fused:
            y = e._first_block("block_one", x, "gn", True)
        else:
            z = e._conv("block_one.conv.0", x, "k3", need_gx=False, norm_groups=16)
            y = e._norm("block_one.conv.1", z, "gn")
        ycopy = y.clone()
        gy = _randn(tuple(y.shape), gen).to(BF)
        e.G[id(y)] = gy
        for fn in reversed(e.tape):
            fn()
    print(f"first block B={B}: launched {sorted(names)}")
    assert ("first_block_bwd_kernel" in names) == fused
    what = f"first block B={B}"
    # the convolution's bf16 output (the same deterministic launch again): against fp64 here, and the input of the fp64 norm below,
    # so the reference of the normalisation sees the same stored values the block normalised
    e.recording = False
    zq = e._conv("block_one.conv.0", x, "k3", need_gx=False)
    zc, _, _, _ = conv_ref64("k3", x, w, b, torch.zeros(B, *sp, C, device=DEV))
    assert_bf16_elementwise(_nc(zq), _nc(zc), f"z {what}")
    del zc
    yr, gzr, dgr, dbr, _ = norm_ref64("gn", zq, gy, gamma, beta)
    _, _, gwr, gbr = conv_ref64("k3", x, w, b, gzr)
    assert_bf16_elementwise(_nc(ycopy), _nc(yr), f"y {what}")
    # one pass: the norm's data gradient is never rounded, so dW is fp32 accumulation only (the bound of
    # test_first_block_backward_in_one_pass); unfused, dW is formed from the bf16-stored data gradient (the bound of
    # test_first_layer_wgrad_with_norm_backward_on_load)
    _close_max(e.g["block_one.conv.0.weight"], gwr, f"gw {what}", 2e-4 if fused else 2e-3)
    # sum(gz) is ~0 analytically (one channel per group): held on the scale of the terms that cancel in it
    scale_b = float(gzr.abs().sum((0, 1, 2, 3)).max())
    err_b = float((e.g["block_one.conv.0.bias"].double() - gbr).abs().max())
    assert err_b <= (1e-5 if fused else 1e-4) * scale_b, (err_b, scale_b)
    _close_max(e.g["block_one.conv.1.weight"], dgr, f"dgamma {what}")
    _close_max(e.g["block_one.conv.1.bias"], dbr, f"dbeta {what}")
    _expect(names, expect, what)


def test_first_block_bwd_refuses_17_samples():
    """dycon_first_block_bwd takes at most 16 samples: B = 17 is refused by the argument check, before anything is launched"""
    B, sp, C = 17, (4, 4, 4), 16
    x = torch.zeros(B, *sp, 1, dtype=BF, device=DEV)
    z = torch.zeros(B, *sp, C, dtype=BF, device=DEV)
    stats = torch.zeros(B * 16 * 2, device=DEV)
    gw, gb = torch.zeros(C, 1, 3, 3, 3, device=DEV), torch.zeros(C, device=DEV)
    ws = torch.zeros(1 << 20, device=DEV)
    torch.cuda.synchronize()
    prof = ops.KernelProfiler()
    try:
        with pytest.raises(DyconLibraryError, match="B <= 16"):
            ops.first_block_bwd(x, z, z, stats, B, 16, gw, gb, ws=ws)
        assert prof.count() == 0
    finally:
        prof.close()


# ------------------------------------------------------------------------------------------------------------------- ledger
def _declared_kernels():
    out = set()
    for f in ("conv.hip", "norm.hip"):
        src = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src):
            out.add(m.group(1))
    return out


# kernels of csrc/conv.hip / csrc/norm.hip that the configurations launch and that an EXISTING test compares with a non-HIP reference
COVERED_ELSEWHERE = {
    "conv_k3_halo_kernel<1>": "test_conv_small_gpu::test_halo_conv_forward",               # 12^3, 128 channels, B = 8 / 16
    "conv_k3_halo_kernel<2>": "test_conv_small_gpu::test_halo_conv_forward",               # ... B = 4, 256 output columns
    "conv_k3_lds_kernel<32, 4, 4, 8>": "test_fullsize_gpu::test_conv_full_size_bf16",      # 64 -> 64 @ 24^3, B = 4
    # U-Net widths (16 / 32 / 48 / 96 channels) on the LDS kernel, bf16 against F.conv3d
    "conv_k3_lds_kernel<16, 1, 4, 4>": "test_ops_gpu::test_conv",
    "conv_k3_lds_kernel<16, 2, 4, 4>": "test_ops_gpu::test_conv",
    "conv_k3_lds_kernel<16, 3, 4, 4>": "test_ops_gpu::test_conv",
    "conv_k3_lds_kernel<32, 1, 4, 4>": "test_ops_gpu::test_conv",
    "conv_k3_lds_kernel<32, 3, 4, 4>": "test_ops_gpu::test_conv",
    # the U-Net's 16 -> 2 head with fp32 logits (conv_direct), its weight / bias gradient and its weight packing: ("1x1", 16, 2) in bf16
    "head_1x1_fwd_kernel<__hip_bfloat16, 16, 2>": "test_ops_gpu::test_conv",
    "head_1x1_bwd_kernel<__hip_bfloat16, 2, 16>": "test_ops_gpu::test_conv",
    "wgrad_1x1_skinny_kernel<__hip_bfloat16, float, 16, 2>": "test_ops_gpu::test_conv",
    "colsum_kernel<float>": "test_ops_gpu::test_conv",
    "pack_tcn_kernel": "test_ops_gpu::test_conv",
    # every weight repacked in one launch by the module route (nn.Module forward), against the CPU evaluator
    "pack_batch_kernel": "test_eval_gpu::test_single_case_matches_oracle",
}


def _rows_expect():
    rows = [r[-1] for r in CONV_TABLE] + [r[-1] for r in NORM_TABLE] + [r[-1] for r in HEAD_TABLE] + [r[-1] for r in FIRST_BLOCK]
    return {k for ex in rows for k in ex}


LEDGER = [
    ("vnet_gn_96_b4", dict(model="vnet"), (96, 96, 96), 4),
    ("vnet_gn_96_b8", dict(model="vnet"), (96, 96, 96), 8),
    ("vnet_gn_112x112x96_b4", dict(model="vnet"), (112, 112, 96), 4),
    ("isles_112x112x80_b4", dict(model="vnet", dice_variant="multiclass", teacher_mode="eval", poly_lr=True, feature_scaler=4),
     (112, 112, 80), 4),
    ("isles_96x96x64_b8", dict(model="vnet", dice_variant="multiclass", teacher_mode="eval", poly_lr=True, feature_scaler=4),
     (96, 96, 64), 8),
    ("unet_96_b4", dict(model="unet_3D"), (96, 96, 96), 4),
    ("eval_96x96x64", None, (96, 96, 64), 4),
]


def _launched_by(cfg, kw, patch, B):
    names = set()
    if kw is None:                   # the evaluator: bf16 V-Net, windows of 96 x 96 x 64 in chunks of 4 -> last chunks of 1 and 3
        from dycon_paper_replication_amd.networks.net_factory_3d import net_factory_3d
        from dycon_paper_replication_amd.utils import test_3d_patch as T3
        model = net_factory_3d("vnet", 1, 2, 2, dtype=BF).cuda()
        for depth in (80, 88):       # 5 and 7 windows along z (stride 4)
            image = np.random.default_rng(depth).standard_normal((96, 96, depth)).astype(np.float32)
            with launched(names):
                T3.test_single_case(model, image, 16, 4, patch, num_classes=2, batch_size=B)
        return names
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    tr = DyconTrainer(TrainConfig(batch_size=B, labeled_bs=B // 2, replay=False, **kw), DEV)
    vol, lab, _ = make_batch(5, B, patch)
    with launched(names):
        tr.step(vol.to(DEV), lab.to(DEV), epoch=0)
    del tr
    torch.cuda.empty_cache()
    return names


@pytest.mark.parametrize("cfg,kw,patch,B", LEDGER, ids=[r[0] for r in LEDGER])
def test_ledger(cfg, kw, patch, B):
    declared = _declared_kernels()
    assert {"conv_k3_p16_kernel", "conv_k3_halo_kernel", "norm_fused_fwd_kernel", "first_block_bwd_kernel"} <= declared, sorted(declared)
    for kname, test_id in COVERED_ELSEWHERE.items():
        mod, fn = test_id.split("::")
        assert hasattr(importlib.import_module(mod), fn), f"{kname}: {test_id} does not exist"
    launched_names = _launched_by(cfg, kw, patch, B)
    in_scope = sorted(n for n in launched_names if re.match(r"\w+", n).group(0) in declared)
    print(f"ledger {cfg}: {len(in_scope)} conv / norm kernels: {in_scope}")
    covered = _rows_expect() | set(COVERED_ELSEWHERE)
    missing = [n for n in in_scope if n not in covered]
    assert not missing, f"{cfg}: launched without a parity case: {missing}"
