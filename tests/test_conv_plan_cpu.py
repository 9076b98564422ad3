"""CPU tests of the forward-convolution plan (csrc/conv.hip conv_fwd_plan, read through dycon_conv_gemm_plan / ops.conv_plan) and of
the weight-gradient workspace query: pure host code, no GPU.

tests/golden/conv_plans.json holds what the four older queries answered over plan_grid() at the last commit where each of them
walked its own copy of the dispatch conditions (tests/golden/make_golden_conv_plans.py).  The answers must not have moved, with one
class of exception: shapes the launch serves with a kernel that splits nothing (c1, p16, p32, lds), where the old split / workspace
queries nevertheless reported split-K slabs."""
import ctypes
import itertools
import json
import os

import pytest

from conftest import GOLDEN
from dycon_paper_replication_amd import _lib, ops
from dycon_paper_replication_amd._lib import (BF16, CONV_1X1, CONV_C1, CONV_GEMM, CONV_HALO, CONV_K2S2, CONV_K3, CONV_LDS, CONV_NONE,
                                              CONV_P16, CONV_P32, CONV_TILE, CONV_W_CHUNK16, CONV_W_FRAG, F32)
from test_conv_small_gpu import CASES as SMALL_CASES
from test_dispatch_parity_gpu import CONV_TABLE

QUERIES = ("dycon_conv_gemm_workspace", "dycon_conv_gemm_splits", "dycon_conv_stats_chunks", "dycon_conv_wgrad_workspace")
SPATIAL = [(4, 4, 4), (6, 6, 6), (6, 6, 4), (12, 12, 12), (12, 12, 8), (14, 14, 10), (24, 24, 16), (24, 24, 24), (48, 48, 32),
           (48, 48, 48), (50, 44, 46), (56, 56, 40), (96, 96, 64), (96, 96, 96)]
CHANNELS = [(1, 16), (1, 32), (16, 16), (16, 32), (32, 32), (32, 64), (48, 48), (48, 96), (64, 64), (64, 128), (128, 128), (128, 256),
            (256, 256), (16, 2)]
MODES = [(CONV_1X1, 0), (CONV_1X1, 1), (CONV_K3, 0), (CONV_K2S2, 0)]      # scatter is legal with 1x1 only
LDS_MIN_VOXELS = 24 ** 3
SLABLESS = (CONV_C1, CONV_P16, CONV_P32, CONV_LDS)


def plan_grid():
    """(dtype, mode, scatter, B, D, H, W, Cin, Cout) rows, in the order of the fixture"""
    for dtype, (mode, scatter), B, sp, (cin, cout) in itertools.product((F32, BF16), MODES, (1, 2, 3, 4, 8), SPATIAL, CHANNELS):
        yield (dtype, mode, scatter, B) + sp + (cin, cout)


def wgrad_grid():
    """the rows of plan_grid() that differ in an argument of dycon_conv_wgrad_workspace (no dtype, no scatter)"""
    return [s for s in plan_grid() if s[0] == F32 and s[2] == 0]


def ask(lib, shape):
    """the four older queries for one row of plan_grid() (a scatter has N = 8 * Cout columns)"""
    dtype, mode, scatter, B, D, H, W, cin, cout = shape
    N = 8 * cout if scatter else cout
    return (lib.dycon_conv_gemm_workspace(dtype, mode, scatter, B, D, H, W, cin, N),
            lib.dycon_conv_gemm_splits(dtype, mode, scatter, B, D, H, W, cin, N),
            lib.dycon_conv_stats_chunks(dtype, mode, B, D, H, W, cin, cout),
            lib.dycon_conv_wgrad_workspace(mode, B, D, H, W, cin, cout))


def _plan(shape):
    dtype, mode, scatter, B, D, H, W, cin, cout = shape
    return ops.conv_plan(dtype, mode, scatter, 0, B, D, H, W, cin, 8 * cout if scatter else cout, cout)


def test_query_answers_unchanged():
    lib = _lib.load()
    gold = json.load(open(os.path.join(GOLDEN, "conv_plans.json")))
    grid, wgrid = list(plan_grid()), wgrad_grid()
    assert (gold["rows"], gold["wgrad_rows"]) == (len(grid), len(wgrid)) == (len(gold["splits"]), len(gold["wgrad_workspace"]))
    wgrad = {s[1:2] + s[3:]: v for s, v in zip(wgrid, gold["wgrad_workspace"])}
    rows = [s + (w, n, c, wgrad[s[1:2] + s[3:]]) for s, w, n, c in zip(grid, gold["workspace"], gold["splits"], gold["chunks"])]
    changed, wrong = [], []
    for r in rows:
        shape, old = tuple(r[:9]), tuple(r[9:])
        new, plan = ask(lib, shape), _plan(shape)
        assert (plan.workspace, plan.splits) == new[:2], shape        # the queries are fields of the plan
        if new == old:
            continue
        # the one exception: a kernel without slabs, where the old queries reported some -- now 1 split and no workspace
        if plan.family in SLABLESS and (old[1] > 1 or old[0] > 0) and new[:2] == (0, 1) and new[2:] == old[2:]:
            changed.append((shape, old))
        else:
            wrong.append((shape, old, new, plan))
    assert not wrong, wrong[:5]
    assert changed, "no LDS-served shape with slabs in the fixture"
    assert ((BF16, CONV_K3, 0, 1, 24, 24, 24, 128, 128), (21233664, 3)) in [(s, o[:2]) for s, o in changed]
    for shape, _ in changed:
        assert shape[4] * shape[5] * shape[6] >= LDS_MIN_VOXELS, shape
        assert _plan(shape).family not in (CONV_HALO, CONV_TILE, CONV_GEMM), shape


# every forward entry of tests/test_dispatch_parity_gpu.py CONV_TABLE (kind, B, cin, cout, spatial, the kernels the row lists), plus
# the shapes of tests/test_conv_small_gpu.py CASES (the one-launch kernel of the small levels) and the first layer at 96^3
FORWARD = [r[1:] for r in CONV_TABLE] + [("k3", B, cin, cout, sp, ["conv_k3_halo_kernel"]) for B, cin, cout, sp in SMALL_CASES] + [
    ("k3", 4, 1, 16, (96, 96, 96), ["conv_k3_c1_kernel"])]


@pytest.mark.parametrize("kind,B,cin,cout,sp,kernels", FORWARD, ids=[r[0] for r in CONV_TABLE] + [None] * (len(SMALL_CASES) + 1))
def test_family_names_the_launched_kernel(kind, B, cin, cout, sp, kernels):
    mode = {"k3": CONV_K3, "k2s2": CONV_K2S2, "deconv": CONV_1X1, "1x1": CONV_1X1}[kind]
    scatter = int(kind == "deconv")
    plan = ops.conv_plan(BF16, mode, scatter, 0, B, *sp, cin, 8 * cout if scatter else cout, cout)
    name = _lib.load().dycon_conv_kernel_name(plan.family).decode()
    if plan.family == CONV_GEMM:      # a k2s2 / deconv row also lists its data gradient's generic kernel: the forward one, by its arguments
        assert f"conv_gemm_kernel<__hip_bfloat16, {mode}, {'true' if scatter else 'false'}>" in kernels, (plan, kernels)
    else:
        fwd = [k for k in kernels if k.startswith("conv_")]
        assert len(fwd) == 1 and fwd[0].startswith(name + "_kernel"), (plan, name, kernels)
    if plan.family == CONV_HALO:
        assert (plan.splits, plan.workspace) == (1, 0)
    assert plan.name == (name + "_splitk" if plan.family == CONV_GEMM and plan.splits > 1 else name)


def test_plan_corners():
    none = ops.conv_plan(BF16, CONV_K3, 0, 0, 2, 12, 12, 12, 1, 16, 16)        # one input channel below 24^3: dycon_conv_direct's
    assert none.family == CONV_NONE
    # k2s2 with odd dimensions, a dimension of 1 (no output rows) included, and shapes that are no shapes: refused, nothing divides by zero
    for shape in [(1, 1, 4, 4), (1, 4, 4, 1), (2, 3, 4, 4), (1, 1, 1, 1), (0, 4, 4, 4), (1, 4, -2, 4)]:
        for dtype, cin in ((BF16, 64), (F32, 16)):
            refused = ops.conv_plan(dtype, CONV_K2S2, 0, 0, *shape, cin, 64, 64)
            assert (refused.family, refused.name) == (CONV_NONE, "none"), (shape, refused)
            assert _lib.load().dycon_conv_gemm_splits(dtype, CONV_K2S2, 0, *shape, cin, 64) >= 1
    null = ctypes.c_void_p(8)         # never dereferenced: the argument checks come before the plan and any launch
    rc = _lib.load().dycon_conv_gemm(null, null, null, null, BF16, CONV_K2S2, 0, 0, 1, 1, 4, 4, 64, 64, 64, None, 0, None)
    assert rc != 0 and b"k2s2 needs even dims" in _lib.load().dycon_last_error()
    assert ops.conv_plan(BF16, CONV_K3, 0, 0, 2, 24, 24, 24, 1, 16, 16).family == CONV_C1
    assert ops.conv_plan(BF16, CONV_K3, 0, 0, 2, 48, 48, 48, 48, 96, 96).weights == CONV_W_CHUNK16
    assert ops.conv_plan(BF16, CONV_K3, 0, 0, 2, 12, 12, 12, 48, 96, 96).weights == CONV_W_FRAG
    # statistics: the persistent kernels only, and not while accumulating
    p32 = ops.conv_plan(BF16, CONV_K3, 0, 0, 3, 56, 56, 40, 32, 32, 32)
    assert (p32.family, p32.chunks, p32.splits, p32.workspace) == (CONV_P32, 256, 1, 0)
    acc = ops.conv_plan(BF16, CONV_K3, 0, 1, 3, 56, 56, 40, 32, 32, 32)
    assert (acc.family, acc.chunks) == (CONV_LDS, 0)
    assert ops.conv_plan(BF16, CONV_K3, 0, 0, 4, 96, 96, 96, 16, 16, 16).chunks > 0
    assert ops.conv_plan(BF16, CONV_K3, 0, 1, 4, 96, 96, 96, 16, 16, 16).chunks == 0
    assert ops.conv_plan(F32, CONV_K3, 0, 0, 4, 96, 96, 96, 16, 16, 16).family == CONV_GEMM


def test_wgrad_names():
    lib = _lib.load()
    name = lambda xd, gd, mode, B, sp, cin, cout: lib.dycon_conv_wgrad_name(xd, gd, mode, B, *sp, cin, cout).decode()   # noqa: E731
    assert name(BF16, BF16, CONV_K3, 1, (50, 44, 46), 1, 16) == "wgrad_k3_c1"
    assert name(BF16, BF16, CONV_K3, 1, (24, 24, 16), 64, 64) == "wgrad_k3_bf16"
    assert name(BF16, BF16, CONV_K3, 1, (24, 24, 16), 1, 32) == "wgrad_k3_bf16"
    assert name(BF16, BF16, CONV_K2S2, 1, (12, 12, 8), 128, 256) == "wgrad_k2s2_bf16"
    assert name(BF16, BF16, CONV_1X1, 1, (12, 12, 8), 256, 512) == "wgrad_1x1_bf16"
    assert name(BF16, F32, CONV_1X1, 1, (12, 12, 8), 16, 2) == "wgrad_1x1_skinny"
    assert name(F32, F32, CONV_K3, 1, (12, 12, 8), 64, 64) == "conv_wgrad"
    assert name(F32, F32, CONV_K3, 1, (12, 12, 8), 1, 16) == "conv_wgrad_direct"
