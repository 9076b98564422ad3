"""Guard-band tests, op level: no kernel reads or writes outside its tensors.

Every row runs its op (forward and backward through mini_engine / ops) inside tests/guard.py's guarded(): inputs, labels and
weights are wrap()ped, and every output, workspace, split-K slab and packed weight the package allocates gets 0xFF bands too.  Then
  (a) check(): every band is intact (no write past either end);
  (b) every result is finite and within the project's existing bound of the fp64 reference (a read past the end that reaches the
      arithmetic meets NaN);
  (c) the same call on ordinary tensors gives the same bits (the loss sums, double atomics: 1e-6 relative);
  (d) the kernels the row exists for were launched (names captured from the launches, as in test_dispatch_parity_gpu.CONV_TABLE).
The shapes are the smallest that reach each kernel family (confirmed with ops.conv_plan) with partial tiles on every axis.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from guard import guarded
from ref64 import conv_ref64, norm_ref64
from test_fullsize_gpu import assert_bf16_elementwise
from test_gambling_cpu import uncertainty_ref

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import _lib, ops
    from test_dispatch_parity_gpu import _close_max, _nc, launched
    from test_ops_gpu import close, mini_engine, relclose
from oracle import losses as OL

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32


# ------------------------------------------------------------------------------------------------------------------- helpers
def _gen(key):
    return torch.Generator(device=DEV).manual_seed(zlib.crc32(repr(key).encode()))


def _randn(shape, gen, scale=1.0, shift=0.0):
    return torch.randn(shape, generator=gen, device=DEV) * scale + shift


def _plain(t):
    return None if t is None else t.clone()


def _engine(params, dtype, wrap):
    """mini_engine whose parameters and gradient buffers went through `wrap` (guarded: both get bands)"""
    e = mini_engine(params, dtype)
    e.p = {k: wrap(v) for k, v in e.p.items()}
    e.g = {k: wrap(v) for k, v in e.g.items()}
    return e


def run_both(run, what):
    """run(wrap) -> {name: tensor} once inside guarded() with the launches captured, once on ordinary tensors.
    Returns (kernel names, guarded results, ordinary results) after assertion (a)."""
    names = set()
    with guarded() as g:
        with launched(names):
            got = run(g.wrap)
    n = g.check()                                                # (a)
    print(f"{what}: {n} guarded allocations checked; launched {sorted(names)}")
    plain = run(_plain)
    torch.cuda.synchronize()
    assert sorted(got) == sorted(plain)
    return names, got, plain


def assert_finite_under_guard(got, plain, what):
    for k, a in got.items():
        if a is None or not a.is_floating_point():
            continue
        bad = int((~torch.isfinite(a.float())).sum())
        if bad:
            clean = bool(torch.isfinite(plain[k].float()).all())
            raise AssertionError(f"{what} {k}: {bad} of {a.numel()} elements are NaN / Inf under the guard" +
                                 (" but none on ordinary tensors: an out-of-bounds read reached the arithmetic" if clean else
                                  " and on ordinary tensors too"))


def assert_same_bits(got, plain, what):
    """(c) for the deterministic ops"""
    assert_finite_under_guard(got, plain, what)
    for k, a in got.items():
        b = plain[k]
        assert (a is None) == (b is None), f"{what} {k}"
        if a is not None:
            assert a.dtype == b.dtype and torch.equal(a, b), \
                f"{what} {k}: {int((a != b).sum())} of {a.numel()} elements differ from the same call on ordinary tensors"


def assert_same_1e6(got, plain, what):
    """(c) for the ops that sum with double atomics: the 1e-6 relative bound of test_checkpoint_resume_continues_the_run"""
    assert_finite_under_guard(got, plain, what)
    for k, a in got.items():
        b = plain[k]
        if a is not None:
            assert float((a.double() - b.double()).abs().max()) <= 1e-6 * float(b.double().abs().max()), f"{what} {k}"


def expect(names, want, what):
    """(d): an entry with template arguments must have been launched as written, a bare name in any instantiation"""
    bases = {n.split("<")[0].split("::")[-1] for n in names}
    missing = [k for k in want if (k not in names if "<" in k else k not in bases)]
    assert not missing, f"{what}: expected kernels not launched: {missing}; launched {sorted(names)}"


def test_guard_on_the_device():
    """the helper on CUDA tensors: requests are guarded, poisoned and aligned as documented (its detection is shown on the CPU,
    tests/test_guard_cpu.py: nothing here writes outside a tensor)"""
    with guarded() as g:
        a = torch.empty((2, 3, 5, 7, 16), dtype=BF, device=DEV)
        b = torch.empty_like(a, dtype=torch.float64)
        c = torch.empty(9, dtype=torch.int32, device=torch.device(DEV))
        d = torch.empty(4099, dtype=torch.uint8, device="cuda")
        z = torch.zeros(1000, dtype=F32, device=DEV)
        h = torch.empty(5)                                   # host tensors pass through
        w = g.wrap(torch.arange(6, device=DEV))
        assert len(g.allocs) == 6 and h.device.type == "cpu"
        assert all(bool(torch.isnan(t.float()).all()) for t in (a, b)) and bool((c == -1).all()) and bool((d == 255).all())
        assert float(z.abs().max()) == 0 and torch.equal(w, torch.arange(6, device=DEV))
        assert all(t.data_ptr() % 512 == 0 and t.is_contiguous() for t in (a, b, c, d, z, w))
        for rec in g.allocs:
            assert bool((rec.base[:rec.band] == 0xFF).all()) and bool((rec.base[rec.band + rec.nbytes:] == 0xFF).all())
        a.zero_()
        d.fill_(3)
        assert g.check() == 6
    assert torch.empty(3, device=DEV).untyped_storage().nbytes() == 12 and len(g.allocs) == 6      # the originals are back


# ------------------------------------------------------------------------------------------------------------------- conv table
PK, RP, FIN = 'pack_bfrag_kernel<__hip_bfloat16>', 'reduce_partials_kernel<4>', 'splitk_finish_kernel<__hip_bfloat16>'
GEMM_K3, GEMM_K2, GEMM_SC, GEMM_1X1 = ('conv_gemm_kernel<__hip_bfloat16, 1, false>', 'conv_gemm_kernel<__hip_bfloat16, 2, false>',
                                       'conv_gemm_kernel<__hip_bfloat16, 0, true>', 'conv_gemm_kernel<__hip_bfloat16, 0, false>')
WG4, WG2, WG1 = 'wgrad_k3_bf16_kernel<4, false, 8>', 'wgrad_k3_bf16_kernel<2, false, 4>', 'wgrad_k3_bf16_kernel<1, false, 4>'
F32_PK, F32_SC, F32_K2 = 'pack_bfrag_kernel<float>', 'conv_gemm_kernel<float, 0, true>', 'conv_gemm_kernel<float, 2, false>'
# id, kind, B, cin, cout, spatial (input), storage dtype, kernels the row exists to cover (forward, data gradient, weight gradient)
CONV_ROWS = [
    ("c1", "k3", 1, 1, 16, (25, 26, 23), BF, ['conv_k3_c1_kernel<1, false>', 'wgrad_k3_c1_kernel<false>', PK, RP]),
    ("p16", "k3", 1, 16, 16, (25, 26, 23), BF, ['conv_k3_p16_kernel<2, false, false>', WG1, PK, RP]),
    ("lds_32_32", "k3", 1, 32, 32, (25, 26, 23), BF, ['conv_k3_lds_kernel<32, 2, 4, 4>', WG2, PK, RP]),
    ("lds_16_32", "k3", 1, 16, 32, (25, 26, 23), BF, ['conv_k3_lds_kernel<16, 2, 4, 4>', 'conv_k3_lds_kernel<32, 1, 4, 4>', WG2, PK, RP]),
    # 48 input channels: chunk-major weights; its data gradient is 16 -> 48, three n-tiles
    ("lds_48_16", "k3", 1, 48, 16, (25, 26, 23), BF, ['conv_k3_lds_kernel<16, 1, 4, 4>', 'conv_k3_lds_kernel<16, 3, 4, 4>', WG1, PK, RP]),
    ("lds_64_64_wide", "k3", 1, 64, 64, (25, 26, 23), BF, ['conv_k3_lds_kernel<32, 4, 4, 8>', WG4, PK, RP]),
    # 4 x 84 tiles: more than the 256 workgroups up to which 64 -> 64 takes the wide form above
    ("lds_64_64_b4", "k3", 4, 64, 64, (25, 26, 23), BF, ['conv_k3_lds_kernel<32, 4, 2, 4>', WG4, PK, RP]),
    # 96 output channels: no tile kernel for the weight gradient, the generic MFMA one with its un-fused bias gradient
    ("lds_32_96", "k3", 1, 32, 96, (25, 26, 23), BF, ['conv_k3_lds_kernel<32, 3, 4, 4>', 'conv_k3_lds_kernel<32, 2, 4, 4>',
                                                     'conv_wgrad_kernel<__hip_bfloat16, __hip_bfloat16, 1>', 'colsum_kernel<__hip_bfloat16>', PK, RP]),
    ("p32_b2", "k3", 2, 32, 32, (41, 58, 57), BF, ['conv_k3_p32_kernel<8, false>', WG2, PK, RP]),
    # 128 -> 128 @ 13 x 11 x 10: conv_tile_plan cuts the 108 k-steps into 2 ranges at B = 8 (variant <1>), 4 at B = 5 (<2>)
    ("halo1_b8", "k3", 8, 128, 128, (13, 11, 10), BF, ['conv_k3_halo_kernel<1>', WG4, PK, RP]),
    ("halo2_b5", "k3", 5, 128, 128, (13, 11, 10), BF, ['conv_k3_halo_kernel<2>', WG4, PK, RP]),
    ("tile_256", "k3", 1, 256, 256, (5, 7, 3), BF, ['conv_k3_tile_kernel<2>', FIN, WG4, PK, RP]),
    ("tile_64_128_b3", "k3", 3, 64, 128, (5, 7, 3), BF, ['conv_k3_tile_kernel<2>', GEMM_K3, FIN, WG4, PK, RP]),
    ("gemm_64", "k3", 1, 64, 64, (5, 7, 9), BF, [GEMM_K3, FIN, WG4, PK, RP]),
    ("k2s2_16", "k2s2", 1, 16, 32, (10, 6, 14), BF, [GEMM_K2, GEMM_SC, 'wgrad_k2s2_bf16_kernel<2>', PK, RP]),
    ("k2s2_128", "k2s2", 1, 128, 256, (6, 10, 2), BF, [GEMM_K2, GEMM_SC, FIN, 'wgrad_k2s2_bf16_kernel<4>', PK, RP]),
    ("deconv_256", "deconv", 1, 256, 128, (3, 5, 2), BF, [GEMM_SC, GEMM_K2, 'colsum_kernel<__hip_bfloat16>', FIN, 'wgrad_k2s2_bf16_kernel<4>', PK, RP]),
    # 3 x 8 x 693 = 16 632 output rows: 65 column-sum partials, the fewest that take reduce_partials_small_kernel (more than 64)
    ("deconv_32_b3", "deconv", 3, 32, 16, (9, 7, 11), BF, [GEMM_SC, GEMM_K2, 'colsum_kernel<__hip_bfloat16>', 'reduce_partials_small_kernel',
                                                         'wgrad_k2s2_bf16_kernel<2>', PK, RP]),
    ("1x1_256", "1x1", 1, 256, 512, (3, 5, 2), BF, [GEMM_1X1, FIN, 'wgrad_1x1_bf16_kernel<4>', PK, RP]),
    ("1x1_head_f32_logits", "1x1", 1, 16, 2, (5, 7, 9), BF, ['head_1x1_fwd_kernel<__hip_bfloat16, 16, 2>', 'head_1x1_bwd_kernel<__hip_bfloat16, 2, 16>',
                                                           'wgrad_1x1_skinny_kernel<__hip_bfloat16, float, 16, 2>', 'colsum_kernel<float>', 'pack_tcn_kernel']),
    ("f32_k3", "k3", 1, 16, 32, (5, 7, 9), F32, ['conv_gemm_kernel<float, 1, false>', 'splitk_finish_kernel<float>', 'conv_wgrad_kernel<float, float, 1>',
                                               'colsum_kernel<float>', F32_PK, RP]),
    ("f32_k2s2", "k2s2", 1, 16, 32, (6, 4, 10), F32, [F32_K2, F32_SC, 'conv_wgrad_kernel<float, float, 2>', 'colsum_kernel<float>', F32_PK, RP]),
    ("f32_deconv", "deconv", 1, 32, 16, (3, 5, 2), F32, [F32_SC, F32_K2, 'conv_wgrad_kernel<float, float, 2>', 'colsum_kernel<float>', F32_PK, RP]),
    # Cin = 8: the weight gradient without the matrix cores; conv_gemm serves no data gradient of 8 columns, so none is asked for
    ("f32_cin8", "k3", 1, 8, 16, (5, 7, 9), F32, ['conv_gemm_kernel<float, 1, false>', 'conv_wgrad_direct_kernel']),
]
# the families the rows above were fixed on, checked against the library's own plan before anything runs
FAMILY = {"c1": "conv_k3_c1", "p16": "conv_k3_p16", "lds_32_32": "conv_k3_lds", "lds_16_32": "conv_k3_lds", "lds_48_16": "conv_k3_lds",
          "lds_64_64_wide": "conv_k3_lds", "lds_64_64_b4": "conv_k3_lds", "lds_32_96": "conv_k3_lds", "p32_b2": "conv_k3_p32", "halo1_b8": "conv_k3_halo",
          "halo2_b5": "conv_k3_halo", "tile_256": "conv_k3_tile", "tile_64_128_b3": "conv_k3_tile", "gemm_64": "conv_gemm_splitk"}


ACCUMULATE_KERNELS = [F32_K2, F32_SC, 'conv_wgrad_kernel<float, float, 2>', 'colsum_kernel<float>']
NORM_ACC_KERNELS = ['norm_apply_kernel<__hip_bfloat16, true>', 'norm_bwd_apply_kernel<__hip_bfloat16, true>', 'norm_partial_kernel<__hip_bfloat16, 0>',
                    'norm_partial_kernel<__hip_bfloat16, 1>']
HEAD_KERNELS = ['norm_apply_head_kernel<__hip_bfloat16>', 'norm_head_bwd_apply_kernel<__hip_bfloat16>', 'norm_head_partial_kernel<__hip_bfloat16>',
                'norm_head_finalize_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_finalize_stats_kernel', 'norm_finalize_bwd_kernel']
FIRST_BLOCK_KERNELS = ['conv_k3_c1_kernel<1, false>', 'first_block_bwd_kernel', 'first_block_reduce_kernel', 'first_block_finalize_kernel',
                       'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_finalize_stats_kernel', 'norm_apply_kernel<__hip_bfloat16, false>']
# (norm_fused_fwd_kernel<.., true, ..>: the form that sums the slabs; the finish launch of this row belongs to the data gradient's convolution)
FUSE_FINISH_KERNELS = ['conv_k3_tile_kernel<2>', 'norm_fused_fwd_kernel<__hip_bfloat16, 8, 8, true, 1>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 8, 1>',
                       'norm_sum_dparams_kernel', WG4]


def _out_shape(kind, B, sp, cout):
    if kind == "k2s2":
        return (B,) + tuple(s // 2 for s in sp) + (cout,)
    if kind == "deconv":
        return (B,) + tuple(2 * s for s in sp) + (cout,)
    return (B,) + tuple(sp) + (cout,)


@pytest.mark.parametrize("cid,kind,B,cin,cout,sp,dtype,want", CONV_ROWS, ids=[r[0] for r in CONV_ROWS])
def test_conv_guarded(cid, kind, B, cin, cout, sp, dtype, want):
    gen = _gen(("guard conv", cid))
    k = {"k3": 3, "k2s2": 2, "deconv": 2, "1x1": 1}[kind]
    out_f32 = kind == "1x1" and cout == 2
    need_gx = cin % 16 == 0
    if cid in FAMILY:
        plan = ops.conv_plan(ops.BF16, _lib.CONV_K3, 0, 0, B, *sp, cin, cout, cout)
        assert plan.name == FAMILY[cid], f"{cid}: the plan puts this shape on {plan.name}"
    wshape = (cin, cout, k, k, k) if kind == "deconv" else (cout, cin, k, k, k)
    w = _randn(wshape, gen) / float(np.sqrt(cin * k ** 3))
    if dtype == BF:
        w = w.to(BF).float()                      # the kernels multiply bf16-rounded weights
    b = _randn((cout,), gen)
    x = _randn((B,) + sp + (cin,), gen).to(dtype)
    gy = _randn(_out_shape(kind, B, sp, cout), gen).to(F32 if out_f32 else dtype)

    def run(wrap):
        e = _engine({"l.weight": w, "l.bias": b}, dtype, wrap)
        xd = wrap(x)
        y = e._conv("l", xd, kind, need_gx=need_gx, out_dtype=F32 if out_f32 else None)
        e.G[id(y)] = wrap(gy)
        for fn in reversed(e.tape):
            fn()
        torch.cuda.synchronize()
        return {"y": y, "gx": e.G.get(id(xd)), "gw": e.g["l.weight"], "gb": e.g["l.bias"]}

    what = f"conv {cid}: {kind} {cin}->{cout} @ {sp} B={B}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    yr, gxr, gwr, gbr = conv_ref64(kind, x, w, b, gy)                                           # (b)
    if dtype == BF:
        assert_bf16_elementwise(_nc(got["y"]), _nc(yr), f"y {what}")
        if need_gx:
            assert_bf16_elementwise(_nc(got["gx"]), _nc(gxr), f"gx {what}")
    else:
        close(got["y"], yr, 1e-4, 1e-5, f"y {what}")
        if need_gx:
            close(got["gx"], gxr, 1e-4, 1e-5, f"gx {what}")
    _close_max(got["gw"], gwr, f"gw {what}")
    _close_max(got["gb"], gbr, f"gb {what}")
    assert_same_bits(got, plain, what)                                                          # (c)
    expect(names, want, what)                                                                   # (d)


def test_conv_accumulate_guarded():
    """test_ops_gpu.test_conv_accumulate under the guard: the prior gradient tensor is an in/out buffer of the data gradient"""
    gen = _gen("guard accumulate")
    w = _randn((32, 16, 2, 2, 2), gen, 0.1)
    b = torch.zeros(32, device=DEV)
    x = _randn((1, 4, 4, 6, 16), gen)
    gy = _randn((1, 2, 2, 3, 32), gen)
    prior = _randn(tuple(x.shape), gen)

    def run(wrap):
        e = _engine({"l.weight": w, "l.bias": b}, F32, wrap)
        xd = wrap(x)
        y = e._conv("l", xd, "k2s2")
        e.G[id(y)] = wrap(gy)
        acc = e.G[id(xd)] = wrap(prior)
        for fn in reversed(e.tape):
            fn()
        torch.cuda.synchronize()
        assert e.G[id(xd)] is acc                # accumulated in place
        return {"y": y, "gx": e.G[id(xd)], "gw": e.g["l.weight"]}

    what = "conv accumulate k2s2 16->32"
    names, got, plain = run_both(run, what)
    yr, gxr, gwr, _ = conv_ref64("k2s2", x, w, b, gy)
    close(got["y"], yr, 1e-4, 1e-5, "y")
    close(got["gx"], gxr + prior.double(), 1e-4, 1e-5, "gx + prior")
    _close_max(got["gw"], gwr, "gw")
    assert_same_bits(got, plain, what)
    expect(names, ACCUMULATE_KERNELS, what)


# ------------------------------------------------------------------------------------------------------------------- upconv_k3
@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("cin,cout,sp", [(16, 16, (3, 5, 7)), (64, 32, (3, 5, 7)), (16, 16, (1, 4, 6))],
                         ids=["16_16", "64_32", "extent1"])
def test_upconv_k3_guarded(cin, cout, sp, dtype):
    """dycon_upconv_k3 (both KMODEs: Cin a multiple of the k-step or not) against fp64 F.interpolate + F.conv3d, with the bound
    test_vnet_blocks_gpu.test_upconv_k3_equals_resize_then_conv uses for this kernel (1e-4 fp32, 2^-7 bf16 of the largest output)"""
    gen = _gen(("guard upconv", cin, cout, sp))
    B = 2
    x = _randn((B,) + sp + (cin,), gen).to(dtype)
    w = (_randn((cout, cin, 3, 3, 3), gen) * (2.0 / (27 * cin)) ** 0.5).to(dtype).float()
    bias = _randn((cout,), gen, 0.1)

    def run(wrap):
        wd = wrap(w)
        wf = ops.pack_bfrag(wd, dtype, 27, cin, cout, cout, 1, 27, 0, cin * 27)
        y = ops.upconv_k3(wrap(x), wf, wrap(bias), cout)
        torch.cuda.synchronize()
        return {"y": y}

    what = f"upconv_k3 {cin}->{cout} @ {sp} {dtype}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    up = F.interpolate(x.double().permute(0, 4, 1, 2, 3), scale_factor=2, mode="trilinear", align_corners=False)
    ref = F.conv3d(up, w.double(), bias.double(), padding=1).permute(0, 2, 3, 4, 1)
    err = float((got["y"].double() - ref).abs().max()) / float(ref.abs().max())
    tol = 1e-4 if dtype == F32 else 2.0 ** -7
    print(f"{what}: err {err:.3e} (bound {tol:.3e})")
    assert err <= tol
    assert_same_bits(got, plain, what)
    tn = "float" if dtype == F32 else "__hip_bfloat16"
    kmode = 0 if cin % (16 if dtype == F32 else 32) == 0 else 1
    expect(names, [f"(anonymous namespace)::upconv_k3_kernel<{tn}, {kmode}>", f"pack_bfrag_kernel<{tn}>"], what)


# ------------------------------------------------------------------------------------------------------------------- norms
THREE = ['norm_apply_kernel<__hip_bfloat16, false>', 'norm_bwd_apply_kernel<__hip_bfloat16, false>', 'norm_finalize_bwd_kernel',
         'norm_finalize_stats_kernel', 'norm_partial_kernel<__hip_bfloat16, 0>', 'norm_partial_kernel<__hip_bfloat16, 1>']
# id, kind, C, spatial, mode, kernels (all B = 2)
NORM_ROWS = [
    ("gn256_v257", "gn", 256, (1, 1, 257), "relu",
     ['norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 8>', 'norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 8>', 'norm_sum_dparams_kernel']),
    ("gn64_v2049_three_launch", "gn", 64, (3, 683, 1), "relu", THREE),
    ("gn32_v245_skip", "gn", 32, (7, 7, 5), "skip",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 2, false, 1>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 2, 1>', 'norm_sum_dparams_kernel']),
    ("in16_v245", "in", 16, (7, 7, 5), "relu",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 1>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 1>']),
    # the other instantiations of the one-launch form a real step launches (channels per group x rows per thread)
    ("gn256_v245", "gn", 256, (7, 7, 5), "relu",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 16, 16, false, 1>', 'norm_fused_bwd_kernel<__hip_bfloat16, 16, 16, 1>', 'norm_sum_dparams_kernel']),
    ("gn128_v294", "gn", 128, (7, 7, 6), "relu",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 8, false, 8>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 8, 8>', 'norm_sum_dparams_kernel']),
    ("gn64_v294_skip", "gn", 64, (7, 7, 6), "skip",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 4, false, 8>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 4, 8>', 'norm_sum_dparams_kernel']),
    ("gn32_v294", "gn", 32, (7, 7, 6), "relu",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 2, false, 8>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 2, 8>', 'norm_sum_dparams_kernel']),
    ("bn128_v245_scale", "bn", 128, (7, 7, 5), "scale",
     ['norm_fused_fwd_kernel<__hip_bfloat16, 8, 1, false, 8>', 'norm_fused_bwd_kernel<__hip_bfloat16, 8, 1, 8>', 'norm_sum_dparams_kernel',
      'scale_channels_kernel<__hip_bfloat16>']),
]


@pytest.mark.parametrize("nid,kind,C,sp,mode,want", NORM_ROWS, ids=[r[0] for r in NORM_ROWS])
def test_norm_guarded(nid, kind, C, sp, mode, want):
    gen = _gen(("guard norm", nid))
    B = 2
    z = _randn((B,) + sp + (C,), gen, 1.5, 0.3).to(BF)
    affine = kind != "in"
    gamma = _randn((C,), gen, 0.2, 1.0) if affine else None
    beta = _randn((C,), gen, 0.2) if affine else None
    skip = _randn((B,) + sp + (C,), gen).to(BF) if mode == "skip" else None
    cs = (torch.rand(B * C, generator=gen, device=DEV) > 0.5).float() * 2.0 if mode == "scale" else None
    gy = _randn((B,) + sp + (C,), gen).to(BF)
    rm0, rv0 = _randn((C,), gen, 0.1), 1.0 + torch.rand(C, generator=gen, device=DEV)

    def run(wrap):
        e = _engine({"n.weight": gamma, "n.bias": beta} if affine else {}, BF, wrap)
        if kind == "bn":
            e.buf = {"n.running_mean": wrap(rm0), "n.running_var": wrap(rv0)}
        zd, sd = wrap(z), wrap(skip)
        y = e._norm("n" if affine else None, zd, kind, relu=True, skip=sd, training=True, chan_scale=wrap(cs))
        ycopy = y.clone()
        e.G[id(y)] = wrap(gy)
        for fn in reversed(e.tape):
            fn()
        torch.cuda.synchronize()
        out = {"y": ycopy, "gz": e.G[id(zd)], "gskip": e.G[id(sd)] if sd is not None else None}
        if affine:
            out.update(dgamma=e.g["n.weight"], dbeta=e.g["n.bias"])
        if kind == "bn":
            out.update(running_mean=e.buf["n.running_mean"], running_var=e.buf["n.running_var"])
        return out

    what = f"norm {nid}: {kind} C={C} @ {sp} B={B} {mode}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    run64 = (rm0.double(), rv0.double()) if kind == "bn" else None
    yr, gzr, dgr, dbr, _ = norm_ref64(kind, z, gy, gamma, beta, relu=True, skip=skip, chan_scale=cs, running=run64)
    assert_bf16_elementwise(_nc(got["y"]), _nc(yr), f"y {what}")
    assert_bf16_elementwise(_nc(got["gz"]), _nc(gzr), f"gz {what}", acc_noise=2e-3)
    if skip is not None:
        assert torch.equal(got["gskip"], gy), f"gskip {what}: not gy exactly"
    if affine:
        _close_max(got["dgamma"], dgr, f"dgamma {what}")
        _close_max(got["dbeta"], dbr, f"dbeta {what}")
    if kind == "bn":
        for nm, ref in (("running_mean", run64[0]), ("running_var", run64[1])):
            np.testing.assert_allclose(got[nm].cpu().numpy(), ref.cpu().numpy(), rtol=1e-5, atol=1e-7, err_msg=f"{nm} {what}")
    assert_same_bits(got, plain, what)
    expect(names, want, what)


def test_norm_accumulator_form_guarded():
    """dycon_norm_fwd_acc / dycon_norm_bwd_acc (statistics by double atomics into the caller's zeroed arena slice): C = 16,
    V = 14 x 14 x 12, two samples"""
    gen = _gen("guard norm acc")
    Nb, sp, C, G = 2, (14, 14, 12), 16, 16
    V = sp[0] * sp[1] * sp[2]
    z = _randn((Nb,) + sp + (C,), gen, 1.3, 0.4).to(BF)
    gy = _randn((Nb,) + sp + (C,), gen).to(BF)
    gamma, beta = _randn((C,), gen, 0.2, 1.0), _randn((C,), gen, 0.2)
    nacc = ops.query("dycon_norm_acc_doubles", Nb, V, C)

    def run(wrap):
        zd, gd, bd = wrap(z), wrap(gamma), wrap(beta)
        acc = wrap(torch.zeros(nacc, dtype=torch.float64, device=DEV))
        y, stats = ops.norm_fwd(zd, Nb, V, C, G, gd, bd, True, acc=acc)
        dg, db = wrap(torch.full((C,), float("nan"), device=DEV)), wrap(torch.full((C,), float("nan"), device=DEV))
        acc2 = wrap(torch.zeros(nacc, dtype=torch.float64, device=DEV))
        gz = ops.norm_bwd(zd, False, wrap(gy), stats, Nb, V, C, G, gd, bd, True, dg, db, acc=acc2)
        torch.cuda.synchronize()
        return {"y": y, "stats": stats, "gz": gz, "dgamma": dg, "dbeta": db}

    what = "norm accumulator form C=16 V=2352"
    assert not ops.norm_fwd_is_fused(z, V, C, G)
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    yr, gzr, dgr, dbr, _ = norm_ref64("gn", z, gy, gamma, beta)
    assert_bf16_elementwise(_nc(got["y"]), _nc(yr), f"y {what}")
    assert_bf16_elementwise(_nc(got["gz"]), _nc(gzr), f"gz {what}", acc_noise=2e-3)
    _close_max(got["dgamma"], dgr, f"dgamma {what}")
    _close_max(got["dbeta"], dbr, f"dbeta {what}")
    # double atomics: the last bits of the statistics can differ between runs; y / gz are bf16 (one ulp where they do)
    assert_same_1e6({k: got[k] for k in ("stats", "dgamma", "dbeta")}, plain, what)
    for k in ("y", "gz"):
        assert float((got[k].float() - plain[k].float()).abs().max()) <= 1e-2 * float(plain[k].float().abs().max()), k
    expect(names, NORM_ACC_KERNELS, what)


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_norm_head_guarded(drop):
    """Engine._norm_head (GroupNorm(16) -> ReLU [-> Dropout3d factor] -> 16 -> 2 head in the norm's passes) @ (10, 9, 13), B = 3,
    against fp64 autograd with the bounds of test_dispatch_parity_gpu.test_norm_head_dispatch_bf16"""
    gen = _gen(("guard head", drop))
    B, sp, C = 3, (10, 9, 13), 16
    z = _randn((B,) + sp + (C,), gen, 1.5, 0.3).to(BF)
    gamma, beta = _randn((C,), gen, 0.2, 1.0), _randn((C,), gen, 0.2)
    hw, hb = _randn((2, C, 1, 1, 1), gen, 0.4), _randn((2,), gen)
    cs = (torch.rand(B * C, generator=gen, device=DEV) > 0.5).float() * 2.0 if drop else None
    gl = _randn((B,) + sp + (2,), gen)

    def run(wrap):
        e = _engine({"n.weight": gamma, "n.bias": beta, "h.weight": hw, "h.bias": hb}, BF, wrap)
        zd = wrap(z)
        logits = e._norm_head("n", zd, "gn", "h", training=True, chan_scale=wrap(cs))
        lcopy = logits.clone()
        e.G[id(logits)] = wrap(gl)
        for fn in reversed(e.tape):
            fn()
        torch.cuda.synchronize()
        return {"logits": lcopy, "gz": e.G[id(zd)], "dgamma": e.g["n.weight"], "dbeta": e.g["n.bias"], "head gw": e.g["h.weight"],
                "head gb": e.g["h.bias"]}

    what = f"norm head @ {sp} B={B} drop={drop}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    zr = z.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    w64 = hw.double()
    a = F.relu(F.group_norm(zr, 16, g64, b64, 1e-5))
    if cs is not None:
        a = a * cs.double().reshape(B, C, 1, 1, 1)
    ref = F.conv3d(a, w64, hb.double()).detach()
    gl64 = gl.double().permute(0, 4, 1, 2, 3)
    aq = a.detach().to(BF).double()              # the head's weight gradient reads the activations rounded to bf16 ...
    gw64 = torch.einsum("bodhw,bcdhw->oc", gl64, aq).reshape(w64.shape)
    gb64 = gl64.sum((0, 2, 3, 4))
    gy64 = F.conv3d(gl64, w64.reshape(2, C).t().reshape(C, 2, 1, 1, 1))
    (gz64,) = torch.autograd.grad(a, zr, gy64, retain_graph=True)
    a.backward(gy64.to(BF).double())             # ... and dgamma / dbeta the head's data gradient rounded to bf16
    lg = _nc(got["logits"]).double()
    bound = 2.0 ** -8 * F.conv3d(a.detach().abs(), w64.abs()) + 2.0 ** -7 * ref.abs() + 1e-3 * float(ref.pow(2).mean().sqrt())
    excess = (lg - ref).abs() - bound
    assert float(excess.max()) <= 0, f"logits {what}: {int((excess > 0).sum())} elements off, worst excess {float(excess.max()):.3e}"
    assert_bf16_elementwise(_nc(got["gz"]), gz64, f"gz {what}", acc_noise=2e-3)
    for nm, rf in (("dgamma", g64.grad), ("dbeta", b64.grad), ("head gw", gw64), ("head gb", gb64)):
        _close_max(got[nm], rf, f"{nm} {what}")
    assert_same_bits(got, plain, what)
    expect(names, HEAD_KERNELS, what)


def test_first_block_guarded():
    """Engine._first_block (conv 1 -> 16, GroupNorm(16), ReLU; the backward in one pass) @ (24, 20, 29), B = 2, with the bounds of
    test_dispatch_parity_gpu.test_first_block_dispatch_bf16"""
    gen = _gen("guard first block")
    B, sp, C = 2, (24, 20, 29), 16
    w = (_randn((C, 1, 3, 3, 3), gen) / float(np.sqrt(27))).to(BF).float()
    b = _randn((C,), gen, 0.1)
    gamma, beta = _randn((C,), gen, 0.2, 1.0), _randn((C,), gen, 0.2)
    x = _randn((B,) + sp + (1,), gen).to(BF)
    gy = _randn((B,) + sp + (C,), gen).to(BF)
    names_p = {"block_one.conv.0.weight": w, "block_one.conv.0.bias": b, "block_one.conv.1.weight": gamma, "block_one.conv.1.bias": beta}

    def run(wrap):
        e = _engine(names_p, BF, wrap)
        xd = wrap(x)
        assert e._fuses_first_block(xd, "gn", True)
        y = e._first_block("block_one", xd, "gn", True)
        ycopy = y.clone()
        e.G[id(y)] = wrap(gy)
        for fn in reversed(e.tape):
            fn()
        e.recording = False
        zq = e._conv("block_one.conv.0", xd, "k3", need_gx=False)     # the block's stored convolution output (same launch again)
        torch.cuda.synchronize()
        return {"y": ycopy, "z": zq, **{k: e.g[k] for k in names_p}}

    what = f"first block @ {sp} B={B}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    zc, _, _, _ = conv_ref64("k3", x, w, b, torch.zeros(B, *sp, C, device=DEV))
    assert_bf16_elementwise(_nc(got["z"]), _nc(zc), f"z {what}")
    yr, gzr, dgr, dbr, _ = norm_ref64("gn", got["z"], gy, gamma, beta)
    _, _, gwr, gbr = conv_ref64("k3", x, w, b, gzr)
    assert_bf16_elementwise(_nc(got["y"]), _nc(yr), f"y {what}")
    _close_max(got["block_one.conv.0.weight"], gwr, f"gw {what}", 2e-4)
    scale_b = float(gzr.abs().sum((0, 1, 2, 3)).max())       # sum(gz) is ~0 analytically: on the scale of the terms that cancel
    err_b = float((got["block_one.conv.0.bias"].double() - gbr).abs().max())
    assert err_b <= 1e-5 * scale_b, (err_b, scale_b)
    _close_max(got["block_one.conv.1.weight"], dgr, f"dgamma {what}")
    _close_max(got["block_one.conv.1.bias"], dbr, f"dbeta {what}")
    assert_same_bits(got, plain, what)
    expect(names, FIRST_BLOCK_KERNELS, what)


def test_split_k_finish_fused_into_norm_guarded():
    """fuse_finish=True, 128 -> 128 @ (5, 6, 4), B = 3: the convolution leaves its split-K slabs (the deferred workspace is the
    guarded tensor of interest) to the one-launch norm that follows (dycon_norm_fwd_slab)"""
    gen = _gen("guard fuse finish")
    B, sp, cin, cout = 3, (5, 6, 4), 128, 128
    w = (_randn((cout, cin, 3, 3, 3), gen) / float(np.sqrt(cin * 27))).to(BF).float()
    b = _randn((cout,), gen, 0.3)
    gamma, beta = _randn((cout,), gen, 0.2, 1.0), _randn((cout,), gen, 0.2)
    x = _randn((B,) + sp + (cin,), gen).to(BF)
    gy = _randn((B,) + sp + (cout,), gen).to(BF)
    assert ops.conv_plan(ops.BF16, _lib.CONV_K3, 0, 0, B, *sp, cin, cout, cout).splits > 1

    def run(wrap):
        e = _engine({"l.weight": w, "l.bias": b, "n.weight": gamma, "n.bias": beta}, BF, wrap)
        e.fuse_finish = True
        xd = wrap(x)
        z = e._conv("l", xd, "k3", norm_groups=16)
        assert id(z) in e._deferred, "the split-K finish was not left to the norm"
        y = e._norm("n", z, "gn")
        ycopy = y.clone()
        e.G[id(y)] = wrap(gy)
        norm_bwd, conv_bwd = reversed(e.tape)
        norm_bwd()
        gz = e.G[id(z)].clone()                  # the stored (bf16) data gradient the convolution's backward reads
        conv_bwd()
        torch.cuda.synchronize()
        return {"z": z, "y": ycopy, "gz": gz, "gx": e.G[id(xd)], "gw": e.g["l.weight"], "gb": e.g["l.bias"], "dgamma": e.g["n.weight"],
                "dbeta": e.g["n.bias"]}

    what = f"split-K finish fused into the norm 128->128 @ {sp} B={B}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    zr, _, _, _ = conv_ref64("k3", x, w, b, gy)
    assert_bf16_elementwise(_nc(got["z"]), _nc(zr), f"z {what}")
    yr, gzr, dgr, dbr, _ = norm_ref64("gn", got["z"], gy, gamma, beta)
    assert_bf16_elementwise(_nc(got["y"]), _nc(yr), f"y {what}")
    assert_bf16_elementwise(_nc(got["gz"]), _nc(gzr), f"gz {what}", acc_noise=2e-3)
    _close_max(got["dgamma"], dgr, f"dgamma {what}")
    _close_max(got["dbeta"], dbr, f"dbeta {what}")
    _, gxr, gwr, gbr = conv_ref64("k3", x, w, b, got["gz"])
    assert_bf16_elementwise(_nc(got["gx"]), _nc(gxr), f"gx {what}")
    _close_max(got["gw"], gwr, f"gw {what}")
    # (sum(gz) per channel is ~0 analytically -- the norm backward removes the group mean; held on the scale of its terms)
    assert float((got["gb"].double() - gbr).abs().max()) <= 1e-3 * float(got["gz"].double().abs().sum((0, 1, 2, 3)).max())
    assert_same_bits(got, plain, what)
    expect(names, FUSE_FINISH_KERNELS, what)


# ------------------------------------------------------------------------------------------------------------------- ledger
# kernels of csrc/conv.hip / csrc/norm.hip that a real step or evaluation launches and no op-level row above names: reached by a
# whole-path row of tests/test_guard_step_gpu.py, which asserts the launch
REACHED_BY_A_GUARDED_PATH = {"pack_batch_kernel": "test_guard_step_gpu::test_single_case_guarded"}


def test_every_ledger_kernel_is_reached_under_the_guard():
    """every conv / norm kernel that test_dispatch_parity_gpu.test_ledger accepts in a real step (its rows and COVERED_ELSEWHERE:
    test_ledger fails on a launch outside them) is named by a guarded row here or reached by a guarded whole path"""
    import re
    import test_dispatch_parity_gpu as T
    declared = T._declared_kernels()
    ledger = sorted(n for n in T._rows_expect() | set(T.COVERED_ELSEWHERE) if re.match(r"\w+", n).group(0) in declared)
    rows = [r[-1] for r in CONV_ROWS] + [r[-1] for r in NORM_ROWS] + [ACCUMULATE_KERNELS, NORM_ACC_KERNELS, HEAD_KERNELS, FIRST_BLOCK_KERNELS,
                                                                    FUSE_FINISH_KERNELS]
    named = {k for row in rows for k in row}
    missing = [n for n in ledger if n not in named and n not in REACHED_BY_A_GUARDED_PATH]
    print(f"{len(ledger)} ledger kernels, {len(named & set(ledger))} named by an op-level row, {sorted(REACHED_BY_A_GUARDED_PATH)} by a whole path")
    assert not missing, f"conv / norm kernels of a real step without a guarded row: {missing}"


# ------------------------------------------------------------------------------------------------------------------- spatial.hip
@pytest.mark.parametrize("C,dtype", [(16, BF), (8, F32)], ids=["c16_bf16", "c8_fp32"])
def test_maxpool2_guarded(C, dtype):
    gen = _gen(("guard maxpool", C))
    B, sp = 2, (6, 10, 14)
    x = _randn((B,) + sp + (C,), gen).to(dtype)
    gy = _randn((B,) + tuple(s // 2 for s in sp) + (C,), gen).to(dtype)

    def run(wrap):
        xd = wrap(x)
        y, idx = ops.maxpool2_fwd(xd)
        gx = ops.maxpool2_bwd(wrap(gy), idx, xd.shape)
        torch.cuda.synchronize()
        return {"y": y, "idx": idx, "gx": gx}

    what = f"maxpool2 C={C} {dtype}"
    names, got, plain = run_both(run, what)
    xr = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    yr = F.max_pool3d(xr, 2)
    (gxr,) = torch.autograd.grad(yr, xr, gy.double().permute(0, 4, 1, 2, 3))
    close(_nc(got["y"]), yr, 0, 0, "y")                          # a maximum and a scatter: exact
    close(_nc(got["gx"]), gxr, 0, 0, "gx")
    assert_same_bits(got, plain, what)
    tn = "float" if dtype == F32 else "__hip_bfloat16"
    expect(names, [f"maxpool2_fwd_kernel<{tn}>", f"maxpool2_bwd_kernel<{tn}>"], what)


@pytest.mark.parametrize("align", [False, True], ids=["half_pixel", "align_corners"])
def test_trilinear_guarded(align):
    """(5, 7, 3) -> (12, 9, 13), forward and gathered adjoint, and the channel-window forms: out= a guarded (..., 12) tensor with
    coff=4 -- the channels outside the window keep their fill bit for bit"""
    gen = _gen(("guard trilinear", align))
    B, C, sp, out = 1, 8, (5, 7, 3), (12, 9, 13)
    x = _randn((B,) + sp + (C,), gen)
    r = _randn((B,) + out + (C,), gen)
    fill = _randn((B,) + out + (12,), gen)
    gwin = _randn((B,) + out + (12,), gen)

    def run(wrap):
        xd = wrap(x)
        y = ops.trilinear_fwd(xd, out, align)
        gx = ops.trilinear_bwd(wrap(r), xd.shape, align)
        win = wrap(fill)
        ops.trilinear_fwd(wrap(x[..., :4].contiguous()), out, align, out=win, coff=4)
        gxw = ops.trilinear_bwd(wrap(gwin), (B,) + sp + (4,), align, coff=4)
        torch.cuda.synchronize()
        return {"y": y, "gx": gx, "window": win, "gx window": gxw}

    what = f"trilinear {sp} -> {out} align_corners={align}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)

    def ref(xs, rs):
        xr = xs.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
        yr = F.interpolate(xr, size=out, mode="trilinear", align_corners=align)
        (g,) = torch.autograd.grad(yr, xr, rs.double().permute(0, 4, 1, 2, 3))
        return yr.detach(), g
    yr, gxr = ref(x, r)
    close(_nc(got["y"]), yr, 1e-5, 1e-6, "y")
    close(_nc(got["gx"]), gxr, 1e-4, 1e-5, "gx")
    ywr, gxwr = ref(x[..., :4], gwin[..., 4:8])
    close(_nc(got["window"][..., 4:8]), ywr, 1e-5, 1e-6, "window")
    assert torch.equal(got["window"][..., :4], fill[..., :4]) and torch.equal(got["window"][..., 8:], fill[..., 8:]), \
        "channels outside the window changed"
    close(_nc(got["gx window"]), gxwr, 1e-4, 1e-5, "gx window")
    assert_same_bits(got, plain, what)
    expect(names, ["trilinear_fwd_kernel<float>", "trilinear_bwd_kernel<float>"], what)


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
def test_copy_channels_and_relu_guarded(dtype):
    """copy_channels into a channel window; relu_fwd / relu_bwd with skip and chan_scale at 630 elements (not a multiple of 8)"""
    gen = _gen(("guard pointwise", dtype))
    src = _randn((2, 4, 5, 6, 16), gen).to(dtype)
    dst0 = _randn((2, 4, 5, 6, 40), gen).to(dtype)
    B, sp, C = 2, (3, 5, 7), 3
    z = _randn((B,) + sp + (C,), gen).to(dtype)
    skip = _randn((B,) + sp + (C,), gen).to(dtype)
    gy = _randn((B,) + sp + (C,), gen).to(dtype)
    cs = (torch.rand(B * C, generator=gen, device=DEV) > 0.5).float() * 2.0
    assert z.numel() % 8 != 0

    def run(wrap):
        dst = wrap(dst0)
        ops.copy_channels(wrap(src), 4, dst, 10, 8)
        zd, cd = wrap(z), wrap(cs)
        y = ops.relu_fwd(zd, wrap(skip), cd)
        gz = ops.relu_bwd(zd, wrap(gy), cd)
        torch.cuda.synchronize()
        return {"dst": dst, "y": y, "gz": gz}

    what = f"copy_channels / relu {dtype}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    assert torch.equal(got["dst"][..., 10:18], src[..., 4:12])
    assert torch.equal(got["dst"][..., :10], dst0[..., :10]) and torch.equal(got["dst"][..., 18:], dst0[..., 18:])
    s64 = cs.double().reshape(B, 1, 1, 1, C)
    yr = F.relu(z.double()) * s64 + skip.double()
    gzr = gy.double() * (z.double() > 0) * s64
    if dtype == F32:
        close(got["y"], yr, 1e-6, 1e-7, "y")
        close(got["gz"], gzr, 1e-6, 1e-7, "gz")
    else:                                          # one bf16 rounding of an exactly representable fp32 result
        close(got["y"], yr.float().to(BF), 0, 0, "y")
        close(got["gz"], gzr.float().to(BF), 0, 0, "gz")
    assert_same_bits(got, plain, what)
    tn = "float" if dtype == F32 else "__hip_bfloat16"
    expect(names, [f"copy_channels_kernel<{tn}>", f"relu_fwd_kernel<{tn}>", f"relu_bwd_kernel<{tn}>"], what)


# ------------------------------------------------------------------------------------------------------------------- losses.hip
def _seg_ref64(s, t, lab, LB, beta, C):
    """the oracle's losses in double on NCDHW logits: the six values and, per term, d / d s_logits"""
    s64 = s.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    t64 = t.double().permute(0, 4, 1, 2, 3)
    lab = lab.long()
    sp, tp = F.softmax(s64, 1), F.softmax(t64, 1)
    terms = {"ce": F.cross_entropy(s64[:LB], lab[:LB]), "dice": OL.dice_loss(sp[:LB, 1], lab[:LB] == 1),
             "dice_mc": OL.dice_loss_multiclass(sp[:LB], lab[:LB], C), "cons_mse": OL.softmax_mse(sp[LB:], tp[LB:]).mean(),
             "cons_kl": OL.softmax_kl(sp[LB:], tp[LB:]), "uncl": OL.uncl(s64, t64, beta)}
    grads = {k: torch.autograd.grad(v, s64, retain_graph=True)[0].permute(0, 2, 3, 4, 1) for k, v in terms.items()}
    return {k: float(v.detach()) for k, v in terms.items()}, grads


SEG_TERMS = ("ce", "dice", "dice_mc", "cons_mse", "cons_kl", "uncl")       # vals[0..5]; coef slots ce, dice, dice_mc, cons, uncl
COEF_SLOT = {"ce": 0, "dice": 1, "dice_mc": 2, "cons_mse": 3, "cons_kl": 3, "uncl": 4}


@pytest.mark.parametrize("fast", [False, True], ids=["libm", "fast"])
@pytest.mark.parametrize("lab_dtype", [torch.uint8, torch.int64], ids=["u8", "i64"])
@pytest.mark.parametrize("C", [2, 3, 8], ids=["seg_losses", "seg_lossesc3", "seg_lossesc8"])
def test_seg_losses_guarded(C, lab_dtype, fast):
    """seg_losses_* (C = 2) / seg_lossesc_* (C = 3, 8) at B = 3, LB = 1, V = 5 x 7 x 9: values and every term's gradient (cons_kind 0
    and 1) against the oracle's losses in double, at test_voxel_losses_golden's tolerances (x 10 for the fast sequences)"""
    gen = _gen(("guard seg", C))
    B, LB, sp, beta = 3, 1, (5, 7, 9), 1.7
    V = sp[0] * sp[1] * sp[2]
    s, t = _randn((B,) + sp + (C,), gen, 2.0), _randn((B,) + sp + (C,), gen, 2.0)
    lab = torch.randint(0, C, (B,) + sp, generator=gen, device=DEV).to(lab_dtype)
    two = C == 2
    fwd, bwd, fin = (ops.seg_losses_fwd, ops.seg_losses_bwd, ops.seg_losses_finalize) if two else \
        (ops.seg_lossesc_fwd, ops.seg_lossesc_bwd, ops.seg_lossesc_finalize)

    def run(wrap):
        sd, td, ld = wrap(s), wrap(t), wrap(lab)
        sums = fwd(sd, td, ld, LB, beta, fast=fast)
        vals = fin(sums, B, LB, V, beta) if two else fin(sums, B, LB, V, C, beta)
        out = {"sums": sums, "vals": vals[:6].clone()}       # (vals[6] of the 8 allocated floats are written)
        for term in SEG_TERMS:
            coef = torch.zeros(5, device=DEV)
            coef[COEF_SLOT[term]] = 1
            out["g " + term] = bwd(sd, td, ld, LB, beta, sums, wrap(coef), 1 if term == "cons_kl" else 0, fast=fast)
        torch.cuda.synchronize()
        return out

    what = f"seg losses C={C} {lab_dtype} fast={fast}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    vals_r, grads_r = _seg_ref64(s, t, lab, LB, beta, C)
    k = 10.0 if fast else 1.0
    for i, term in enumerate(SEG_TERMS):
        close(got["vals"][i], vals_r[term], k * (1e-4 if term == "cons_kl" else 1e-5), 1e-6 if i < 3 or i == 5 else 1e-7, term)
        close(got["g " + term], grads_r[term], k * 1e-4, k * (1e-9 if term.startswith("cons") else 1e-8), "gradient " + term)
    assert_same_1e6(got, plain, what)
    base, targs = ("seg_losses", "") if two else ("seg_lossesc", f"{C}, ")
    tf = "true" if fast else "false"
    expect(names, [f"{base}_fwd_kernel<{targs}{tf}>", f"{base}_bwd_kernel<{targs}{tf}>", f"{base}_finalize_kernel"], what)


def test_l2norm_maskpool_guarded():
    """l2norm at R = 50, C = 256 (one row below the eps clamp); mask_pool with k = (4, 8, 2)"""
    gen = _gen("guard l2norm")
    x = _randn((1, 50, 256), gen)
    x[0, 3] = 0
    gy = _randn((1, 50, 256), gen)
    lab = (torch.rand((2, 16, 24, 8), generator=gen, device=DEV) > 0.5)

    def run(wrap):
        y, nrm = ops.l2norm_fwd(wrap(x))
        gx = ops.l2norm_bwd(y, nrm, wrap(gy))
        m8 = ops.mask_pool(wrap(lab.to(torch.uint8)), (4, 8, 2))
        m64 = ops.mask_pool(wrap(lab.long()), (4, 8, 2))
        torch.cuda.synchronize()
        return {"y": y, "norms": nrm, "gx": gx, "mask u8": m8, "mask i64": m64}

    what = "l2norm R=50 C=256 / mask_pool (4, 8, 2)"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    xr = x.double().requires_grad_(True)
    yr = F.normalize(xr, dim=-1)
    (gxr,) = torch.autograd.grad(yr, xr, gy.double())
    close(got["y"], yr, 1e-5, 1e-6, "y")
    close(got["gx"], gxr, 1e-4, 1e-5, "gx")
    mr = (F.avg_pool3d(lab.double().unsqueeze(1), (4, 8, 2)) > 0.5).float().reshape(2, -1)
    close(got["mask u8"], mr, 0, 0, "mask u8")
    close(got["mask i64"], mr, 0, 0, "mask i64")
    assert_same_bits(got, plain, what)
    expect(names, ["l2norm_fwd_kernel<float>", "l2norm_bwd_kernel<float>", "mask_pool_kernel"], what)


@pytest.mark.parametrize("N,Dm,dtype,want", [(100, 64, F32, [f"fecl_kernel<float, {i}, false>" for i in (1, 2, 3, 4)] + ["fecl_combine_kernel<float>"]),
                                             (1030, 128, BF, [f"fecl_rows128_kernel<{i}, 8, false>" for i in (1, 2, 3)] +
                                              ["fecl_rows128_grad_kernel<8>", "fecl_combine_kernel<__hip_bfloat16>"])],
                         ids=["n100_fp32", "n1030_bf16_rows128"])
def test_fecl_guarded(N, Dm, dtype, want):
    """fecl_fwd / fecl_bwd on fecl_kernel (fp32, N = 100) and on the 128-row kernels (bf16, N = 1030: ragged last row block and
    column tile) against the oracle in double on the stored inputs, with the bounds of test_fecl_rows128_kernel_vs_oracle
    (loss 3e-4 / 1e-6, gradient 2e-2 of its largest element; fp32 storage: test_fecl_golden's 1e-4)"""
    gen = _gen(("guard fecl", N))
    B, epoch = 2, 300
    f = F.normalize(_randn((B, N, Dm), gen), dim=-1).to(dtype)
    t = F.normalize(f.float() + 0.05 * _randn((B, N, Dm), gen), dim=-1).to(dtype)
    mask = (torch.rand((B, N), generator=gen, device=DEV) > 0.85).float()
    thr = OL.threshold_rampup(epoch, 1500, 0.3, 0.5)

    def run(wrap):
        args = (wrap(f), wrap(t), wrap(mask), None, 0.6, 2.0, True, thr, 1.0)
        loss, st = ops.fecl_fwd(*args)
        gf = ops.fecl_bwd(*args, st, wrap(torch.ones(1, device=DEV)))
        torch.cuda.synchronize()
        return {"loss": loss, "grad": gf}

    what = f"fecl N={N} Dm={Dm} {dtype}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    fr = f.double().cpu().requires_grad_(True)
    ref = OL.fecl(fr, mask.double().cpu().view(B, 1, N), t.double().cpu(), None, epoch, 0.6, 2.0, True, 1500, 1.0)
    (gr,) = torch.autograd.grad(ref, fr)
    if dtype == BF:
        close(got["loss"][0], ref, 3e-4, 1e-6, "loss")
        relclose(got["grad"], gr, 2e-2, "fecl rows128 grad")
    else:
        close(got["loss"][0], ref, 1e-4, 1e-6, "loss")
        relclose(got["grad"], gr, 1e-4, "fecl grad")
    assert_same_1e6({"loss": got["loss"]}, plain, what)
    tol = 1e-6 if dtype == F32 else 2.0 ** -7      # (a bf16 gradient moves by one rounding step where a double sum's last bit differs)
    assert float((got["grad"].double() - plain["grad"].double()).abs().max()) <= tol * float(plain["grad"].double().abs().max())
    expect(names, want, what)


@pytest.mark.parametrize("fast", [False, True], ids=["libm", "fast"])
def test_gambling_uncertainty_guarded(fast):
    """gambling_uncertainty fwd / bwd at (8, 12, 4), k = (4, 4, 2), with test_gambling_gpu.test_fused_uncertainty_and_adjoint's bounds"""
    gen = _gen("guard gambling")
    B, sp, k = 2, (8, 12, 4), (4, 4, 2)
    x = _randn((B,) + sp + (2,), gen, 3.0)
    base = _randn((B,) + sp + (2,), gen)
    N = (sp[0] // k[0]) * (sp[1] // k[1]) * (sp[2] // k[2])
    gu = _randn((B, N), gen)

    def run(wrap):
        xd = wrap(x)
        u = ops.gambling_uncertainty(xd, k, fast=fast)
        gl = wrap(base)
        ops.gambling_uncertainty_bwd(xd, k, wrap(gu), gl, fast=fast)
        torch.cuda.synchronize()
        return {"u": u, "g_logits": gl}

    what = f"gambling uncertainty {sp} k={k} fast={fast}"
    names, got, plain = run_both(run, what)
    assert_finite_under_guard(got, plain, what)
    ld = x.double().permute(0, 4, 1, 2, 3).requires_grad_(True)
    ur = uncertainty_ref(ld, k)
    (ur * gu.double()).sum().backward()
    rel = lambda a, r: float((a.double() - r).norm() / r.norm().clamp_min(1e-30))     # noqa: E731
    tol_u, tol_g = (2e-5, 1e-4) if fast else (2e-6, 2e-5)
    assert rel(got["u"], ur.detach()) <= tol_u
    assert rel((got["g_logits"] - base).permute(0, 4, 1, 2, 3), ld.grad) <= tol_g
    assert_same_bits(got, plain, what)
    tf = "true" if fast else "false"
    expect(names, [f"gambling_uncertainty_kernel<{tf}, false>", f"gambling_uncertainty_kernel<{tf}, true>"], what)
