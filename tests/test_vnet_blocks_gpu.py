"""networks.VNet's building blocks on the GPU against an fp64 twin, and the fused up-sampling convolution (dycon_upconv_k3)
against the composition of the two launches it replaces.

The fp64 twin of a case is the block's own parameter container (an nn.Sequential of torch's Conv3d / ConvTranspose3d / norm / ReLU /
Upsample modules at the reference's indices) run on the CPU in float64 -- relu(conv(x) + x) for the residual block -- once per
case, shared by the fp32 and bf16 tests.  It is tied to the reference's own fp64 run through the fixture
(tests/golden/vnet_blocks.npz: strided samples and the 2-norm of every tensor, to 1e-6), and EVERY element of every tensor is then
compared against it:
fp32: the project's rule (tests/ref64.py and the parity tests): max |got - ref64| <= 1e-4 x the tensor's max-abs.
bf16: twice the error the reference itself makes when run with bf16 modules, parameters and inputs on the CPU, per tensor, as
stored in the fixture (the factor 2: fp32 accumulation over all 27 taps and one rounding at the store here, per-op rounding there).
The scale of a tensor is `stat[0]` of the fixture (its fp64 max-abs; see make_golden_vnet_blocks.py for the analytically zero bias
gradients).  A NaN / Inf fails.
"""
import copy
import importlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from test_vnet_blocks_cpu import B, CASE_IDS, CASES, case_tensors, fixture_keys, sample_stride

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_TWINS = {}


@pytest.fixture(scope="module")
def gold():
    return load_golden("vnet_blocks")


@pytest.fixture(scope="module")
def V():
    return importlib.import_module("dycon_paper_replication_amd.networks.VNet")


def _twin(gold, V, i):
    """fp64 tensors of case i (y, gx, g.<param>, batchnorm: buf.<buffer>, y_eval), computed once and held to the fixture"""
    if i in _TWINS:
        return _TWINS[i]
    name, cls, args, dhw, norm = CASES[i]
    keys, shapes = fixture_keys(gold, name)
    sd, x, gy = case_tensors(i, keys, shapes)
    blk = getattr(V, cls)(*args, normalization=norm)
    blk.load_state_dict(sd, strict=True)
    seq = copy.deepcopy(blk.conv).double().train()
    run = (lambda t: F.relu(seq(t) + t)) if cls == "ResidualConvBlock" else seq
    xr = x.double().requires_grad_(True)
    y = run(xr)
    y.backward(gy.double())
    out = {"y": y.detach(), "gx": xr.grad}
    for k, p in seq.named_parameters():
        out["g.conv." + k] = p.grad
    if norm == "batchnorm":
        for k, b in seq.named_buffers():
            out["buf.conv." + k] = b.detach().clone().double()
        seq.eval()
        with torch.no_grad():
            out["y_eval"] = run(x.double())
    for k, t in out.items():
        if k.endswith("num_batches_tracked"):
            continue
        flat = t.reshape(-1)
        scale, norm2 = float(gold[f"{name}/{k}/stat"][0]), float(gold[f"{name}/{k}/stat"][1])
        ref = torch.from_numpy(gold[f"{name}/{k}"]).double()
        assert float((flat[::sample_stride(flat.numel())] - ref).abs().max()) <= 1e-6 * scale, (name, k, "twin != reference fp64 run")
        assert abs(float(flat.norm()) - norm2) <= 1e-6 * max(norm2, scale), (name, k, "twin norm")
    _TWINS[i] = out
    return out


def _check(gold, twin, name, key, got, dtype):
    got = got.detach().double().cpu().reshape(-1)
    assert bool(torch.isfinite(got).all()), f"{name} {key}: non-finite values"
    ref = twin[key].reshape(-1)
    assert got.numel() == ref.numel(), f"{name} {key}: {got.numel()} elements"
    scale, _norm, _e32, ebf = (float(v) for v in gold[f"{name}/{key}/stat"])
    tol = 1e-4 if dtype == torch.float32 else 2.0 * ebf
    err = float((got - ref).abs().max()) / scale          # every element
    print(f"{name} {key} {str(dtype)[6:]}: err {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (name, key, err, tol)


def _build(V, gold, i, dtype):
    name, cls, args, dhw, norm = CASES[i]
    keys, shapes = fixture_keys(gold, name)
    sd, x, gy = case_tensors(i, keys, shapes)
    m = getattr(V, cls)(*args, normalization=norm, dtype=dtype)
    m.load_state_dict(sd, strict=True)          # the state_dict the reference class loaded in the generator
    return m.to(DEV), x.to(DEV), gy.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_block_forward_backward(gold, V, i, dtype):
    name, cls, args, dhw, norm = CASES[i]
    twin = _twin(gold, V, i)
    m, x, gy = _build(V, gold, i, dtype)
    m.train()
    x.requires_grad_(True)
    y = m(x)
    assert y.dtype == dtype and y.shape == gy.shape and y.is_contiguous(memory_format=torch.channels_last_3d)
    y.backward(gy.to(dtype))
    _check(gold, twin, name, "y", y, dtype)
    _check(gold, twin, name, "gx", x.grad, dtype)
    for k, p in m.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32, k
        _check(gold, twin, name, "g." + k, p.grad, dtype)
    if norm == "batchnorm":
        for k, b in m.named_buffers():      # running statistics after one training forward, then the .eval() forward
            if k.endswith("num_batches_tracked"):
                assert int(b) == 1
            else:
                _check(gold, twin, name, "buf." + k, b, dtype)
        m.eval()
        with torch.no_grad():
            _check(gold, twin, name, "y_eval", m(x.detach()), dtype)


def test_input_without_gradient_and_bf16_parameters(gold, V):
    i = CASE_IDS.index("up_c16_groupnorm")
    m, x, gy = _build(V, gold, i, torch.bfloat16)
    y = m(x)                                   # the input asks for no gradient: parameter gradients only
    y.backward(gy.to(torch.bfloat16))
    assert x.grad is None and all(p.grad is not None for p in m.parameters())
    with pytest.raises(TypeError, match="fp32"):
        m.bfloat16()(x)


# the three 32 -> 16 shapes in both storage types (chunked k-steps), and 16 / 48 input channels at the odd shape: in bf16 those keep
# all channels resident and run the flat-K loop, whose last k-step runs past the 27 taps (48: 40.5 chunks of 32)
UPCONV_CASES = [((5, 6, 7), 32, "fp32"), ((5, 6, 7), 32, "bf16"), ((1, 3, 4), 32, "fp32"), ((1, 3, 4), 32, "bf16"),
                ((9, 9, 17), 32, "fp32"), ((9, 9, 17), 32, "bf16"), ((5, 6, 7), 16, "bf16"), ((5, 6, 7), 48, "bf16"),
                ((5, 6, 7), 16, "fp32"), ((5, 6, 7), 48, "fp32")]


@pytest.mark.parametrize("dhw,Cin,dt", UPCONV_CASES, ids=[f"{'x'.join(map(str, c[0]))}-c{c[1]}-{c[2]}" for c in UPCONV_CASES])
def test_upconv_k3_equals_resize_then_conv(dhw, Cin, dt):
    """dycon_upconv_k3 through the C ABI against trilinear_fwd(align_corners=False) -> conv_gemm on the same operands: pins the
    zero padding on the UP-SAMPLED grid independently of the module code.  fp32: the 1e-4 rule; this is the branch that pins the
    semantics.  bf16: ASSUMING both forms produce the same bf16 up-sampled operand (same taps, same association order, rounded at
    the same point; not asserted separately), the results differ by the fp32 summation order alone, which can move the single
    rounding at the store by one bf16 ulp of the value: at most 2^-7 of the tensor's max-abs."""
    from dycon_paper_replication_amd import ops
    from dycon_paper_replication_amd._lib import CONV_K3
    dtype = torch.float32 if dt == "fp32" else torch.bfloat16
    Cout = 16
    gen = torch.Generator().manual_seed(77 + dhw[0] + Cin)
    x = torch.randn((B,) + dhw + (Cin,), generator=gen).to(DEV).to(dtype)
    w = (torch.randn((Cout, Cin, 3, 3, 3), generator=gen) * (2.0 / (27 * Cin)) ** 0.5).to(DEV)
    bias = (0.1 * torch.randn(Cout, generator=gen)).to(DEV)
    wf = ops.pack_bfrag(w, dtype, 27, Cin, Cout, Cout, 1, 27, 0, Cin * 27)
    fused = ops.upconv_k3(x, wf, bias, Cout)
    up = ops.trilinear_fwd(x, tuple(2 * s for s in dhw), False)
    comp = ops.conv_gemm(up, wf, bias, CONV_K3, Cout, Cout)
    torch.cuda.synchronize()
    assert fused.shape == comp.shape == (B,) + tuple(2 * s for s in dhw) + (Cout,)
    assert bool(torch.isfinite(fused.float()).all())
    err = float((fused.double() - comp.double()).abs().max()) / float(comp.double().abs().max())
    tol = 1e-4 if dtype == torch.float32 else 2.0 ** -7
    print(f"upconv_k3 {dhw} {Cin} {dtype}: err {err:.3e} (bound {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_upsampling_both_dispatch_branches(gold, V, dtype):
    """Upsampling's two forward forms (the fused kernel, resize -> convolution) through the module, whichever the dispatch picks"""
    i = CASE_IDS.index("up_seam_groupnorm")
    m, x, _ = _build(V, gold, i, dtype)
    with torch.no_grad():
        m.fused_upconv = True
        y_fused = m(x)
        m.fused_upconv = False
        y_comp = m(x)
    err = float((y_fused.double() - y_comp.double()).abs().max()) / float(y_comp.double().abs().max())
    print(f"Upsampling fused vs composition {dtype}: {err:.3e}")
    assert err <= (1e-4 if dtype == torch.float32 else 2 * float(gold["up_seam_groupnorm/y/stat"][3]))


@pytest.mark.parametrize("Cin", [1, 24])
def test_upconv_k3_refuses_unsupported_channels(Cin):
    from dycon_paper_replication_amd import ops
    from dycon_paper_replication_amd._lib import DyconLibraryError
    x = torch.zeros((1, 2, 2, 2, Cin), device=DEV)
    with pytest.raises(DyconLibraryError, match="unsupported channels"):
        ops.upconv_k3(x, torch.zeros(27 * 32 * 16, device=DEV), None, 16)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_channels_last_input_is_used_in_place(gold, V, dtype):
    from dycon_paper_replication_amd.networks._blocks import _ndhwc
    i = CASE_IDS.index("down_groupnorm")
    m, x, _ = _build(V, gold, i, dtype)
    x = x.to(dtype)
    xcl = x.contiguous(memory_format=torch.channels_last_3d)
    assert _ndhwc(xcl, dtype).data_ptr() == xcl.data_ptr()          # no copy, no cast
    with torch.no_grad():
        y0, y1 = m(x), m(xcl)
        assert torch.equal(y0, y1)
        # the output is the next block's operand as it stands
        assert y1.is_contiguous(memory_format=torch.channels_last_3d) and y1.dtype == dtype
        assert _ndhwc(y1, dtype).data_ptr() == y1.data_ptr()
        nxt = V.UpsamplingDeconvBlock(64, 32, normalization="groupnorm", dtype=dtype).to(DEV)
        y2 = nxt(y1)
        assert y2.shape == x.shape[:1] + (32,) + x.shape[2:] and y2.is_contiguous(memory_format=torch.channels_last_3d)


def test_packed_weights_follow_the_parameters(V):
    torch.manual_seed(5)
    m = V.ConvBlock(1, 16, 16, normalization="none").to(DEV)
    x = torch.randn(1, 16, 6, 6, 6, device=DEV)
    with torch.no_grad():
        y = m(x)
        m.conv[0].weight.mul_(2.0)
        m.conv[0].bias.mul_(2.0)
        y2 = m(x)
    assert float((y2 - 2 * y).abs().max()) <= 1e-5 * float(y2.abs().max())      # relu(2z) = 2 relu(z); x2 is exact in fp32


def test_three_level_chain(V):
    """down, down, Upsampling, UpsamplingDeconvBlock with the skip adds done by torch: forward + backward once at 16^3"""
    torch.manual_seed(11)
    dt = torch.bfloat16
    stem = V.ConvBlock(1, 1, 16, normalization="groupnorm", dtype=dt).to(DEV)
    d1 = V.DownsamplingConvBlock(16, 32, normalization="groupnorm", dtype=dt).to(DEV)
    r1 = V.ResidualConvBlock(2, 32, 32, normalization="groupnorm", dtype=dt).to(DEV)
    d2 = V.DownsamplingConvBlock(32, 64, normalization="groupnorm", dtype=dt).to(DEV)
    u2 = V.Upsampling(64, 32, normalization="groupnorm", dtype=dt).to(DEV)
    u1 = V.UpsamplingDeconvBlock(32, 16, normalization="groupnorm", dtype=dt).to(DEV)
    x = torch.randn(2, 1, 16, 16, 16, device=DEV)
    x1 = stem(x)
    x2 = r1(d1(x1))
    x3 = d2(x2)
    out = u1(u2(x3) + x2) + x1
    assert out.shape == (2, 16, 16, 16, 16) and out.dtype == dt
    out.float().square().mean().backward()
    for blk in (stem, d1, r1, d2, u2, u1):
        for k, p in blk.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), (type(blk).__name__, k)


def test_turnoff_drop(V):
    torch.manual_seed(3)
    net = V.VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=True, seed=1).to(DEV)
    twin = V.VNet(n_channels=1, n_classes=2, normalization="groupnorm", has_dropout=False, seed=1).to(DEV)
    twin.load_state_dict(net.state_dict())
    x = torch.randn(2, 1, 32, 32, 32, device=DEV)
    net.train()
    twin.train()
    with torch.no_grad():
        calls = net._drop_calls
        off = net(x, turnoff_drop=True)
        assert net._drop_calls == calls and net.has_dropout is True          # no mask drawn, the switch restored
        ref = twin(x)                                                         # training mode without dropout
        for a, b in zip(off, ref):
            assert torch.equal(a, b)
        net.eval()
        ev = net(x)                                                           # .eval(): dropout off (the GroupNorm body is mode-free)
        assert torch.equal(off[1], ev[1])
        net.train()
        # the default call: dropout on, and bit-identical with and without the keyword (same Philox offset: the call counter is rewound)
        calls = net._drop_calls
        d0 = net(x)
        net._drop_calls = calls
        d1 = net(x, turnoff_drop=False)
        assert torch.equal(d0[1], d1[1]) and torch.equal(d0[2], d1[2])
        assert not torch.equal(d0[1], off[1])
