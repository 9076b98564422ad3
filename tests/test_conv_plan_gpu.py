"""The corner the forward plan closes: an LDS-served shape for which the old split query answered > 1 (bf16 k=3 64 -> 64 at 24^3,
B = 1).  The launch runs conv_k3_lds_kernel, which writes y and no slab, so a deferred finish there would hand the norm slabs nothing
wrote.  With every torch.empty poisoned with NaN (the fixture of test_dispatch_parity_gpu)."""
import numpy as np
import pytest
import torch

from test_dispatch_parity_gpu import launched, poisoned  # noqa: F401  (poisoned: a fixture)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from dycon_paper_replication_amd import _lib, ops
    from dycon_paper_replication_amd._lib import BF16, CONV_K3, CONV_LDS, DyconLibraryError

DEV = "cuda:0"


def test_defer_finish_on_an_lds_shape(poisoned):  # noqa: F811
    B, sp, C = 1, (24, 24, 24), 64
    plan = ops.conv_plan(BF16, CONV_K3, 0, 0, B, *sp, C, C, C)
    assert (plan.family, plan.splits, plan.workspace) == (CONV_LDS, 1, 0)
    gen = torch.Generator(device=DEV).manual_seed(24)
    w = (torch.randn((C, C, 3, 3, 3), generator=gen, device=DEV) / float(np.sqrt(27 * C)))
    b = torch.randn((C,), generator=gen, device=DEV)
    x = torch.randn((B,) + sp + (C,), generator=gen, device=DEV).bfloat16()
    wf = ops.pack_bfrag(w, torch.bfloat16, 27, C, C, C, 1, 27, 0, C * 27)
    names = set()
    with launched(names):
        y = ops.conv_gemm(x, wf, b, CONV_K3, C, C)
        yd, dc = ops.conv_gemm(x, wf, b, CONV_K3, C, C, defer_finish=True)
    assert dc is None
    assert bool(torch.isfinite(y.float()).all())
    assert torch.equal(y, yd)
    convs = [n for n in names if n.startswith(("conv_", "splitk_"))]
    assert convs and all(n.startswith("conv_k3_lds_kernel") for n in convs), sorted(names)
    # the C ABI itself: a deferred finish needs slabs, and this plan has none -- refused before anything is launched
    out, ws = torch.empty_like(y), torch.empty(4 << 20, device=DEV)      # room for the 3 slabs the old query asked for
    torch.cuda.synchronize()
    prof = ops.KernelProfiler()
    try:
        with pytest.raises(DyconLibraryError, match="defer_finish needs a split-K shape"):
            _lib.call("dycon_conv_gemm_ex", x.data_ptr(), wf.data_ptr(), b.data_ptr(), out.data_ptr(), BF16, CONV_K3, 0, 0, B, *sp, C, C, C,
                      ws.data_ptr(), ws.numel() * 4, 1, torch.cuda.current_stream().cuda_stream)
        assert prof.count() == 0
    finally:
        prof.close()
