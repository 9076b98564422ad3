"""utils.monitor / ops.similarity_histograms (dycon_simhist) on the GPU against the reference monitor's semantics
(code/utils/monitor.py:7-50), restated here: float64 normalise, matmul and / tau, torch.eq pair masks, np.histogram of the float32
values."""
import numpy as np
import pytest
import torch

from dycon_paper_replication_amd import _lib, ops
from dycon_paper_replication_amd.utils import monitor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = {torch.bfloat16: 1e-4, torch.float32: 2e-5}


def _sim64(feat, mask, tau, rows=None):
    """float64 similarities / tau of sample rows [r0, r1) against all rows, and the torch.eq pair mask"""
    x = feat.double()
    x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    r0, r1 = rows if rows is not None else (0, x.shape[1])
    sim = torch.matmul(x[:, r0:r1], x.transpose(1, 2)) / tau
    eq = torch.eq(mask[:, r0:r1, None], mask[:, None, :])
    return sim, eq


def _np_hist(values_f32, counts_of_values, bins):
    """np.histogram(values, bins) of a multiset given as distinct float32 values and their multiplicities (the bin of a value
    does not depend on how often it occurs; the range only on the extremes)"""
    if values_f32.size == 0:
        return np.histogram(values_f32, bins)
    return np.histogram(values_f32, bins, weights=counts_of_values)


def _exact_oracle(feat, mask, tau, bins):
    sim, eq = _sim64(feat, mask, tau)
    out = []
    for sel in (eq, ~eq):
        u, c = torch.unique(sim[sel].float(), return_counts=True)
        out.append(_np_hist(u.cpu().numpy(), c.cpu().numpy(), bins))
    return out


def _signed_unit_rows(B, N, Dm, dtype, seed):
    """rows with +-0.5 on four coordinates: exact in bf16 and fp32, norm exactly 1; with tau = 0.5 every similarity is a
    multiple of 0.5 (0 sits on edge 25 of [-2, 2] at 50 bins)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(B, N, Dm)
    idx = torch.stack([torch.randperm(Dm, generator=g)[:4] for _ in range(B * N)]).reshape(B, N, 4)
    sgn = torch.randint(0, 2, (B, N, 4), generator=g).float() * 2 - 1
    x.scatter_(2, idx, 0.5 * sgn)
    m = torch.randint(0, 2, (B, N), generator=g).float()
    return x.to(DEV, dtype), m.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("Dm", [16, 256])
@pytest.mark.parametrize("N", [1, 37, 129, 1728])
@pytest.mark.parametrize("B", [1, 3])
def test_exact_parity(dtype, Dm, N, B):
    x, m = _signed_unit_rows(B, N, Dm, dtype, seed=N * 7 + Dm + B)
    counts, edges, _ = ops.similarity_histograms(x, m, tau=0.5, bins=50)
    counts, edges = counts.cpu().numpy(), edges.cpu().numpy()
    for k, (ec, ee) in enumerate(_exact_oracle(x, m, 0.5, 50)):
        if ec.sum() == 0:       # empty set: numpy's float64 linspace(0, 1)
            np.testing.assert_allclose(edges[k], ee, rtol=0, atol=1e-7)
            assert not counts[k].any()
            continue
        assert ee.dtype == np.float32
        np.testing.assert_array_equal(counts[k], ec.astype(np.int64), err_msg=f"set {k}")
        np.testing.assert_array_equal(edges[k].view(np.int32), ee.view(np.int32), err_msg=f"set {k} edges")
    assert counts.sum() == B * N * N


def _check_bounds(x, m, tau, bins, counts, edges, minmax, chunk=None):
    """totals exact; extremes within delta of the float64 oracle; per bin |dcount| <= oracle values within delta of its edges"""
    B, N, _ = x.shape
    d = DELTA[x.dtype]
    counts, edges, minmax = counts.cpu(), edges.cpu().double(), minmax.cpu().double()
    npos = sum(int((m[b] == v).sum()) ** 2 for b in range(B) for v in torch.unique(m[b]))
    assert int(counts[0].sum()) == npos and int(counts[1].sum()) == B * N * N - npos
    ref = torch.zeros(2, bins, dtype=torch.int64)
    near = torch.zeros(2, bins + 1, dtype=torch.int64)
    lo = torch.full((2,), float("inf"), dtype=torch.float64)
    hi = -lo
    e_dev = edges.to(DEV)
    chunk = chunk or N
    for r0 in range(0, N, chunk):
        sim, eq = _sim64(x, m, tau, (r0, min(N, r0 + chunk)))
        for k, sel in enumerate((eq, ~eq)):
            v = sim[sel]
            if v.numel() == 0:
                continue
            lo[k] = min(lo[k], float(v.min()))
            hi[k] = max(hi[k], float(v.max()))
            idx = (torch.bucketize(v, e_dev[k], right=True) - 1).clamp_(0, bins - 1)
            ref[k] += torch.bincount(idx, minlength=bins).cpu()
            near[k] += torch.stack([((v - e).abs() <= d).sum() for e in e_dev[k]]).cpu()
    for k in range(2):
        if ref[k].sum() == 0:
            continue
        assert abs(float(minmax[2 * k]) - float(lo[k])) <= d and abs(float(minmax[2 * k + 1]) - float(hi[k])) <= d
        slack = near[k][:-1] + near[k][1:]
        dc = (counts[k] - ref[k]).abs()
        assert bool((dc <= slack).all()), (k, dc[dc > slack], slack[dc > slack])


def _random(B, N, Dm, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, Dm, generator=g) + 0.3 * torch.randn(B, 1, Dm, generator=g)     # a shared direction: skewed similarities
    m = (torch.rand(B, N, generator=g) < 0.3).float()
    return x.to(DEV, dtype), m.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,N,Dm", [(2, 1728, 256), (2, 2352, 256), (2, 100, 40), (2, 1000, 40)])
def test_random_embeddings(dtype, B, N, Dm):
    x, m = _random(B, N, Dm, dtype, seed=N + Dm)
    counts, edges, minmax = ops.similarity_histograms(x, m, tau=0.6, bins=50)
    _check_bounds(x, m, 0.6, 50, counts, edges, minmax)


def test_isles_size_no_quadratic_buffer():
    x, m = _random(2, 15680, 256, torch.bfloat16, seed=15680)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    counts, edges, minmax = ops.similarity_histograms(x, m, tau=0.6, bins=50)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 64 << 20
    _check_bounds(x, m, 0.6, 50, counts, edges, minmax, chunk=1024)


def test_empty_negatives():
    x, _ = _random(2, 300, 64, torch.float32, seed=1)
    m = torch.ones(2, 300, device=DEV)
    counts, edges, minmax = ops.similarity_histograms(x, m)
    assert int(counts[0].sum()) == 2 * 300 * 300 and not counts[1].any()
    np.testing.assert_allclose(edges[1].cpu().numpy(), np.linspace(0, 1, 51), rtol=0, atol=1e-7)
    assert minmax[2:].tolist() == [0.0, 1.0]


def test_single_row():
    x = torch.randn(1, 1, 32, device=DEV)
    counts, edges, minmax = ops.similarity_histograms(x, torch.zeros(1, 1, device=DEV), tau=0.6)
    v = np.float32(torch.nn.functional.normalize(x.double(), dim=-1).square().sum().item() / 0.6)
    assert abs(float(minmax[0]) - v) < 1e-6 and float(minmax[0]) == float(minmax[1])
    ec, ee = np.histogram(minmax[:1].cpu().numpy(), 50)        # range (v - 0.5, v + 0.5)
    np.testing.assert_array_equal(edges[0].cpu().numpy(), ee)
    np.testing.assert_array_equal(counts[0].cpu().numpy(), ec)
    assert not counts[1].any()


def test_zero_rows():
    x, m = _signed_unit_rows(2, 40, 16, torch.float32, seed=3)
    x[:, ::5] = 0            # zero rows: similarity 0 against everything, itself included
    counts, edges, _ = ops.similarity_histograms(x, m, tau=0.5)
    for k, (ec, ee) in enumerate(_exact_oracle(x, m, 0.5, 50)):
        np.testing.assert_array_equal(counts[k].cpu().numpy(), ec)
        np.testing.assert_array_equal(edges[k].cpu().numpy(), ee)


def test_mask_shapes_and_three_classes():
    x, _ = _random(2, 500, 64, torch.bfloat16, seed=4)
    m = torch.randint(0, 3, (2, 500), device=DEV).float()
    a = ops.similarity_histograms(x, m)
    b = ops.similarity_histograms(x, m[:, None, :])
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    _check_bounds(x, m, 0.6, 50, *a)


def test_bitwise_reproducible():
    x, m = _random(2, 2352, 256, torch.bfloat16, seed=5)
    a = ops.similarity_histograms(x, m)
    b = ops.similarity_histograms(x, m)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_bad_arguments_launch_nothing():
    x, m = _random(1, 64, 32, torch.float32, seed=6)
    lib = _lib.load()
    counts = torch.full((2, 300), -7, dtype=torch.int64, device=DEV)
    edges = torch.full((2, 301), -7.0, device=DEV)
    minmax = torch.full((4,), -7.0, device=DEV)
    ws = torch.empty(1 << 16, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    args = lambda D, bins, nws=ws.numel() * 4: (x.data_ptr(), m.data_ptr(), _lib.F32, 1, 64, D, 0.6, bins, counts.data_ptr(),  # noqa: E731
                                                 edges.data_ptr(), minmax.data_ptr(), ws.data_ptr(), nws, s)
    for bad in (args(32, 0), args(32, 257), args(300, 50), args(32, 50, 16)):
        assert lib.dycon_simhist(*bad) == -22
        assert lib.dycon_last_error()
    torch.cuda.synchronize()
    assert bool((counts == -7).all()) and bool((edges == -7).all()) and bool((minmax == -7).all())
    with pytest.raises(ValueError):
        ops.similarity_histograms(x, m, bins=0)
    with pytest.raises(_lib.DyconLibraryError):
        ops.similarity_histograms(torch.randn(1, 8, 300, device=DEV), torch.zeros(1, 8, device=DEV))


def test_monitor_writes_png(tmp_path):
    x, m = _random(2, 700, 64, torch.bfloat16, seed=8)
    counts, edges = monitor.monitor_similarity_distributions(x, m[:, None, :], 3, str(tmp_path))
    png = tmp_path / "epoch_3_similarity_distributions.png"
    assert png.exists() and png.read_bytes()[:4] == b"\x89PNG"
    c, e, _ = ops.similarity_histograms(x, m)
    np.testing.assert_array_equal(counts, c.cpu().numpy())
    np.testing.assert_array_equal(edges, e.cpu().numpy())


def test_monitor_on_trainer_outputs(tmp_path):
    """the documented one-line call on a step's outputs, after eager steps and after a replayed one"""
    from dycon_paper_replication_amd.synthetic import make_batch
    from dycon_paper_replication_amd.trainer import DyconTrainer, TrainConfig
    tr = DyconTrainer(TrainConfig(model="vnet", labeled_bs=1, batch_size=2, dtype=torch.bfloat16, seed=11), DEV)
    for it in range(4):                 # 1-2 eager, 3 recorded, 4 replayed
        vol, lab, _ = make_batch(900 + it, 2, (32, 32, 32))
        out = tr.step(vol.to(DEV), lab.to(DEV))
        if it in (0, 3):
            B, C = out["s_feat"].shape[0], out["s_feat"].shape[-1]
            feat = out["s_feat"].reshape(B, -1, C)
            counts, edges = monitor.monitor_similarity_distributions(feat[:2], out["mask"][:2], it, str(tmp_path))
            _check_bounds(feat[:2], out["mask"][:2], 0.6, 50, torch.from_numpy(counts), torch.from_numpy(edges),
                          ops.similarity_histograms(feat[:2], out["mask"][:2])[2])
    assert tr._rp is not None
    assert (tmp_path / "epoch_3_similarity_distributions.png").exists()
