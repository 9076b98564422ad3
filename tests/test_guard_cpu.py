"""The guarded allocator of tests/guard.py on CPU tensors (the device check relaxed): the detector detects.  The only deliberate
out-of-range writes are plain torch indexing into the helper's own base buffer."""
import re

import pytest
import torch

import guard
from guard import guarded

REAL = {n: getattr(torch, n) for n in ("empty", "empty_like", "zeros", "zeros_like")}


def _originals_in_place():
    return all(getattr(torch, n) is f for n, f in REAL.items())


def test_clean_allocate_write_check_passes():
    with guarded("cpu") as g:
        a = torch.empty((2, 3, 5, 7, 4), dtype=torch.float32)
        b = torch.empty_like(a)
        c = torch.empty(33, dtype=torch.bfloat16, device="cpu")
        d = torch.empty(2, 5, dtype=torch.int32)
        w = g.wrap(torch.arange(10, dtype=torch.int64))
        assert a.shape == (2, 3, 5, 7, 4) and a.dtype == torch.float32 and a.is_contiguous() and b.shape == a.shape
        assert a.data_ptr() % 64 == 0 and c.shape == (33,) and d.shape == (2, 5)
        # the poison: NaN in the float types, -1 in the integers
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(c.float()).all()) and bool((d == -1).all())
        assert torch.equal(w, torch.arange(10))
        a.fill_(1.0)
        b.copy_(a * 2)
        c.zero_()
        d[1, 4] = 7
        w[-1] = 3
        assert g.check() == 5 and guard.check() == 5
    assert _originals_in_place()
    assert g.check() == 5            # the guard stays usable after the block
    assert len(g.sites()) == 5 and all(k.startswith("tests/test_guard_cpu.py:") for k in g.sites())


@pytest.mark.parametrize("side", ["before", "after"])
def test_write_one_element_outside_is_reported(side):
    with guarded("cpu") as g:
        keep = torch.empty(100, dtype=torch.float32)
        t = torch.empty((3, 5), dtype=torch.float32); line = _line()         # noqa: E702
        t.zero_()
        assert g.check() == 2
        rec = g.allocs[-1]
        assert rec.shape == (3, 5) and rec.nbytes == 60 and rec.band == guard.BAND
        flat = rec.base[rec.band - 4:rec.band + rec.nbytes + 4].view(torch.float32)     # the interior and one element either side
        assert torch.equal(flat[1:-1].view(3, 5), t)
        flat[0 if side == "before" else -1] = 1.0        # plain torch indexing through the base buffer
        with pytest.raises(AssertionError) as err:
            g.check()
    msg = str(err.value)
    print(msg)
    assert "1 guard band(s) of 2 allocations damaged" in msg
    lines = msg.splitlines()[1:]
    assert len(lines) == 1
    assert lines[0].startswith(f"tests/test_guard_cpu.py:{line}: empty (3, 5) float32: band {side} the tensor damaged")
    # 1.0f = 00 00 80 3f: all four bytes differ from 0xFF
    want = "bytes -4 .. -1 from its edge, 4 bytes" if side == "before" else "bytes +0 .. +3 from its edge, 4 bytes"
    assert lines[0].endswith(want), lines[0]
    assert bool((keep != keep).all())        # (the other allocation is untouched)
    assert _originals_in_place()


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_call_site_is_the_frame_inside_the_package(tmp_path, monkeypatch):
    """an allocation made by package code is reported at the package's line, not at the test's"""
    pkg = tmp_path / "dycon_paper_replication_amd"
    pkg.mkdir()
    src = pkg / "fake_ops.py"
    src.write_text("import torch\n\n\ndef make(n):\n    return torch.empty(n, dtype=torch.uint8)\n")
    monkeypatch.setattr(guard, "ROOT", str(tmp_path))
    monkeypatch.setattr(guard, "PACKAGE", str(pkg) + "/")
    ns = {}
    exec(compile(src.read_text(), str(src), "exec"), ns)
    with guarded("cpu") as g:
        t = ns["make"](7)
        g.allocs[-1].base[g.allocs[-1].band + 7] = 0        # one byte past the end
        with pytest.raises(AssertionError, match=re.escape("dycon_paper_replication_amd/fake_ops.py:5: empty (7,) uint8: band after the tensor "
                                                           "damaged, bytes +0 .. +0 from its edge, 1 bytes")):
            g.check()
    assert t.numel() == 7


def test_zeros_keeps_its_interior_zero():
    with guarded("cpu") as g:
        z = torch.zeros(1000, dtype=torch.float64)
        zl = torch.zeros_like(torch.ones(4, 6, dtype=torch.int32))
        assert z.dtype == torch.float64 and float(z.abs().max()) == 0 and zl.shape == (4, 6) and int(zl.abs().max()) == 0
        for rec in g.allocs:
            assert bool((rec.base[:rec.band] == 0xFF).all()) and bool((rec.base[rec.band + rec.nbytes:] == 0xFF).all())
            assert bool((rec.base[rec.band:rec.band + rec.nbytes] == 0).all())
        assert g.check() == 2


def test_band_holds_four_planes_and_keeps_alignment():
    assert guard.band_bytes((1, 25, 26, 23, 16), 2) == guard.BAND                    # 4 planes = 76 544 B
    big = guard.band_bytes((2, 41, 200, 200, 32), 2)                                 # 4 planes = 10 240 000 B
    assert big >= 4 * 200 * 200 * 32 * 2 and big % 512 == 0 and big - 4 * 200 * 200 * 32 * 2 < 512
    assert guard.band_bytes((3, 7), 4) == guard.BAND and guard.band_bytes((1 << 26,), 4) == guard.BAND
    with pytest.raises(AssertionError, match="fewer than 64 rows"):
        guard.band_bytes((5, 1 << 20), 4)
    with guarded("cpu") as g:
        t = torch.empty((1, 2, 300, 300, 8), dtype=torch.float32)
        assert g.allocs[-1].band == guard.band_bytes(t.shape, 4) > guard.BAND
        assert (t.data_ptr() - g.allocs[-1].base.data_ptr()) % 512 == 0


def test_other_requests_pass_through_untouched():
    nc = torch.ones(2, 3, 4, 5).permute(0, 2, 3, 1)                 # not contiguous
    with guarded("cpu") as g:
        a = torch.empty_like(nc)                                    # preserve_format of a permuted tensor: not contiguous
        b = torch.empty((2, 3, 4, 5), memory_format=torch.channels_last)
        c = torch.empty((3, 3), layout=torch.sparse_coo)
        d = torch.zeros((3, 3), layout=torch.sparse_coo)
        e = torch.empty(5, requires_grad=True)
        f = torch.empty((2, 2), out=torch.ones(4))
        h = torch.empty((0, 4))
        i = torch.zeros(3, dtype=torch.bool)
        assert len(g.allocs) == 0
        assert a.stride() == nc.stride() and not a.is_contiguous() and b.is_contiguous(memory_format=torch.channels_last)
        assert c.layout == torch.sparse_coo and d.layout == torch.sparse_coo and e.requires_grad and f.shape == (2, 2)
        assert h.shape == (0, 4) and i.dtype == torch.bool and not bool(i.any())
        j = torch.empty_like(nc, memory_format=torch.contiguous_format)      # ... asked to be contiguous: guarded
        assert len(g.allocs) == 1 and j.is_contiguous() and j.shape == nc.shape
        assert g.check() == 1
    with guarded() as g:                                            # the default guards CUDA requests only
        k = torch.empty(10)
        assert len(g.allocs) == 0 and k.shape == (10,)


def test_originals_restored_after_an_exception():
    with pytest.raises(RuntimeError, match="boom"):
        with guarded("cpu"):
            assert not _originals_in_place()
            raise RuntimeError("boom")
    assert _originals_in_place()
    t = torch.empty(3)
    assert t.untyped_storage().nbytes() == 12
