"""Guard bands around every tensor the package allocates: a test-side allocator wrapper that shows where the kernels touch memory.

    with guarded() as g:
        x = g.wrap(x)                # inputs, labels, weights the test built: copied into a guarded allocation
        y = ops.something(x)         # every output / workspace the package allocates inside gets bands too
    g.check()                        # every band of every allocation made so far is still all 0xFF

While active, guarded() replaces the allocation calls through which dycon_paper_replication_amd/{ops,engine,trainer,aspp}.py make the
tensors that reach the C ABI:

    torch.empty        outputs, workspaces (ops._ws), split-K slabs, packed weights, statistics, loss accumulators (ops.py, engine.py,
                       aspp.py)
    torch.empty_like   outputs shaped like an input (ops.py; trainer.py's contiguous staging copies)
    torch.zeros        the trainer's flat parameter / teacher / gradient / momentum arenas and its accumulators (trainer.py)
    torch.zeros_like   the zero gradients of an absent loss branch (engine.py)

They were found with a search of the four files for `torch.<factory>(`, `.new_*(`, `.clone(`, `.contiguous(` and `.to(`.  The other
tensor-making calls found are not intercepted: `.contiguous()` / `.to()` / `.clone()` of caller-provided tensors (a test passes these
through wrap() instead), torch.stack(...).contiguous() of the eval-mode BatchNorm statistics (2C floats made by torch, read by one
kernel), torch.from_numpy(...).to(device) of the pack-job table and the host-side pinned flag.

A request is guarded when it is for the guarded device type (CUDA; the CPU self-test relaxes that), strided and contiguous, and of a
plain numeric dtype; everything else goes to the real function untouched.  For n bytes the replacement allocates ONE uint8 buffer
of band + n + band bytes with the real torch.empty under the caller's stream context, fills all of it with 0xFF (zeros*: the bands
with 0xFF, the interior with 0), synchronises the device (so the fill cannot race with a side stream's first write: this is about
addresses, not stream ordering) and returns the interior viewed with the requested dtype and shape.  0xFF.. is NaN in bf16 / fp32 /
fp64, 255 in uint8 and -1 in int32 / int64: one pattern poisons every type, so an out-of-bounds READ that reaches the arithmetic
turns the result into NaN, and an out-of-bounds WRITE changes a band byte that check() finds.  Reads and writes that land in a band
stay inside a live allocation: nothing here can fault.

The band is 1 MiB, raised where needed to 4 z-planes (4 * H * W * C elements) of a (B, D, H, W, C) tensor and rounded up to 512 B, so
data_ptr() keeps the allocator's 512-byte alignment that production sees.  Four planes is the z-extent of every voxel tile of the
library (CL_TZ, UC_TZ, CH_T); the helper asserts that the band also holds 64 GEMM rows (CT_BM) of the tensor's last axis.

What this cannot see: a read past the end whose value is discarded by a select (not by arithmetic) leaves no trace; a write of 0xFF
bytes onto a band, and any access that reaches beyond the band, are invisible too.
"""
import contextlib
import os
import sys

import torch

BAND = 1 << 20
ALIGN = 512
TILE_PLANES = 4              # CL_TZ, UC_TZ, CH_T
GEMM_ROWS = 64               # CT_BM
GROUP_BYTES = 256 << 20      # check(): bands are concatenated in groups of at most this many bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKAGE = os.path.join(ROOT, "dycon_paper_replication_amd") + os.sep
_HERE = os.path.abspath(__file__)
_NAMES = ("empty", "empty_like", "zeros", "zeros_like")
_REAL = {n: getattr(torch, n) for n in _NAMES}
_DTYPES = {torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float16, torch.bfloat16, torch.float32, torch.float64}
_ACTIVE = []


def _call_site():
    """file:line of the innermost frame inside the package; of the innermost frame outside this module where there is none"""
    f = sys._getframe(1)
    first = None
    while f is not None:
        fn = os.path.abspath(f.f_code.co_filename)
        if fn != _HERE:
            if first is None:
                first = (fn, f.f_lineno)
            if fn.startswith(PACKAGE):
                return f"{os.path.relpath(fn, ROOT)}:{f.f_lineno}"
        f = f.f_back
    fn, line = first if first is not None else ("?", 0)
    return f"{os.path.relpath(fn, ROOT) if fn.startswith(ROOT + os.sep) else fn}:{line}"


def band_bytes(shape, itemsize):
    """bytes of each band for a tensor of this shape: 1 MiB, or 4 z-planes of a 5-D channels-last tensor where that is more"""
    need = BAND
    if len(shape) == 5:
        need = max(need, TILE_PLANES * shape[2] * shape[3] * shape[4] * itemsize)
    band = (need + ALIGN - 1) // ALIGN * ALIGN
    assert band % ALIGN == 0 and band >= BAND
    if len(shape) == 5:
        assert band >= TILE_PLANES * shape[2] * shape[3] * shape[4] * itemsize, (shape, band)
    if len(shape) >= 2:      # (a 1-D tensor is a flat arena or workspace: it has no rows)
        assert band >= GEMM_ROWS * shape[-1] * itemsize, f"band of {band} B holds fewer than {GEMM_ROWS} rows of {tuple(shape)}"
    return band


class _Alloc:
    __slots__ = ("base", "band", "nbytes", "shape", "dtype", "site", "how")

    def __init__(self, base, band, nbytes, shape, dtype, site, how):
        self.base, self.band, self.nbytes, self.shape, self.dtype, self.site, self.how = base, band, nbytes, shape, dtype, site, how

    def bands(self):
        return (("before", self.base[:self.band]), ("after", self.base[self.band + self.nbytes:]))


class Guard:
    def __init__(self, device_type="cuda"):
        self.device_type = device_type
        self.allocs = []

    # ------------------------------------------------------------------------------------------------------------ allocation
    def _device(self, device):
        """the torch.device a factory call with this `device` argument allocates on"""
        if device is None:
            return _REAL["empty"](0).device
        return torch.device(device)

    def _eligible(self, dtype, device, layout, memory_format, kw):
        if kw:                                   # out=, names=, pin_memory=, requires_grad=: not a plain allocation
            return False
        if layout not in (None, torch.strided) or memory_format not in (None, torch.contiguous_format):
            return False
        return device.type == self.device_type and dtype in _DTYPES

    def alloc(self, shape, dtype, device, zero=False, how="empty", site=None):
        """a guarded tensor of this shape / dtype on this device; its interior is 0xFF.. (or 0 with `zero`)"""
        shape = tuple(int(s) for s in shape)
        itemsize = _REAL["empty"](0, dtype=dtype).element_size()
        n = itemsize
        for s in shape:
            n *= s
        band = band_bytes(shape, itemsize)
        base = _REAL["empty"](band + n + band, dtype=torch.uint8, device=device)
        base.fill_(0xFF)
        if zero and n:
            base[band:band + n].zero_()
        if device.type == "cuda":
            torch.cuda.synchronize(device)
        assert base.data_ptr() % itemsize == 0
        self.allocs.append(_Alloc(base, band, n, shape, dtype, site or _call_site(), how))
        return base[band:band + n].view(dtype).view(shape)

    def wrap(self, t):
        """a copy of t inside a guarded allocation (None stays None)"""
        if t is None:
            return None
        out = self.alloc(t.shape, t.dtype, t.device, how="wrap", site=_call_site())
        out.copy_(t)
        if t.device.type == "cuda":
            torch.cuda.synchronize(t.device)
        return out

    # ------------------------------------------------------------------------------------------------------------ the check
    def damaged(self):
        """True if any band byte of any allocation made so far is not 0xFF: one min over the concatenated bands (uint8: 255 is the
        largest value), in groups of at most GROUP_BYTES so the concatenation stays small"""
        mins, group, size = [], [], 0
        by_dev = {}
        for a in self.allocs:
            by_dev.setdefault(a.base.device, []).append(a)
        for allocs in by_dev.values():
            for a in allocs:
                for _, b in a.bands():
                    group.append(b)
                    size += b.numel()
                if size >= GROUP_BYTES:
                    mins.append(torch.cat(group).min().reshape(1).cpu())
                    group, size = [], 0
            if group:
                mins.append(torch.cat(group).min().reshape(1).cpu())
                group, size = [], 0
        return bool(mins) and int(torch.cat(mins).min()) != 0xFF

    def report(self):
        """one line per damaged band: call site, shape, dtype, side, first / last damaged byte relative to the tensor's edge
        (before: -1 is the byte just in front of element 0; after: 0 is the first byte past the last element), damaged bytes"""
        lines = []
        for a in self.allocs:
            for side, b in a.bands():
                bad = (b != 0xFF).nonzero().reshape(-1)
                if bad.numel() == 0:
                    continue
                first, last = int(bad[0]), int(bad[-1])
                if side == "before":
                    first, last = first - a.band, last - a.band
                lines.append(f"{a.site}: {a.how} {a.shape} {str(a.dtype).replace('torch.', '')}: band {side} the tensor damaged, "
                             f"bytes {first:+d} .. {last:+d} from its edge, {int(bad.numel())} bytes")
        return lines

    def check(self):
        if self.device_type == "cuda":
            torch.cuda.synchronize()
        if self.damaged():
            lines = self.report()
            raise AssertionError(f"out-of-bounds write: {len(lines)} guard band(s) of {len(self.allocs)} allocations damaged\n" + "\n".join(lines))
        return len(self.allocs)

    def sites(self):
        """{call site: number of allocations} of everything guarded so far"""
        out = {}
        for a in self.allocs:
            out[a.site] = out.get(a.site, 0) + 1
        return out

    # ------------------------------------------------------------------------------------------------------------ replacements
    @staticmethod
    def _size(args):
        if len(args) == 1 and not isinstance(args[0], int):
            return tuple(args[0])
        return tuple(args)

    def _factory(self, name, zero):
        real = _REAL[name]

        def factory(*args, dtype=None, device=None, layout=None, memory_format=None, **kw):
            try:
                shape = tuple(int(s) for s in self._size(args))
                dt_ = dtype if dtype is not None else torch.get_default_dtype()
                dev = self._device(device)
                ok = self._eligible(dt_, dev, layout, memory_format, kw) and all(s > 0 for s in shape)
            except (TypeError, ValueError, RuntimeError):
                ok = False
            if not ok:
                extra = dict(kw)
                for k, v in (("dtype", dtype), ("device", device), ("layout", layout), ("memory_format", memory_format)):
                    if v is not None:
                        extra[k] = v
                return real(*args, **extra)
            return self.alloc(shape, dt_, dev, zero=zero, how=name)
        return factory

    def _like(self, name, zero):
        real = _REAL[name]

        def like(inp, *, dtype=None, device=None, layout=None, memory_format=None, **kw):
            ok = torch.is_tensor(inp) and inp.layout == torch.strided
            if ok:
                dt_ = dtype if dtype is not None else inp.dtype
                dev = torch.device(device) if device is not None else inp.device
                dense = memory_format == torch.contiguous_format or (memory_format in (None, torch.preserve_format) and inp.is_contiguous())
                ok = dense and self._eligible(dt_, dev, layout, None, kw) and inp.numel() > 0
            if not ok:
                extra = dict(kw)
                for k, v in (("dtype", dtype), ("device", device), ("layout", layout), ("memory_format", memory_format)):
                    if v is not None:
                        extra[k] = v
                return real(inp, **extra)
            return self.alloc(inp.shape, dt_, dev, zero=zero, how=name)
        return like

    def install(self):
        torch.empty = self._factory("empty", False)
        torch.zeros = self._factory("zeros", True)
        torch.empty_like = self._like("empty_like", False)
        torch.zeros_like = self._like("zeros_like", True)


def restore():
    for n in _NAMES:
        setattr(torch, n, _REAL[n])


@contextlib.contextmanager
def guarded(device_type="cuda"):
    """the allocation calls of the module docstring guarded for the block; the Guard stays usable (check, report) afterwards.
    The originals are restored on exit, also when the body raises.  Not re-entrant."""
    assert not _ACTIVE, "guarded() is not re-entrant"
    g = Guard(device_type)
    _ACTIVE.append(g)
    g.install()
    try:
        yield g
    finally:
        restore()
        _ACTIVE.pop()


def wrap(t):
    """Guard.wrap of the active guarded() block"""
    return _ACTIVE[-1].wrap(t)


def check():
    """Guard.check of the active guarded() block"""
    return _ACTIVE[-1].check()
