"""Mask post-processing on the MI355X (csrc/morphology.hip, utils/morphology.py) against scipy.ndimage, bit for bit
(tests/morphology_ref.py): erosion, dilation, opening, closing, hole filling, the size filter, `PostProcess` chains and the per-class
form, under guard bands, and through the evaluators' `postprocess` keyword.  Every comparison is np.testing.assert_array_equal on
integers; only HD95 / ASD of the evaluators are held at the rtol 1e-12 of tests/test_components_gpu.py.

Every call takes a batch of 3 to 5 volumes, so a leak between rows or volumes shows.  A test asserts that scipy's result is neither
empty nor the input for the (input, operation) pairs meant to exercise a kernel:

    dilation            the density-0.35 volume, always
    erosion, opening    the density-0.93 volume while every axis is at least 2 n + 2 long (n erosions strip n layers off every face;
                        one layer of margin) and, beyond 3 iterations, for 6 neighbours only (at 18 / 26 neighbours the 7 % of
                        background erases everything within 7 steps)
    closing             the density-0.35 volume under the same axis rule (its erosion half eats from the faces)
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import components_ref as CR
import morphology_ref as MR
from guard import guarded

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import eval_classes as EC
from dycon_paper_replication_amd.utils import isles_eval as IE
from dycon_paper_replication_amd.utils import lesions as LE
from dycon_paper_replication_amd.utils import morphology as M
from dycon_paper_replication_amd.utils import surface_eval as SE
from dycon_paper_replication_amd.utils.sliding_window import Blend

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-12
STENCILS = {"erosion": M.binary_erosion, "dilation": M.binary_dilation, "opening": M.binary_opening, "closing": M.binary_closing}


@functools.lru_cache(maxsize=None)
def _batch(kind, shape):
    if kind == "random":
        b = MR.random_batch(shape)
    elif kind == "named":
        b = MR.named_batch(shape)
    elif kind == "holes":
        b = MR.hole_batch(shape)
    elif kind == "boundary":                                  # density 0.7, full, empty, density 0.93
        r = MR.random_batch(shape)
        b = np.stack([r[1], np.ones(shape, np.uint8), np.zeros(shape, np.uint8), r[2]])
    else:
        raise KeyError(kind)
    b.setflags(write=False)
    return b


@functools.lru_cache(maxsize=None)
def _ref(kind, shape, op, args):
    """scipy's result for every volume of a batch, computed once"""
    out = np.stack([MR.OPS[op](v, *args) for v in _batch(kind, shape)])
    out.setflags(write=False)
    return out


def _dev(a, dtype=np.uint8):
    """binary: any non-zero value is foreground, so an int64 batch carries 7s"""
    return torch.from_numpy(np.asarray(a).astype(dtype) * (7 if dtype == np.int64 else 1)).to(DEV)


def _host(t):
    assert t.is_cuda and t.dtype == torch.uint8
    return t.cpu().numpy()


def _exercised(shape, op, c, n):
    """index of the volume of a "random" batch on which scipy's result must be neither empty nor the input, or None"""
    if op == "dilation":
        return 0
    if min(shape) < 2 * n + 2:
        return None
    if op == "closing":
        return 0
    return 2 if (c == 1 or n <= 3) else None


def _check_stencils(kind, shape, connectivities, iterations, dtype=np.uint8):
    batch = _batch(kind, shape)
    t = _dev(batch, dtype)
    for c in connectivities:
        for n in iterations:
            for op, fn in STENCILS.items():
                want = _ref(kind, shape, op, (c, n))
                if kind == "random":
                    v = _exercised(shape, op, c, n)
                    if v is not None:
                        assert want[v].any() and not np.array_equal(want[v], batch[v]), (shape, op, c, n)
                got = fn(t, c, n)
                assert got.shape == t.shape
                np.testing.assert_array_equal(_host(got), want, err_msg=f"{kind} {shape} {op} connectivity {c} iterations {n}")


# ------------------------------------------------------------------------------------------------------------------- stencils
@pytest.mark.parametrize("connectivity", [1, 2, 3])
@pytest.mark.parametrize("shape", MR.SHAPES)
def test_stencils_equal_scipy_on_random_masks(shape, connectivity):
    _check_stencils("random", shape, (connectivity,), (1, 2, 3))


@pytest.mark.parametrize("shape", [MR.SHAPES[0], MR.SHAPES[2]])
def test_stencils_equal_scipy_on_named_cases(shape):
    """full then empty, corner then frame, the eight corners; the hollow boxes and the blocks on the faces"""
    _check_stencils("named", shape, (1, 2, 3), (1, 2))
    _check_stencils("holes", shape, (1, 2, 3), (1, 2))
    full, empty = _ref("named", shape, "erosion", (1, 1))[:2]
    assert full.sum() == np.prod([s - 2 for s in shape]) and not empty.any()        # a full volume erodes from its faces
    face = _batch("holes", shape)[4]
    closed = _ref("holes", shape, "closing", (1, 1))[4]
    assert face[0].any() and not closed[0].any() and closed.any()                    # closing's border rule


@pytest.mark.parametrize("shape", MR.BOUNDARY_SHAPES)
def test_stencils_at_word_boundaries(shape):
    """Z = 1, 63, 64, 65, 128, 129: the carry between words and the unused bits of a row's last word"""
    _check_stencils("boundary", shape, (1, 2, 3), (1, 2))
    t = _dev(_batch("boundary", shape))
    np.testing.assert_array_equal(_host(M.binary_dilation(t, 3, 3)), _ref("boundary", shape, "dilation", (3, 3)))
    # a dilation that left bits beyond Z set would feed them back through the carry of the next erosion
    np.testing.assert_array_equal(_host(M.PostProcess(M.Dilation(3, 2), M.Erosion(1, 1), M.Dilation(1, 1))(t)),
                                  np.stack([MR.chain(v, [("dilation", (3, 2)), ("erosion", (1, 1)), ("dilation", (1, 1))])
                                            for v in _batch("boundary", shape)]))


def test_eight_word_rows_and_seven_iterations():
    """(16, 16, 512): 8 words per row; 7 iterations is deeper than any halo a fused launch would carry"""
    _check_stencils("random", MR.LONG_ROW, (1, 3), (1, 7))
    _check_stencils("random", MR.SHAPES[0], (1, 2), (7,))


@pytest.mark.parametrize("dtype", [np.uint8, np.int64])
def test_input_forms(dtype):
    """uint8 and int64 with any non-zero value as foreground; numpy and CUDA inputs; one (X, Y, Z) volume"""
    shape = MR.SHAPES[2]
    _check_stencils("random", shape, (2,), (1,), dtype)
    batch = _batch("random", shape)
    as_numpy = batch.astype(dtype) * 3
    np.testing.assert_array_equal(_host(M.binary_opening(as_numpy, 1, 1)), _ref("random", shape, "opening", (1, 1)))
    np.testing.assert_array_equal(_host(M.binary_fill_holes(_batch("holes", shape).astype(dtype) * 5)), _ref("holes", shape, "fill_holes", (1,)))
    np.testing.assert_array_equal(_host(M.remove_small_components(as_numpy, 30)), _ref("random", shape, "min_size", (30, 3)))
    one = M.binary_closing(_dev(batch[0], dtype), 3, 1)
    assert one.shape == shape
    np.testing.assert_array_equal(_host(one), _ref("random", shape, "closing", (3, 1))[0])
    as_float = batch.astype(np.float32) * 0.25
    np.testing.assert_array_equal(_host(M.binary_erosion(torch.from_numpy(as_float).to(DEV), 1, 1)), _ref("random", shape, "erosion", (1, 1)))


# ------------------------------------------------------------------------------------------------------------------- fill_holes
@pytest.mark.parametrize("shape", MR.SHAPES[:2] + [MR.LONG_ROW])
def test_fill_holes_equals_scipy_on_random_masks(shape):
    batch = _batch("random", shape)
    t = _dev(batch)
    for c in (1, 2, 3):
        want = _ref("random", shape, "fill_holes", (c,))
        for v in (1, 2):                                         # densities 0.7 and 0.93 have holes
            filled = int(want[v].sum()) - int(batch[v].sum())
            print(f"{shape} connectivity {c} density {MR.DENSITIES[v]}: {filled} voxels filled")
            assert filled > 0
        np.testing.assert_array_equal(_host(M.binary_fill_holes(t, c)), want)


@pytest.mark.parametrize("shape", MR.SHAPES)
def test_fill_holes_named_cases(shape):
    holes = _batch("holes", shape)
    solid = MR.solid_box(shape)
    for c in (1, 2, 3):
        want = _ref("holes", shape, "fill_holes", (c,))
        got = _host(M.binary_fill_holes(_dev(holes), c))
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got[0], solid)                                  # the hollow box is filled
        np.testing.assert_array_equal(got[1], holes[1])                               # the tunnel keeps it open
        assert (got[2].sum() == solid.sum() - 1) if c == 1 else np.array_equal(got[2], holes[2])       # the diagonal step
        np.testing.assert_array_equal(got[3], MR.solid_box(shape, 60, 68))            # the cavity across z = 63 / 64
        np.testing.assert_array_equal(_host(M.binary_fill_holes(_dev(_batch("named", shape)), c)), _ref("named", shape, "fill_holes", (c,)))


@pytest.mark.parametrize("shape", MR.BOUNDARY_SHAPES)
def test_fill_holes_and_min_size_at_word_boundaries(shape):
    t = _dev(_batch("boundary", shape))
    for c in (1, 3):
        np.testing.assert_array_equal(_host(M.binary_fill_holes(t, c)), _ref("boundary", shape, "fill_holes", (c,)))
        np.testing.assert_array_equal(_host(M.remove_small_components(t, 4, c)), _ref("boundary", shape, "min_size", (4, c)))


# ------------------------------------------------------------------------------------------------------------------- size filter
@pytest.mark.parametrize("shape", MR.SHAPES + [MR.LONG_ROW])
def test_remove_small_components_equals_scipy(shape):
    batch = _batch("random", shape)
    t = _dev(batch)
    for c, k in ((3, 30), (1, 30), (2, 2), (3, 1)):
        want = _ref("random", shape, "min_size", (k, c))
        if k > 1:
            assert 0 < want[0].sum() < batch[0].sum()           # some components go, some stay
        np.testing.assert_array_equal(_host(M.remove_small_components(t, k, c)), want)
    np.testing.assert_array_equal(_host(M.remove_small_components(t, 1)), batch)
    assert not _host(M.remove_small_components(t, 1 << 40)).any()


def test_min_size_keeps_k_and_drops_k_minus_one():
    shape, k = MR.SHAPES[2], 9
    blobs = np.stack([MR.two_blobs(shape, k), MR.two_blobs(shape, k + 1), CR.named(shape)["full"], CR.named(shape)["empty"]])
    got = _host(M.remove_small_components(_dev(blobs), k, 1))
    np.testing.assert_array_equal(got, np.stack([MR.min_size(v, k, 1) for v in blobs]))
    assert [int(g.sum()) for g in got] == [k, 2 * k + 1, int(np.prod(shape)), 0]


# ------------------------------------------------------------------------------------------------------------------- pipelines
CHAINS = [
    ((M.Opening(1, 2), M.FillHoles(), M.MinSize(30), M.Largest()),
     [("opening", (1, 2)), ("fill_holes", (1,)), ("min_size", (30, 3)), ("largest", (3,))]),
    ((M.MinSize(30, 1), M.Closing(2, 1), M.FillHoles(3), M.Erosion(3, 1)),
     [("min_size", (30, 1)), ("closing", (2, 1)), ("fill_holes", (3,)), ("erosion", (3, 1))]),
    ((M.Largest(1), M.Dilation(1, 2)), [("largest", (1,)), ("dilation", (1, 2))]),
    ((), []),
]
ONE_BY_ONE = {M.Erosion: M.binary_erosion, M.Dilation: M.binary_dilation, M.Opening: M.binary_opening, M.Closing: M.binary_closing}


def _step_alone(step, t):
    if type(step) in ONE_BY_ONE:
        return ONE_BY_ONE[type(step)](t, step.connectivity, step.iterations)
    if isinstance(step, M.FillHoles):
        return M.binary_fill_holes(t, step.connectivity)
    if isinstance(step, M.MinSize):
        return M.remove_small_components(t, step.min_voxels, step.connectivity)
    return M.PostProcess(step)(t)


@pytest.mark.parametrize("shape", MR.SHAPES[:2])
def test_postprocess_chains_equal_the_scipy_chain(shape):
    batch = _batch("random", shape)
    for dtype in (np.uint8, np.int64):
        t = _dev(batch, dtype)
        for steps, ref_steps in CHAINS:
            want = np.stack([MR.chain(v, ref_steps) for v in batch])
            if steps:
                assert want[1].any() and not np.array_equal(want[1], batch[1]), steps
            got = M.PostProcess(*steps)(t)
            np.testing.assert_array_equal(_host(got), want, err_msg=repr(steps))
            alone = t
            for s in steps:                                      # the packed hand-off between steps changes nothing
                alone = _step_alone(s, alone)
            np.testing.assert_array_equal(_host(got), _host(alone) if steps else want)


def _launches(fn):
    """the kernel names of one call of fn, in launch order (the library's per-launch timer)"""
    lib = _lib.load()
    fn()
    torch.cuda.synchronize()
    _lib.call("dycon_kernel_timing", 1)
    try:
        fn()
        n = lib.dycon_kernel_timing_count()
        ms, st, nm = (ctypes.c_float * n)(), (ctypes.c_ulonglong * n)(), (ctypes.c_int * n)()
        assert lib.dycon_kernel_timing_fetch(0, n, ms, st, nm) == 0
    finally:
        _lib.call("dycon_kernel_timing", 0)
    return [lib.dycon_kernel_timing_name(nm[i]).decode().split("(")[0].split("<")[0].split()[-1] for i in range(n)]


def test_a_run_of_packed_steps_packs_once_and_unpacks_once():
    """and a stencil takes at most one launch per iteration: ceil(n / 4) with the halo of 4 rows"""
    t = _dev(_batch("random", MR.SHAPES[0]))
    names = _launches(lambda: M.PostProcess(M.Opening(1, 2), M.Closing(3, 1), M.FillHoles(), M.Erosion(2, 7))(t))
    print(names)
    assert names.count("morph_pack_kernel") == 1 and names[0] == "morph_pack_kernel"
    assert names.count("morph_unpack_kernel") == 2 and names[-1] == "morph_unpack_kernel"        # FillHoles unpacks the complement
    assert names.count("morph_stencil_kernel") == 4 + 2                                           # 2 + 2 + 1 + 1 iterations, then 7
    assert len(names) == 1 + 6 + 6 + 1                                                            # FillHoles: 6 launches
    names = _launches(lambda: M.PostProcess(M.MinSize(30), M.Dilation(1, 1), M.Largest())(t))
    assert names.count("morph_pack_kernel") == 1 and names.count("morph_unpack_kernel") == 1 and names.count("morph_stencil_kernel") == 1
    assert [n for n in names if n.startswith("morph_")] == ["morph_sizes_kernel", "morph_keep_kernel", "morph_pack_kernel",
                                                           "morph_stencil_kernel", "morph_unpack_kernel"]


CONTESTED = (19, 15, 52)


def _class_map(shape):
    """four classes: blobs one voxel apart (a dilation makes the neighbours claim the gap), and one-voxel layers of classes 2 and 3 in
    turn around one background voxel, CONTESTED: the closing of either class fills the whole stack, so both claim that voxel"""
    lm = np.zeros(shape, np.uint8)
    X, Y, Z = shape
    lm[2:8, 2:Y - 2, 3:40] = 1
    lm[9:14, 2:Y - 2, 3:40] = 2                                  # x = 8 is the gap between 1 and 2
    lm[15:X - 1, 2:Y - 2, 3:40] = 3                              # x = 14 between 2 and 3
    lm[4, 5, 10] = 0                                             # a hole in class 1
    lm[11, 6:9, 20:23] = 3                                       # class 3 inside class 2
    lm[0, 0, 0] = 2                                              # a speck
    x, y, z = np.indices((6, 10, 15))
    lm[16:22, 10:20, 45:60] = 2 + x % 2
    lm[CONTESTED] = 0
    return lm


def test_per_class_equals_its_restatement():
    shape = MR.SHAPES[1]
    maps = np.stack([_class_map(shape), np.roll(_class_map(shape), 7, axis=2), np.zeros(shape, np.uint8)])
    for steps, ref_steps in (((M.Closing(1, 1),), [("closing", (1, 1))]),
                             ((M.Opening(1, 1), M.FillHoles()), [("opening", (1, 1)), ("fill_holes", (1,))]),
                             ((M.Dilation(3, 1), M.MinSize(5)), [("dilation", (3, 1)), ("min_size", (5, 3))])):
        want = np.stack([MR.per_class(v, 4, lambda m: MR.chain(m, ref_steps)) for v in maps])       # noqa: B023
        claims = sum((MR.chain(maps[0] == c, ref_steps) != 0).astype(int) for c in (1, 2, 3))
        if isinstance(steps[0], M.Closing):                      # classes 2 and 3 claim the voxel: the smaller one gets it
            assert claims[CONTESTED] == 2 and want[0][CONTESTED] == 2 and (claims > 1).sum() > 100
            assert (want[0][16:22, 10:20, 45:60] == np.where(maps[0][16:22, 10:20, 45:60] > 0, maps[0][16:22, 10:20, 45:60], 2)).all()
        if isinstance(steps[0], M.Dilation):                     # both neighbours claim the gap between two blobs
            assert claims[8, 5, 10] == 2 and want[0][8, 5, 10] == 1 and want[0][14, 5, 10] == 2
        for dtype in (np.uint8, np.int64):
            got = M.PostProcess(*steps).per_class(torch.from_numpy(maps.astype(dtype)).to(DEV), 4)
            np.testing.assert_array_equal(_host(got), want, err_msg=repr(steps))
    one = M.PostProcess(M.Closing(1, 1)).per_class(maps[0], 4)                                         # numpy, (X, Y, Z)
    np.testing.assert_array_equal(_host(one), MR.per_class(maps[0], 4, lambda m: MR.closing(m, 1, 1)))
    np.testing.assert_array_equal(_host(M.PostProcess().per_class(maps, 3)), np.where(maps < 3, maps, 0))     # values outside 1..C-1 go


def test_same_bits_on_a_second_run_and_on_a_side_stream():
    shape = MR.SHAPES[0]
    t = _dev(_batch("random", shape))
    pp = M.PostProcess(M.Opening(2, 2), M.FillHoles(2), M.MinSize(20), M.Closing(1, 1))
    first = pp(t)
    torch.cuda.synchronize()
    for _ in range(2):
        assert torch.equal(pp(t), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        again = pp(t)
        lm = M.PostProcess(M.Closing(1, 1)).per_class(t, 2)
    side.synchronize()
    assert torch.equal(again, first)
    np.testing.assert_array_equal(_host(lm), _ref("random", shape, "closing", (1, 1)))
    np.testing.assert_array_equal(_host(first), np.stack([MR.chain(v, [("opening", (2, 2)), ("fill_holes", (2,)), ("min_size", (20, 3)),
                                                                        ("closing", (1, 1))]) for v in _batch("random", shape)]))


# ------------------------------------------------------------------------------------------------------------------- out of bounds
@pytest.mark.parametrize("shape", [(5, 6, 65), (6, 6, 129)])
def test_no_kernel_leaves_its_tensors(shape):
    """every entry point under guard bands: a write past the last word of a packed mask or the last voxel of a volume lands in a
    band and is found; a read of the row after the last meets 0xFF words, which a dilation or an erosion would carry into the result"""
    batch = _batch("boundary", shape)
    ref_steps = [("closing", (3, 2)), ("fill_holes", (1,)), ("min_size", (4, 3)), ("erosion", (1, 1))]
    lm = (batch * np.array([1, 2, 3, 1], np.uint8)[:, None, None, None]).astype(np.uint8)
    with guarded() as g:
        t = g.wrap(_dev(batch))
        got = {
            "erosion": M.binary_erosion(t, 3, 2), "dilation": M.binary_dilation(t, 3, 2), "opening": M.binary_opening(t, 2, 1),
            "closing": M.binary_closing(t, 1, 3), "fill_holes": M.binary_fill_holes(t, 1), "min_size": M.remove_small_components(t, 4),
            "chain": M.PostProcess(M.Closing(3, 2), M.FillHoles(), M.MinSize(4), M.Erosion(1, 1))(t),
            "per_class": M.PostProcess(M.Dilation(1, 1)).per_class(g.wrap(torch.from_numpy(lm).to(DEV)), 4),
        }
        n = g.check()
    print(f"{shape}: {n} guarded allocations checked")
    assert n >= 20
    want = {
        "erosion": _ref("boundary", shape, "erosion", (3, 2)), "dilation": _ref("boundary", shape, "dilation", (3, 2)),
        "opening": _ref("boundary", shape, "opening", (2, 1)), "closing": _ref("boundary", shape, "closing", (1, 3)),
        "fill_holes": _ref("boundary", shape, "fill_holes", (1,)), "min_size": _ref("boundary", shape, "min_size", (4, 3)),
        "chain": np.stack([MR.chain(v, ref_steps) for v in batch]),
        "per_class": np.stack([MR.per_class(v, 4, lambda m: MR.dilation(m, 1, 1)) for v in lm]),
    }
    for name in want:
        np.testing.assert_array_equal(_host(got[name]), want[name], err_msg=name)


def test_c_abi_under_guard_bands():
    """the entry points called directly on guarded buffers of exactly the documented sizes"""
    n_vol, X, Y, Z = 2, 4, 3, 129
    W = (Z + 63) // 64
    batch = np.stack([MR.smooth_mask((X, Y, Z), 0.7, 5), np.ones((X, Y, Z), np.uint8)])
    with guarded() as g:
        vol = g.wrap(_dev(batch))
        words, out, scratch, filled = (torch.empty((n_vol, X, Y, W), dtype=torch.int64, device=DEV) for _ in range(4))
        mask, kept = (torch.empty((n_vol, X, Y, Z), dtype=torch.uint8, device=DEV) for _ in range(2))
        root = torch.empty((n_vol, X, Y, Z), dtype=torch.int32, device=DEV)
        ws = torch.empty(int(_lib.load().dycon_morph_fill_workspace(n_vol, X, Y, Z)), dtype=torch.uint8, device=DEV)
        ws2 = torch.empty(int(_lib.load().dycon_cc_min_size_workspace(n_vol, X, Y, Z)), dtype=torch.uint8, device=DEV)
        _lib.call("dycon_morph_pack", vol.data_ptr(), 1, n_vol, X, Y, Z, 0, 0, words.data_ptr(), None)
        _lib.call("dycon_morph_stencil", words.data_ptr(), out.data_ptr(), scratch.data_ptr(), n_vol, X, Y, Z, 3, M.DILATE, 3, None)
        _lib.call("dycon_morph_fill_holes", words.data_ptr(), n_vol, X, Y, Z, 1, filled.data_ptr(), ws.data_ptr(), ws.numel(), None)
        _lib.call("dycon_morph_unpack", out.data_ptr(), n_vol, X, Y, Z, mask.data_ptr(), None)
        _lib.call("dycon_cc_roots", vol.data_ptr(), 1, n_vol, X, Y, Z, 3, 0, root.data_ptr(), None)
        _lib.call("dycon_cc_keep_min_size", root.data_ptr(), n_vol, X, Y, Z, 3, kept.data_ptr(), ws2.data_ptr(), ws2.numel(), None)
        g.check()
    np.testing.assert_array_equal(mask.cpu().numpy(), np.stack([MR.dilation(v, 3, 3) for v in batch]))
    np.testing.assert_array_equal(kept.cpu().numpy(), np.stack([MR.min_size(v, 3, 3) for v in batch]))
    tail = (1 << (Z - 128)) - 1
    for w in (words, out, filled):                              # the unused bits of every row's last word are 0
        assert not (w[..., W - 1] & ~tail).any()


# ------------------------------------------------------------------------------------------------------------------- evaluators
class _LogitNet(torch.nn.Module):
    """the image holds the logit of class 1 (tests/test_components_gpu.py)"""

    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return None, torch.cat([-x, x], 1)


def _ball(shape, centre, radius):
    x, y, z = np.indices(shape)
    return (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2


VOLUME, WINDOW = (32, 32, 24), (16, 16, 16)
KW = dict(patch_size=WINDOW, stride_xy=8, stride_z=8)


def _binary_case():
    """a ball with a cavity, three specks and a small second blob; the ground truth is the ball and the blob"""
    gt = _ball(VOLUME, (14, 15, 11), 8) | _ball(VOLUME, (27, 27, 19), 2)
    pred = gt.copy()
    pred[13:16, 14:17, 10:13] = False                            # a cavity: FillHoles
    for p in ((2, 3, 4), (29, 4, 20), (5, 28, 2)):               # specks: Opening, MinSize
        pred[p] = True
    image = pred.astype(np.float32) * 4.0 - 2.0
    return image, pred.astype(np.uint8), gt.astype(np.uint8)


def test_test_all_case_with_postprocess():
    image, pred, gt = _binary_case()
    cases = [(image, gt), (image[::-1].copy(), gt[::-1].copy())]
    net = _LogitNet().to(DEV)
    pp = M.PostProcess(M.Opening(), M.FillHoles())
    ref_steps = [("opening", (1, 1)), ("fill_holes", (1,))]
    cleaned = MR.chain(pred, ref_steps)
    assert cleaned.any() and not np.array_equal(cleaned, pred) and not np.array_equal(cleaned, gt)
    for device_surface, blend in ((False, None), (True, None), (True, Blend("constant")), (False, Blend("constant"))):
        kw = dict(KW, device_surface=device_surface, blend=blend)
        plain = SE.test_all_case(net, cases, 2, **kw)
        np.testing.assert_array_equal(SE.test_all_case(net, cases, 2, postprocess=None, **kw), plain)
        got = SE.test_all_case(net, cases, 2, postprocess=pp, **kw)
        want = np.mean([SE.calculate_metric_percase(MR.chain(p, ref_steps), g, device_surface=device_surface)
                        for p, g in ((pred, gt), (pred[::-1].copy(), gt[::-1].copy()))], axis=0)
        np.testing.assert_array_equal(got[:2], want[:2])         # Dice, Jaccard: integer counts
        np.testing.assert_allclose(got[2:], want[2:], rtol=RTOL, atol=0)
        assert got[0] != plain[0]
        with_nms = SE.test_all_case(net, cases, 2, nms=1, postprocess=pp, **kw)
        want_nms = SE.calculate_metric_percase(CR.largest(cleaned)[0], gt, device_surface=device_surface)
        np.testing.assert_allclose(with_nms, want_nms, rtol=RTOL, atol=0)       # postprocess comes before nms


def test_test_all_case_classes_with_postprocess():
    shape = VOLUME
    gt = np.zeros(shape, np.int64)
    for c, centre in ((1, (8, 8, 8)), (2, (22, 10, 14)), (3, (12, 24, 12))):
        gt[_ball(shape, centre, 5)] = c
    image = gt.copy()
    image[8, 8, 8] = 0                                           # a hole in class 1
    image[28, 28, 20] = 1                                        # specks of classes 1 and 3
    image[2, 28, 3] = 3
    image[22, 10, 13:16] = 3                                     # class 3 inside class 2: opened away, the hole filled by class 2

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.anchor = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):                                      # the image holds the label: one-hot logits
            return None, torch.cat([4.0 * (x == c).float() for c in range(4)], 1)

    net = Net().to(DEV)
    cases = [(image.astype(np.float32), gt)]
    pp = M.PostProcess(M.Opening(), M.FillHoles())
    cleaned = MR.per_class(image, 4, lambda m: MR.chain(m, [("opening", (1, 1)), ("fill_holes", (1,))]))
    assert not np.array_equal(cleaned, image) and cleaned[22, 10, 14] == 2 and cleaned[28, 28, 20] == 0
    for device_surface in (False, True):
        kw = dict(KW, device_surface=device_surface)
        plain = EC.test_all_case_classes(net, cases, 4, **kw)
        np.testing.assert_array_equal(EC.test_all_case_classes(net, cases, 4, postprocess=None, **kw), plain)
        got = EC.test_all_case_classes(net, cases, 4, postprocess=pp, **kw)
        np.testing.assert_array_equal(got, EC.calculate_metric_perclass(cleaned, gt, 4, device_surface=device_surface))
        assert not np.array_equal(got, plain)


def test_evaluate_isles22_with_min_size():
    image, pred, gt = _binary_case()
    net = _LogitNet().to(DEV)
    cases = [(image, gt)]
    kw = dict(patch_size=WINDOW, stride_xy=8, stride_z=8)
    plain = IE.evaluate_isles22(net, cases, **kw)
    same = IE.evaluate_isles22(net, cases, postprocess=None, **kw)
    for name in plain["per_case"]:
        np.testing.assert_array_equal(same["per_case"][name], plain["per_case"][name])
    k = 40
    cleaned = MR.min_size(pred, k, 3)
    n_gt, n_pred, n_clean = CR.label(gt, 3)[1], CR.label(pred, 3)[1], CR.label(cleaned, 3)[1]
    assert (n_gt, n_pred, n_clean) == (2, 5, 1)                  # the specks and the small blob go
    got = IE.evaluate_isles22(net, cases, postprocess=M.PostProcess(M.MinSize(k)), **kw)
    assert plain["per_case"]["lesion_count_diff"].tolist() == [abs(n_pred - n_gt)]
    assert got["per_case"]["lesion_count_diff"].tolist() == [abs(n_clean - n_gt)]
    assert got["per_case"]["abs_volume_diff"].tolist() == [abs(int(cleaned.sum()) - int(gt.sum()))]
    want = IE.isles_case_metrics(cleaned, gt, device_surface=True)
    want.update((name, float(v)) for name, v in LE.lesion_metrics(cleaned, gt).items() if name in IE.LESION_FIELDS)
    for name, v in got["per_case"].items():
        assert v.tolist() == [want[name]], name


def test_refusals():
    ok = torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device=DEV)
    for bad in (torch.zeros((1, 1, 4, 4, 4), dtype=torch.uint8, device=DEV), torch.zeros((1, 4, 4, 513), dtype=torch.uint8, device=DEV)):
        for f in (M.binary_erosion, M.binary_fill_holes, lambda v: M.remove_small_components(v, 3), M.PostProcess(M.Largest())):
            with pytest.raises(ValueError):
                f(bad)
    with pytest.raises(ValueError):
        M.PostProcess().per_class(ok.float(), 3)                 # a label map holds integers
    with pytest.raises(_lib.DyconLibraryError, match="morph_stencil"):
        _lib.call("dycon_morph_stencil", ok.data_ptr(), ok.data_ptr(), None, 1, 4, 5, 6, 1, 0, 1, None)
