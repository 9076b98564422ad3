"""Signed distance maps on the MI355X (csrc/sdf.hip, utils/util.py) against the scipy restatement of the reference's compute_sdf
(tests/sdf_ref.py) and against the reference's recorded outputs (tests/golden/sdf.npz).

Every comparison is bit equality, NaNs at the same places and no zero with a sign bit: the squared distances are exact integers,
fp64 sqrt and division are correctly rounded on both sides, and with a foreground and a background voxel in the sample the
reference's expression is -posdis / max(posdis) inside and +negdis / max(negdis) outside (tests/test_util_cpu.py checks that form in
numpy).  fp32 outputs are the fp64 values rounded once.  The shapes are the smallest at which each part of the kernels can go wrong."""
import functools

import numpy as np
import pytest
import torch

import sdf_ref as R
import surface_ref as SR
from conftest import load_golden

from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import util

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(got, ref):
    """bit equality up to the payload of a NaN; every zero is +0.0"""
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, got.shape, ref.dtype, ref.shape)
    if not np.array_equal(got, ref, equal_nan=True):
        bad = np.argwhere(~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        raise AssertionError(f"{len(bad)} of {got.size} differ, first at {bad[0].tolist()}: {got[tuple(bad[0])]!r} != {ref[tuple(bad[0])]!r}")
    assert not np.signbit(got[got == 0]).any()
    return True


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def single(shape, at, fill=False):
    m = np.full(shape, fill, bool)
    m[at] = not fill
    return m


@functools.lru_cache(maxsize=None)
def line_batch(shape):
    """blobs, and masks whose only foreground (or only background) voxel sits at an end of a z row or in a corner of the volume"""
    X, Y, Z = shape
    masks = [R.blobs(shape, 11 + Z, 0.3), R.blobs(shape, 12 + X, 0.1), single(shape, (X // 2, Y // 2, 0)),
             single(shape, (X // 2, Y // 2, Z - 1)), single(shape, (X // 2, Y // 2, 0), True), single(shape, (0, Y - 1, Z - 1)),
             single(shape, (X - 1, 0, Z // 2), True)]
    masks = np.stack(masks)
    return masks, np.stack([R.signed_distance(m) for m in masks])


# ------------------------------------------------------------------------------------------------- the reference's recorded outputs
@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_golden_masks(name):
    g = load_golden("sdf")
    img_gt, out_shape, want = g[f"sdf.{name}.img_gt"], tuple(int(n) for n in g[f"sdf.{name}.out_shape"]), g[f"sdf.{name}.sdf"]
    got = util.compute_sdf(img_gt, out_shape)
    assert isinstance(got, np.ndarray)
    same(got, want)
    on_dev = util.compute_sdf_device(dev(img_gt), out_shape, dtype=torch.float64)
    assert on_dev.is_cuda and on_dev.shape == out_shape
    same(on_dev, want)
    same(util.compute_sdf_device(dev(img_gt), out_shape), want.astype(np.float32))
    same(util.compute_sdf(dev(img_gt), out_shape), want)                      # labels already on the device
    same(util.compute_sdf(torch.from_numpy(img_gt), out_shape), want)         # a host tensor


# ------------------------------------------------------------------------------------------------- the kernels' paths
@pytest.mark.parametrize("shape", [(5, 6, 9), (13, 10, 70), (6, 5, 130)], ids=str)
def test_row_pass(shape):
    """Z below a wave | a second, ragged ballot word | a third word and a nearest seed two words away"""
    masks, ref = line_batch(shape)
    same(util.compute_sdf_device(dev(masks), dtype=torch.float64), ref)


@pytest.mark.parametrize("shape", [(13, 10, 70), (33, 21, 8), (130, 3, 5), (3, 260, 5)], ids=str)
def test_axis_passes(shape):
    """line lengths that are no multiple of the four waves | the 256- and the 512-line instantiations"""
    masks, ref = line_batch(shape)
    same(util.compute_sdf_device(dev(masks), dtype=torch.float64), ref)
    same(util.compute_sdf_device(dev(masks)), ref.astype(np.float32))


def test_an_axis_above_512_is_refused():
    for shape in ((513, 2, 2), (2, 513, 2), (2, 2, 513)):
        z = torch.zeros((1,) + shape, dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match="1..512"):
            util.compute_sdf_device(z)
        with pytest.raises(ValueError, match="1..512"):
            util.compute_sdf(z, z.shape)
    with pytest.raises(ValueError, match="CUDA"):
        util.compute_sdf_device(torch.zeros((1, 2, 2, 2), dtype=torch.uint8))


def test_degenerate_samples_in_one_batch():
    shape = (9, 7, 11)
    masks = np.stack([np.zeros(shape, bool), np.ones(shape, bool), single(shape, (4, 2, 9)), single(shape, (1, 5, 3), True)])
    for dtype in (torch.float64, torch.float32):
        got = util.compute_sdf_device(dev(masks), dtype=dtype).cpu().numpy()
        np_dtype = got.dtype.type
        assert not got[0].any() and not np.signbit(got[0]).any()                  # no foreground: +0.0
        assert np.isnan(got[1]).all()                                             # no background: the reference's 0 / 0
        assert got[2][4, 2, 9] == 0 and got[2].max() == 1 and got[2].min() == 0   # its own boundary; the outside by its own maximum
        assert got[3][1, 5, 3] == 1 and got[3].min() == -1
        for s in range(4):
            same(got[s], R.signed_distance(masks[s]).astype(np_dtype))
    raw = util.compute_sdf_device(dev(masks), dtype=torch.float64, normalize=False).cpu().numpy()
    assert len({raw[2].max(), -raw[3].min(), 1.0}) == 3                           # the maxima differ: nothing leaks across samples
    for s in range(4):
        same(raw[s], R.signed_distance(masks[s], normalize=False))


def test_boundary_rule():
    shape = (6, 7, 9)
    box, plate = np.zeros(shape, bool), np.zeros(shape, bool)
    box[:3, :4, 4:] = True                                   # on the faces x = 0, y = 0 and z = Z - 1
    plate[:, 3, :] = True                                    # one voxel thick
    got = util.compute_sdf_device(dev(np.stack([box, plate])), dtype=torch.float64).cpu().numpy()
    same(got[0], R.signed_distance(box))
    same(got[1], R.signed_distance(plate))
    # face voxels without a background neighbour inside the volume are not boundary: they carry their distance.  The corner is the
    # deepest voxel of the box: 3 from x = 3, 4 from y = 4 and 5 from z = 3
    assert got[0][0, 0, 8] == -1.0 and got[0][0, 0, 7] < 0 and got[0][1, 0, 8] < 0
    assert (SR.border6(box) & (got[0] != 0) & box).sum() > 0                   # voxels csrc/surface.hip calls border, not zeroed here
    assert got[0][2, 0, 8] == 0 and got[0][0, 3, 8] == 0 and got[0][0, 0, 4] == 0
    assert not got[1][plate].any() and not np.signbit(got[1][plate]).any()     # max posdis = 1 and all of it boundary: +0.0
    raw = util.compute_sdf_device(dev(box[None]), dtype=torch.float64, normalize=False)[0].cpu().numpy()
    assert raw[0, 0, 8] == -3.0
    same(raw, R.signed_distance(box, normalize=False))


# ------------------------------------------------------------------------------------------------- inputs and extensions
def test_label_dtypes_strides_and_values_above_one():
    shape = (13, 10, 70)
    lab = (R.blobs(shape, 5, 0.3).astype(np.int64) + R.blobs(shape, 6, 0.3) * 4)[None].repeat(2, 0)      # values 0, 1, 4, 5
    lab[1] = lab[1, ::-1, :, ::-1]
    ref = np.stack([R.signed_distance(m != 0) for m in lab])
    assert ((lab > 1) & (ref <= 0)).any()
    for arr in (lab.astype(np.uint8), lab != 0, lab, lab.astype(np.float64), lab.astype(np.int32), lab.astype(np.float32)):
        same(util.compute_sdf_device(dev(arr), dtype=torch.float64), ref)
        same(util.compute_sdf(arr, arr.shape), ref)
    t = dev(lab.astype(np.uint8)).transpose(1, 3)                             # (B, z, y, x) view, not contiguous
    assert not t.is_contiguous()
    same(util.compute_sdf_device(t, dtype=torch.float64), np.stack([R.signed_distance(m.transpose(2, 1, 0) != 0) for m in lab]))
    same(util.compute_sdf_device(dev(lab)[:, ::2], dtype=torch.float64), np.stack([R.signed_distance(m[::2] != 0) for m in lab]))


def test_out_shape_broadcast():
    masks, ref = line_batch((13, 10, 70))
    masks, ref = masks[:3], ref[:3]
    for C in (1, 2):
        out_shape = (3, C, 13, 10, 70)
        want = np.broadcast_to(ref[:, None], out_shape)
        same(util.compute_sdf_device(dev(masks), out_shape, dtype=torch.float64), np.ascontiguousarray(want))
        same(util.compute_sdf(masks, out_shape), R.compute_sdf(masks, out_shape))
    same(util.compute_sdf(masks, (2, 13, 10, 70)), ref[:2])                   # the reference reads out_shape[0] samples
    flat = R.blobs((1, 10, 70), 3, 0.3)[None]                                 # a size-1 axis of the volume grows: numpy's broadcast
    same(util.compute_sdf(flat, (1, 4, 10, 70)), R.compute_sdf(flat, (1, 4, 10, 70)))


def test_unnormalised_and_class_maps():
    shape = (13, 10, 70)
    masks, _ = line_batch(shape)
    same(util.compute_sdf_device(dev(masks), dtype=torch.float64, normalize=False),
         np.stack([R.signed_distance(m, normalize=False) for m in masks]))
    lab = np.stack([np.minimum(sum(R.blobs(shape, 40 + 10 * v + j, 0.25).astype(np.int64) for j in range(3)), 3) for v in range(2)])
    lab[1][lab[1] == 3] = 0                                                   # class 3 absent from sample 1
    assert set(np.unique(lab[0])) == {0, 1, 2, 3}
    for normalize in (True, False):
        ref = R.class_maps(lab, 1, 3, normalize)
        for t in (dev(lab), dev(lab.astype(np.uint8))):
            got = util.compute_sdf_device(t, dtype=torch.float64, normalize=normalize, classes=(1, 3))
            assert got.shape == (2, 3) + shape
            same(got, ref)
        assert not ref[1, 2].any()
    same(util.compute_sdf_device(dev(lab), classes=(2, 2)), R.class_maps(lab, 2, 2).astype(np.float32))


def test_samples_go_in_chunks_over_the_workspace_budget(monkeypatch):
    masks, ref = line_batch((5, 6, 9))
    monkeypatch.setattr(util, "WORKSPACE_BUDGET", 2 * int(_lib.load().dycon_sdf_workspace(1, 5, 6, 9)) + 5)
    same(util.compute_sdf_device(dev(masks), dtype=torch.float64), ref)


def test_the_c_abi_refuses_bad_arguments():
    lab = torch.zeros((2, 4, 5, 6), dtype=torch.uint8, device=DEV)
    out = torch.empty((4, 4, 5, 6), dtype=torch.float64, device=DEV)
    ws = torch.empty(int(_lib.load().dycon_sdf_workspace(4, 4, 5, 6)), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def call(label_bytes=1, n_vol=2, cls_lo=0, n_cls=1, shape=(4, 5, 6), n_rep=1, out_bytes=8, ws_bytes=ws.numel()):
        _lib.call("dycon_sdf", lab.data_ptr(), label_bytes, n_vol, cls_lo, n_cls, *shape, 1, n_rep, out_bytes, out.data_ptr(),
                  ws.data_ptr(), ws_bytes, stream)

    call()
    call(cls_lo=1, n_cls=2)
    for bad, match in ((dict(label_bytes=4), "uint8 or int64"), (dict(out_bytes=2), "fp32 or fp64"), (dict(cls_lo=0, n_cls=2), "class range"),
                       (dict(cls_lo=255, n_cls=2), "class range"), (dict(shape=(4, 5, 513)), "every axis"), (dict(n_rep=0), "n_rep"),
                       (dict(shape=(0, 5, 6)), "every axis"), (dict(cls_lo=1, n_cls=2, ws_bytes=ws.numel() - 1), "workspace")):
        with pytest.raises(_lib.DyconLibraryError, match=match):
            call(**bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- determinism, one real geometry
def test_same_bits_on_every_run():
    masks, ref = line_batch((13, 10, 70))
    t = dev(masks)
    first = util.compute_sdf_device(t, dtype=torch.float64)
    assert torch.equal(util.compute_sdf_device(t, dtype=torch.float64).view(torch.int64), first.view(torch.int64))
    side = torch.cuda.Stream()
    junk = torch.empty(32 << 20, dtype=torch.uint8, device=DEV)
    with torch.cuda.stream(side):                            # an unrelated kernel keeps the memory system busy meanwhile
        for k in range(4):
            junk[: (8 << 20) * (1 + k % 3)].add_(1)
    again = util.compute_sdf_device(t, dtype=torch.float64)
    side.synchronize()
    assert torch.equal(again.view(torch.int64), first.view(torch.int64))
    with torch.cuda.stream(side):                            # and on a stream of its own
        there = util.compute_sdf_device(t, dtype=torch.float64)
    side.synchronize()
    assert torch.equal(there.view(torch.int64), first.view(torch.int64))
    same(first, ref)


def test_real_geometry():
    """(2, 112, 112, 80), the Pancreas patch: one case, the scipy side is the cost"""
    shape = (112, 112, 80)
    masks = np.stack([SR._blobs(shape, 21), SR._blobs(shape, 22)])
    got = util.compute_sdf_device(dev(masks), (2, 1) + shape, dtype=torch.float64)
    same(got, np.stack([R.signed_distance(m) for m in masks])[:, None])
