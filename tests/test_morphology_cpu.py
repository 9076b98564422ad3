"""Mask post-processing without a GPU: the C ABI surface of csrc/morphology.hip, its argument checks (all before any launch), the
validation of the steps, the evaluators' `postprocess` keyword, and the restatements of tests/morphology_ref.py held to scipy."""
import ctypes
import dataclasses
import inspect
import os
import re

import numpy as np
import pytest

import morphology_ref as MR
from conftest import ROOT
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import eval_classes, isles_eval, morphology as M, surface_eval
from dycon_paper_replication_amd import utils

ABI = {"dycon_morph_fill_workspace": 4, "dycon_cc_min_size_workspace": 4, "dycon_morph_pack": 10, "dycon_morph_unpack": 7,
       "dycon_morph_stencil": 11, "dycon_morph_fill_holes": 10, "dycon_cc_keep_min_size": 10, "dycon_morph_merge_class": 7}


def test_c_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    csrc = os.path.join(ROOT, "dycon_paper_replication_amd", "csrc")
    assert re.search(r"global:\s*dycon_\*;", open(os.path.join(csrc, "exports.map")).read())
    assert re.search(r"^SRCS\s*=.*\bmorphology\.hip\b", open(os.path.join(csrc, "Makefile")).read(), re.M)
    lib = _lib.load()
    for name, nargs in ABI.items():
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs and getattr(lib, name)
    assert re.search(r"#define\s+DYCON_MORPH_ERODE\s+0\b", hdr) and re.search(r"#define\s+DYCON_MORPH_DILATE\s+1\b", hdr)
    assert (M.ERODE, M.DILATE) == (0, 1)
    assert utils.morphology is M


def test_workspace_queries():
    lib = _lib.load()
    assert lib.dycon_morph_fill_workspace(2, 5, 7, 130) >= 2 * 5 * 7 * 130 * 5
    assert lib.dycon_cc_min_size_workspace(2, 5, 7, 130) >= 2 * 5 * 7 * 130 * 4
    for bad in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 513, 4), (1, 4, 4, 513), (65536, 1, 1, 1), (17, 512, 512, 512)):
        assert lib.dycon_morph_fill_workspace(*bad) == 0 and lib.dycon_cc_min_size_workspace(*bad) == 0


def test_library_rejects_bad_arguments_before_any_launch():
    """every pointer here is host memory: a launch would fault, a -22 shows that none was made"""
    lib = _lib.load()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    q, r = p + 1024, p + 2048
    shapes = (dict(X=0), dict(Y=0), dict(Z=0), dict(X=513), dict(Y=513), dict(Z=513), dict(n_vol=0), dict(n_vol=65536))

    def pack(vol=p, vol_bytes=1, n_vol=1, X=2, Y=2, Z=2, by_value=0, value=0, packed=q):
        return lib.dycon_morph_pack(vol, vol_bytes, n_vol, X, Y, Z, by_value, value, packed, None)

    def unpack(packed=p, n_vol=1, X=2, Y=2, Z=2, out=q):
        return lib.dycon_morph_unpack(packed, n_vol, X, Y, Z, out, None)

    def stencil(in_=p, out=q, scratch=r, n_vol=1, X=2, Y=2, Z=2, connectivity=1, op=0, iterations=1):
        return lib.dycon_morph_stencil(in_, out, scratch, n_vol, X, Y, Z, connectivity, op, iterations, None)

    def fill(mask=p, n_vol=1, X=2, Y=2, Z=2, connectivity=1, out=q, ws=r, ws_bytes=2048):
        return lib.dycon_morph_fill_holes(mask, n_vol, X, Y, Z, connectivity, out, ws, ws_bytes, None)

    def keep(root=p, n_vol=1, X=2, Y=2, Z=2, min_voxels=1, out=q, ws=r, ws_bytes=2048):
        return lib.dycon_cc_keep_min_size(root, n_vol, X, Y, Z, min_voxels, out, ws, ws_bytes, None)

    def merge(label_map=p, vol_bytes=1, mask=q, cls=1, n=8, out=r):
        return lib.dycon_morph_merge_class(label_map, vol_bytes, mask, cls, n, out, None)

    table = (
        (pack, b"morph_pack", (dict(vol=None), dict(packed=None), dict(vol_bytes=4), dict(vol_bytes=0)) + shapes),
        (unpack, b"morph_unpack", (dict(packed=None), dict(out=None)) + shapes),
        (stencil, b"morph_stencil", (dict(in_=None), dict(out=None), dict(connectivity=0), dict(connectivity=4), dict(iterations=0),
                                     dict(iterations=65), dict(iterations=-1), dict(op=2), dict(op=-1), dict(scratch=None, iterations=2),
                                     dict(out=p), dict(scratch=p, iterations=2), dict(scratch=q, iterations=2),
                                     dict(out=p + 8, X=2, Y=2, Z=2)) + shapes),
        (fill, b"morph_fill_holes", (dict(mask=None), dict(out=None), dict(ws=None), dict(connectivity=0), dict(connectivity=4),
                                     dict(ws_bytes=0), dict(ws_bytes=511)) + shapes),
        (keep, b"cc_keep_min_size", (dict(root=None), dict(out=None), dict(ws=None), dict(min_voxels=0), dict(min_voxels=-3),
                                     dict(ws_bytes=0), dict(ws_bytes=255)) + shapes),
        (merge, b"morph_merge_class", (dict(label_map=None), dict(mask=None), dict(out=None), dict(vol_bytes=2), dict(cls=0),
                                       dict(cls=256), dict(n=0), dict(n=1 << 31))),
    )
    for fn, name, bads in table:
        for bad in bads:
            assert fn(**bad) == -22, (name, bad)
            assert name in lib.dycon_last_error(), (name, bad, lib.dycon_last_error())


def test_steps_are_frozen_and_validated():
    assert (M.Erosion().connectivity, M.Erosion().iterations) == (1, 1)
    assert M.Opening(1, 2) == M.Opening(connectivity=1, iterations=2) and M.Opening(1, 2) != M.Closing(1, 2)
    assert M.FillHoles().connectivity == 1 and M.MinSize(30).connectivity == 3 and M.Largest().connectivity == 3
    assert M.MinSize(30).min_voxels == 30
    for step in (M.Erosion(), M.Dilation(), M.Opening(), M.Closing(), M.FillHoles(), M.MinSize(2), M.Largest()):
        assert dataclasses.is_dataclass(step)
        with pytest.raises(dataclasses.FrozenInstanceError):
            step.connectivity = 2
    for cls in (M.Erosion, M.Dilation, M.Opening, M.Closing):
        for bad in (dict(connectivity=0), dict(connectivity=4), dict(connectivity=1.5), dict(iterations=0), dict(iterations=-1),
                    dict(iterations=65), dict(iterations=1.5), dict(iterations=True), dict(iterations=None)):
            with pytest.raises(ValueError):
                cls(**bad)
    for bad in (0, 4, "full"):
        with pytest.raises(ValueError):
            M.FillHoles(bad)
        with pytest.raises(ValueError):
            M.Largest(bad)
    for bad in (0, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            M.MinSize(bad)
    with pytest.raises(ValueError):
        M.MinSize(5, connectivity=0)
    with pytest.raises(TypeError):
        M.MinSize()
    pp = M.PostProcess(M.Opening(1, 2), M.FillHoles(), M.MinSize(30), M.Largest())
    assert pp.steps == (M.Opening(1, 2), M.FillHoles(), M.MinSize(30), M.Largest())
    assert pp == M.PostProcess(*pp.steps) and M.PostProcess().steps == ()
    for bad in ("opening", M.Opening, None, 3):
        with pytest.raises(TypeError):
            M.PostProcess(M.Erosion(), bad)
    with pytest.raises(ValueError):
        pp.per_class(np.zeros((2, 2, 2), np.uint8), 1)


def test_public_signatures():
    for fn in (M.binary_erosion, M.binary_dilation, M.binary_opening, M.binary_closing):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["mask", "connectivity", "iterations"]
        assert (sig.parameters["connectivity"].default, sig.parameters["iterations"].default) == (1, 1)
    sig = inspect.signature(M.binary_fill_holes)
    assert list(sig.parameters) == ["mask", "connectivity"] and sig.parameters["connectivity"].default == 1
    sig = inspect.signature(M.remove_small_components)
    assert list(sig.parameters) == ["mask", "min_voxels", "connectivity"] and sig.parameters["connectivity"].default == 3
    assert sig.parameters["min_voxels"].default is inspect.Parameter.empty


def test_evaluators_take_postprocess_keyword_only_before_blend():
    for fn in (surface_eval.test_all_case, eval_classes.test_all_case_classes, isles_eval.evaluate_isles22):
        params = inspect.signature(fn).parameters
        assert list(params)[-2:] == ["postprocess", "blend"], fn.__qualname__
        for name in ("postprocess", "blend"):
            assert params[name].default is None and params[name].kind is inspect.Parameter.KEYWORD_ONLY, (fn.__qualname__, name)
    for fn, args in ((surface_eval.test_all_case, (None, [], 2)), (eval_classes.test_all_case_classes, (None, [], 2)),
                     (isles_eval.evaluate_isles22, (None, []))):
        with pytest.raises(TypeError, match="PostProcess"):          # refused before a case is read or a model touched
            fn(*args, postprocess=M.Opening())


def test_inputs_are_refused_before_any_gpu_work():
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((1, 1, 4, 4, 4), np.uint8), np.zeros((4, 4, 513), np.uint8)):
        with pytest.raises(ValueError):
            M.binary_erosion(bad)
    import torch
    with pytest.raises(ValueError, match="CUDA"):
        M.binary_fill_holes(torch.zeros((4, 4, 4), dtype=torch.uint8))
    with pytest.raises(ValueError):
        M.binary_dilation(np.zeros((4, 4, 4), np.uint8), connectivity=4)
    with pytest.raises(ValueError):
        M.binary_dilation(np.zeros((4, 4, 4), np.uint8), iterations=0)
    with pytest.raises(ValueError):
        M.remove_small_components(np.zeros((4, 4, 4), np.uint8), 0)


# ------------------------------------------------------------------------------------------------------------------- restatements
CPU_SHAPES = MR.SHAPES + [(3, 1, 65), (1, 1, 1)]


def _masks(shape):
    out = [m for m in MR.random_batch(shape)] + [np.ones(shape, np.uint8), np.zeros(shape, np.uint8), MR.corners(shape)]
    if min(shape) >= 5:
        out += list(MR.hole_batch(shape))
    return out


@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_shifted_and_or_is_scipy(shape):
    """erosion = AND, dilation = OR of the mask shifted by every offset of the structure with zero fill: what one thread per word
    computes with shifts, carries and neighbouring rows"""
    for m in _masks(shape):
        for c in (1, 2, 3):
            for n in (1, 2, 3):
                np.testing.assert_array_equal(MR.erosion_shifted(m, c, n), MR.erosion(m, c, n))
                np.testing.assert_array_equal(MR.dilation_shifted(m, c, n), MR.dilation(m, c, n))
                np.testing.assert_array_equal(MR.dilation_shifted(MR.erosion_shifted(m, c, n), c, n), MR.opening(m, c, n))
                np.testing.assert_array_equal(MR.erosion_shifted(MR.dilation_shifted(m, c, n), c, n), MR.closing(m, c, n))


@pytest.mark.parametrize("shape", CPU_SHAPES)
def test_unmarked_background_components_are_scipy_fill_holes(shape):
    for m in _masks(shape):
        for c in (1, 2, 3):
            np.testing.assert_array_equal(MR.fill_holes_components(m, c), MR.fill_holes(m, c))


def test_named_hole_cases_are_what_their_names_say():
    for shape in MR.SHAPES:
        hollow, tunnel, diagonal, straddle, face = MR.hole_batch(shape)
        solid = MR.solid_box(shape)
        for c in (1, 2, 3):
            np.testing.assert_array_equal(MR.fill_holes(hollow, c), solid)
            np.testing.assert_array_equal(MR.fill_holes(tunnel, c), tunnel)
            np.testing.assert_array_equal(MR.fill_holes(straddle, c), MR.solid_box(shape, 60, 68))
        filled = MR.fill_holes(diagonal, 1)
        assert filled.sum() == solid.sum() - 1 and (filled >= diagonal).all()
        np.testing.assert_array_equal(MR.fill_holes(diagonal, 2), diagonal)
        np.testing.assert_array_equal(MR.fill_holes(diagonal, 3), diagonal)
        assert straddle[:, :, 63].any() and not straddle[2, 2, 63] and not straddle[2, 2, 64]
        closed = MR.closing(face, 1, 1)
        assert closed[1, 1, shape[2] - 5] and not face[1, 1, shape[2] - 5]          # the gap is bridged
        assert not closed[0].any() and not closed[:, 0].any() and not closed[:, :, -1].any() and face[0].any()     # the faces are eaten
        blobs = MR.two_blobs(shape, 9)
        assert sorted(np.bincount(MR.CR.label(blobs, 3)[0].ravel())[1:]) == [8, 9]
        assert MR.min_size(blobs, 9).sum() == 9 and MR.min_size(blobs, 8).sum() == 17 and MR.min_size(blobs, 10).sum() == 0


def test_inputs_are_not_vacuous():
    """the figures the GPU tests rely on: holes to fill and survivors of two 26-neighbour erosions at densities 0.7 and 0.93"""
    for shape in MR.SHAPES[:2]:
        batch = MR.random_batch(shape)
        for m, d in zip(batch, MR.DENSITIES):
            assert d - 0.005 < m.mean() < d + 0.02
        for m in batch[1:]:
            filled = int(MR.fill_holes(m).sum() - m.sum())
            left = int(MR.erosion(m, 3, 2).sum())
            print(f"{shape}: density {m.mean():.3f}, fill_holes fills {filled}, 2x 26-neighbour erosion leaves {left}")
            assert filled > 0 and 0 < left < m.sum()


def test_per_class_rule():
    lm = np.zeros((1, 1, 8), np.uint8)
    lm[0, 0] = [1, 1, 0, 2, 2, 0, 3, 0]
    grow = lambda m: MR.dilation(m, 1, 1)                     # noqa: E731
    #            own  own  1<2  own own 2<3 own  3
    assert MR.per_class(lm, 4, grow)[0, 0].tolist() == [1, 1, 1, 2, 2, 2, 3, 3]
    assert MR.per_class(lm, 4, lambda m: m)[0, 0].tolist() == lm[0, 0].tolist()
    assert MR.per_class(lm, 4, lambda m: MR.erosion(m, 1, 1))[0, 0].tolist() == [0] * 8
    assert MR.per_class(lm, 3, lambda m: m)[0, 0].tolist() == [1, 1, 0, 2, 2, 0, 0, 0]          # a value outside 1..C-1 is dropped
