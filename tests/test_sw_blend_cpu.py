"""`sliding_window.Blend` without a GPU: the option's validation, the importance tables, the entry list, the C ABI surface, and the fp64
restatement the GPU tests compare against (tests/sw_blend_ref.py) held to the CPU oracle where the two must agree.

Case B: (24, 40, 12), windows (32, 32, 16), stride 8 / 4 -> 2 windows, padded on two axes (tests/test_ensemble_gpu.py)."""
import ctypes
import dataclasses
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import sw_blend_ref as BR
from conftest import ROOT
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd.utils import ensemble_eval, eval_classes, isles_eval, surface_eval, test_3d_patch as T3
from dycon_paper_replication_amd.utils import sliding_window as SW
from dycon_paper_replication_amd.utils.sliding_window import Blend
from oracle import evaluate as OE
from oracle import nets as ON

PATCH = (32, 32, 16)


def test_blend_defaults_and_validation():
    b = Blend()
    assert (b.weighting, b.sigma_scale, b.mirror_axes) == ("gaussian", 0.125, ())
    assert Blend("constant", mirror_axes=[2, 0]).mirror_axes == (0, 2)                  # stored sorted
    assert Blend(mirror_axes=(2, 1, 0)).mirror_axes == (0, 1, 2)
    with pytest.raises(dataclasses.FrozenInstanceError):
        b.weighting = "constant"
    for bad in (dict(weighting="linear"), dict(weighting=None), dict(mirror_axes=(0, 0)), dict(mirror_axes=(3,)), dict(mirror_axes=(-1,)),
                dict(mirror_axes=(0.5,)), dict(mirror_axes=1), dict(sigma_scale=0.0), dict(sigma_scale=-0.125),
                dict(sigma_scale=float("nan")), dict(sigma_scale=float("inf")), dict(sigma_scale="wide")):
        with pytest.raises(ValueError):
            Blend(**bad)


@pytest.mark.parametrize("patch", [(32, 32, 16), (8, 8, 4), (7, 5, 3), (96, 96, 64)])
def test_window_weights_are_the_formula(patch):
    tabs = SW.window_weights(patch, Blend("gaussian", sigma_scale=0.125))
    assert len(tabs) == 3
    for g, p in zip(tabs, patch):
        assert isinstance(g, np.ndarray) and g.dtype == np.float32 and g.shape == (p,)
        want = np.array([np.float32(math.exp(-0.5 * ((i - (p - 1) / 2) / (0.125 * p)) ** 2)) for i in range(p)])
        assert np.array_equal(g, want)
        assert np.array_equal(g, g[::-1])                                                # g[i] == g[p - 1 - i]
        if p % 2:
            assert g[p // 2] == 1.0
        assert (g > 0).all() and g.max() <= 1.0
    assert all(np.array_equal(a, b) for a, b in zip(tabs, BR.tables(patch, "gaussian", 0.125)))
    for g, p in zip(SW.window_weights(patch, Blend("constant")), patch):
        assert g.dtype == np.float32 and np.array_equal(g, np.ones(p, np.float32))


def test_window_weights_refuse_a_corner_below_1e_30():
    tabs = SW.window_weights(PATCH, Blend())
    assert 2.6e-10 < float(tabs[0].min()) * float(tabs[1].min()) * float(tabs[2].min()) < 2.8e-10      # a normal fp32 number
    # the corner's exponent is -0.5 * (2 * (15.5 / 32) ** 2 + (7.5 / 16) ** 2) / sigma_scale ** 2 = -0.3445 / sigma_scale ** 2, and
    # exp(-69.08) = 1e-30: the limit for this window is sigma_scale = 0.0706
    SW.window_weights(PATCH, Blend(sigma_scale=0.072))
    for narrow in (0.069, 0.03):
        with pytest.raises(ValueError, match="1e-30"):
            SW.window_weights(PATCH, Blend(sigma_scale=narrow))
    with pytest.raises(ValueError):
        SW.window_weights((32, 0, 16), Blend())


@pytest.mark.parametrize("axes,masks", [((), [0]), ((1,), [0, 2]), ((0, 2), [0, 1, 4, 5]), ((0, 1, 2), [0, 1, 2, 3, 4, 5, 6, 7])])
def test_window_entries_order_and_masks(axes, masks):
    wins = SW._windows((40, 36, 20), PATCH, 16, 4)
    assert len(wins) == 8
    ent = SW.window_entries(wins, axes)
    assert ent.dtype == np.int32 and ent.shape == (8 * len(masks), 4)
    assert ent.tolist() == [[x, y, z, m] for x, y, z in wins for m in masks]            # windows in order, masks ascending, 0 first
    assert ent.tolist() == [list(e) for e in BR.entries(BR.windows((40, 36, 20), PATCH, 16, 4), axes)]
    assert np.array_equal(SW.window_entries(wins, Blend(mirror_axes=axes[::-1]).mirror_axes), ent)


def _image(shape):
    return np.random.default_rng(sum(shape)).standard_normal(shape).astype(np.float32)


def test_restatement_with_unit_weights_is_the_oracle_evaluator():
    """measured: 9.6e-8 (the oracle accumulates in fp32)"""
    params = ON.make_vnet_params(3, n_classes=2)
    net = lambda t: ON.forward("vnet", t, params, bn_training=False)[1]                 # noqa: E731
    image = _image((24, 40, 12))
    lab_ref, score_ref = OE.test_single_case(net, image, 8, 4, PATCH, num_classes=1)
    lab, prob = BR.single_case(net, image, 8, 4, PATCH, weighting="constant")
    assert prob.dtype == np.float64 and prob.shape == image.shape == lab.shape
    err = np.abs(prob - score_ref[0]).max()
    print(f"restatement, unit weights, against oracle.evaluate.test_single_case: {err:.3e}")
    assert err <= 1e-6
    decided = np.abs(prob - 0.5) > 1e-6
    assert np.array_equal(lab[decided], lab_ref[decided])
    # a list of nets is the mean of their logits: a net with itself is that net
    _, twice = BR.single_case([net, net], image, 8, 4, PATCH, weighting="constant")
    assert np.abs(twice - prob).max() <= 1e-12


def test_restatement_mirroring_a_pointwise_net_changes_nothing():
    """a pointwise function of the input is flip-equivariant: every orientation of a window gives the same un-flipped softmax, and
    a weighted mean of equal values is that value"""
    net = lambda t: torch.cat([torch.sin(3 * t), t * t - 0.5, 0.25 * t], 1)             # noqa: E731
    image = _image((13, 20, 9))
    for all_classes in (False, True):
        for weighting in ("constant", "gaussian"):
            kw = dict(weighting=weighting, all_classes=all_classes)
            lab0, p0 = BR.single_case(net, image, 4, 2, (8, 8, 6), **kw)
            lab7, p7 = BR.single_case(net, image, 4, 2, (8, 8, 6), mirror_axes=(0, 1, 2), **kw)
            assert p0.shape == ((3,) if all_classes else ()) + image.shape
            assert np.abs(p7 - p0).max() <= 1e-12
            assert 0 < (lab0 != 0).mean() < 1
    # and it is no accident of the restatement: a net that is NOT equivariant moves under mirroring
    shift = lambda t: torch.cat([t, torch.roll(t, 1, 2)], 1)                            # noqa: E731
    assert np.abs(BR.single_case(shift, image, 4, 2, (8, 8, 6), mirror_axes=(0,))[1] - BR.single_case(shift, image, 4, 2, (8, 8, 6))[1]).max() > 1e-3


def test_c_abi_surface():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    csrc = os.path.join(ROOT, "dycon_paper_replication_amd", "csrc")
    assert re.search(r"global:\s*dycon_\*;", open(os.path.join(csrc, "exports.map")).read())
    lib = _lib.load()
    for name, nargs in (("dycon_sw_gather_mirror", 13), ("dycon_sw_accumulate_weighted", 23)):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert len(_lib.SIGNATURES[name][1]) == nargs and getattr(lib, name)
    assert _lib.SIGNATURES["dycon_sw_gather_mirror"] == _lib.SIGNATURES["dycon_sw_gather"]


def test_library_rejects_bad_arguments_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    int3 = ctypes.c_int * 3

    def gather(vol=p, shape=(9, 7, 5), ent=p, n_entries=8, first=0, n=4, patch=(8, 8, 6), out=p):
        return lib.dycon_sw_gather_mirror(vol, *shape, ent, n_entries, first, n, *patch, out, None)

    for bad in (dict(vol=None), dict(ent=None), dict(out=None), dict(shape=(9, 0, 5)), dict(patch=(8, 8, 0)), dict(n=0), dict(n=65, n_entries=100),
                dict(first=-1), dict(first=5), dict(first=8, n=1), dict(n_entries=0), dict(n=9)):
        assert gather(**bad) == -22, bad
        assert b"sw_gather_mirror" in lib.dycon_last_error()

    def acc(ptrs=(p, None, None, None), M=1, C=2, all_classes=0, nb=2, patch=(8, 8, 4), ent=p, g=(p, p, p), score=p, cnt=p, vol=(12, 8, 6),
            lo=None, hi=None):
        return lib.dycon_sw_accumulate_weighted(*ptrs, M, C, all_classes, nb, *patch, ent, *g, score, cnt, *vol, lo, hi, None)

    for bad in (dict(M=0), dict(M=5), dict(M=2), dict(ptrs=(None, p, None, None)), dict(C=1), dict(C=9), dict(all_classes=2), dict(all_classes=-1),
                dict(all_classes=1, M=2, ptrs=(p, p, None, None)), dict(nb=0), dict(nb=65), dict(ent=None), dict(g=(p, None, p)),
                dict(g=(None, p, p)), dict(g=(p, p, None)), dict(score=None), dict(cnt=None), dict(vol=(7, 8, 6)), dict(patch=(8, 8, 0)),
                dict(lo=int3(0, 0, 0)), dict(hi=int3(8, 8, 4)), dict(lo=int3(0, 0, 0), hi=int3(13, 8, 6)), dict(lo=int3(-1, 0, 0), hi=int3(8, 8, 4)),
                dict(lo=int3(4, 0, 0), hi=int3(4, 8, 4))):
        assert acc(**bad) == -22, bad
        assert b"sw_accumulate_weighted" in lib.dycon_last_error()


def test_every_evaluator_takes_blend_as_a_keyword_only_none():
    for fn in (SW._sliding_window, SW.single_case_device, SW.test_single_case, eval_classes.single_case_classes_device,
               eval_classes.test_single_case_classes, eval_classes.test_all_case_classes, ensemble_eval.single_case_ensemble_device,
               ensemble_eval.single_case_plus_device, surface_eval.test_all_case, isles_eval.evaluate_isles22):
        params = inspect.signature(fn).parameters
        assert list(params)[-1] == "blend" and params["blend"].default is None, fn.__qualname__
        if fn is not SW._sliding_window:
            assert params["blend"].kind is inspect.Parameter.KEYWORD_ONLY, fn.__qualname__
    assert T3.test_single_case is SW.test_single_case


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))

    def forward(self, x):
        return None, torch.cat([x, -x], 1), None


def test_guards_raise_before_any_gpu_work():
    image, args = np.zeros((8, 8, 8), np.float32), (4, 4, (8, 8, 8))
    with pytest.raises(ValueError, match="whole-volume"):           # nothing to blend without windows; raised before a case is read
        isles_eval.evaluate_isles22(_Stub(), iter([]), blend=Blend())
    with pytest.raises(TypeError, match="Blend"):
        SW._sliding_window([_Stub()], [lambda x: x], image, *args, 4, torch.device("cpu"), blend="gaussian")
    with pytest.raises(RuntimeError, match="MI355X only"):          # well-formed, but the model is on the CPU
        SW.single_case_device(_Stub(), image, *args, blend=Blend())
