"""Uncertainty maps and calibration of the sliding-window evaluators (csrc/uncertainty.hip, csrc/sw_accumulate.h).

Not in the reference, whose evaluators keep the mean softmax only (code/utils/test_3d_patch.py:334-347).  The sliding window runs a
set of MEMBERS per voxel: every window that covers it x every mirror orientation (``Blend(mirror_axes=...)``) x every model x every
Monte-Carlo dropout pass.  Each member e has its own softmax p_e and the weight w_e the blend gives its window at that voxel.  The
accumulate pass keeps, beside the weighted sum of the softmaxes, the weighted sums of their entropies and of their squares
(``dycon_sw_accumulate_moments``), and one finalize pass (``dycon_sw_finalize_uncertainty``) turns them into

    prob              sum_e w_e p_e / sum_e w_e                         (C, w, h, d)   the mean of the members' SOFTMAXES
    label             argmax_k prob[k], lowest index on ties            uint8
    entropy           H(prob), H(p) = -sum_k p_k ln p_k                 predictive (total) uncertainty, in [0, ln C]
    expected_entropy  sum_e w_e H(p_e) / sum_e w_e                      aleatoric part
    mutual_info       max(0, entropy - expected_entropy)                epistemic part: what the members disagree about
    variance          sum_k max(0, E_e[p_e[k]^2] - prob[k]^2)           in [0, 1 - 1 / C]

Models are members here, and `prob` is the mean of their softmaxes.  That differs from the `_plus` evaluators
(``utils/ensemble_eval.py``), which average the models' LOGITS before one softmax, as the reference does (:460-463): an ensemble scored
there and here gives different probabilities.  With one model and one pass, `label` and `prob` are the bits of
``eval_classes.single_case_classes_device(model, ..., blend=blend)``.

    single_case_uncertainty_device(models, image, stride_xy, stride_z, patch_size)   -> UncertaintyMaps of CUDA tensors
    test_single_case_uncertainty(...)                                                -> the same as numpy arrays
    calibration(prob, label, bins=15, mask=None, uncertainty=None, u_max=None)       -> ECE, MCE, Brier, NLL, accuracy, error AUROC, AURC
    test_all_case_uncertainty(model, cases, num_classes, patch_size, ...)            -> per-case calibration and its mean
"""
from __future__ import annotations

import collections
import ctypes
import math

import numpy as np
import torch

from .. import _lib
from . import case_loop
from .sliding_window import (MAX_MODELS, Blend, _center_pads, _eval_static, _logits_of, _stream, _windows, chunk_box, window_entries,
                             window_weights)

UncertaintyMaps = collections.namedtuple("UncertaintyMaps", "label prob entropy expected_entropy mutual_info variance")
MAX_BINS = 64
_PASS_STRIDE = 1 << 42          # Philox offsets of two forwards differ by at least this much (HipSegNet.forward_mc)


def _check_members(models, mc_passes):
    models = [models] if isinstance(models, torch.nn.Module) else list(models)
    if not 1 <= len(models) <= MAX_MODELS or not all(isinstance(m, torch.nn.Module) for m in models):
        raise ValueError(f"models is one nn.Module or a sequence of 1..{MAX_MODELS}, got {len(models)}")
    if isinstance(mc_passes, bool) or not isinstance(mc_passes, (int, np.integer)) or mc_passes < 1:
        raise ValueError(f"mc_passes must be a positive integer, got {mc_passes!r}")
    if mc_passes > 1:
        for m in models:
            if not (hasattr(m, "forward_mc") and getattr(m, "has_dropout", False)):
                raise ValueError("mc_passes > 1 draws dropout masks inside the model: every model must be a HipSegNet built with "
                                 f"has_dropout=True, got {type(m).__name__}")
    return models, int(mc_passes)


def single_case_uncertainty_device(models, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None, mc_passes=1,
                                   seed=0):
    """The all-class sliding window of one case with its uncertainty maps: `UncertaintyMaps` (label uint8 (w, h, d), prob float32
    (C, w, h, d), entropy, expected_entropy, mutual_info, variance float32 (w, h, d)) as CUDA tensors, without host copies.

    models: one nn.Module or a sequence of 1..4, all with the same class count (2..8).  The members of a voxel are every covering
    window x every mirror orientation of `blend` x every model x every Monte-Carlo pass, each through its own softmax: `prob` is the
    mean of SOFTMAXES, not the softmax of mean logits that `ensemble_eval`'s `_plus` evaluators compute.  Padding, windows, entries,
    chunks and the gather are `sliding_window._sliding_window`'s; blend=None is `Blend("constant")`.

    mc_passes = T > 1 (Monte-Carlo dropout): every chunk goes T times through every model with its dropout masks on and its
    normalisation in inference mode (`HipSegNet.forward_mc`: BatchNorm statistics and `num_batches_tracked` are not touched).  The
    Philox offset is distinct per (chunk, pass, model); the same `seed` gives the same bits.  ValueError for a model that is not a
    HipSegNet with has_dropout=True."""
    models, T = _check_members(models, mc_passes)
    if blend is None:
        blend = Blend("constant")
    elif not isinstance(blend, Blend):
        raise TypeError(f"blend is None or a sliding_window.Blend, got {type(blend).__name__}")
    batch_size = int(batch_size)
    if not 1 <= batch_size <= 64:
        raise ValueError(f"batch_size must be in 1..64, got {batch_size}")
    dev = torch.device(device) if device is not None else next(models[0].parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the model to 'cuda'")
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))).to(dtype=torch.float32)
    w, h, d = img.shape
    p0, p1, p2 = (int(v) for v in patch_size)
    pads = _center_pads((w, h, d), (p0, p1, p2))
    vol = img.to(dev).contiguous()
    ww, hh, dd = (n + lo + hi for n, (lo, hi) in zip((w, h, d), pads))
    wins = _windows((ww, hh, dd), (p0, p1, p2), stride_xy, stride_z)
    tables = [torch.from_numpy(g).to(dev) for g in window_weights((p0, p1, p2), blend)]
    entries = window_entries(wins, blend.mirror_axes)
    origins = torch.from_numpy(entries).to(dev)                     # every entry of the case, uploaded once
    n_rows = len(entries)
    n_chunks = (n_rows + batch_size - 1) // batch_size
    if T > 1 and n_chunks * T * MAX_MODELS * _PASS_STRIDE >= 1 << 64:
        raise ValueError(f"{n_chunks} chunks x {T} passes exceed the Philox offset range")
    f32 = dict(dtype=torch.float32, device=dev)
    cnt, hsum = torch.zeros((ww, hh, dd), **f32), torch.zeros((ww, hh, dd), **f32)
    score = sq = C = None
    int3 = ctypes.c_int * 3
    with _eval_static(models), torch.no_grad():
        for ci, i in enumerate(range(0, n_rows, batch_size)):
            nb = min(batch_size, n_rows - i)
            patches = torch.empty((nb, 1, p0, p1, p2), **f32)
            _lib.call("dycon_sw_gather_mirror", vol.data_ptr(), w, h, d, origins.data_ptr(), n_rows, i, nb, p0, p1, p2, patches.data_ptr(),
                      _stream())
            lo, hi = chunk_box(entries[i:i + nb, :3], (p0, p1, p2))
            for mi, m in enumerate(models):
                for t in range(T):
                    if T > 1:
                        out = m.forward_mc(patches, seed, ((ci * T + t) * MAX_MODELS + mi) * _PASS_STRIDE)
                    else:
                        out = m(patches)
                    logits = _logits_of(out)
                    if C is None:
                        C = int(logits.shape[1])
                        if not 2 <= C <= 8:
                            raise ValueError(f"the uncertainty evaluator takes models of 2..8 classes, got {C}")
                        score, sq = torch.zeros((C, ww, hh, dd), **f32), torch.zeros((C, ww, hh, dd), **f32)
                    if logits.shape[1] != C:
                        raise ValueError(f"the models disagree about the class count: {C} and {logits.shape[1]}")
                    lg = logits.permute(0, 2, 3, 4, 1).contiguous().float()      # NDHWC fp32 (free for the HIP nets' outputs)
                    _lib.call("dycon_sw_accumulate_moments", lg.data_ptr(), C, nb, p0, p1, p2, origins.data_ptr() + 16 * i,
                              *(g.data_ptr() for g in tables), score.data_ptr(), cnt.data_ptr(), hsum.data_ptr(), sq.data_ptr(), ww, hh, dd,
                              int3(*lo), int3(*hi), _stream())
    label = torch.empty((ww, hh, dd), dtype=torch.uint8, device=dev)
    maps = [torch.empty((ww, hh, dd), **f32) for _ in range(4)]
    _lib.call("dycon_sw_finalize_uncertainty", score.data_ptr(), cnt.data_ptr(), hsum.data_ptr(), sq.data_ptr(), C, cnt.numel(),
              label.data_ptr(), *(t.data_ptr() for t in maps), _stream())
    prob = score                                                # the probabilities replaced the sums in place
    if any(lo or hi for lo, hi in pads):
        sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, (w, h, d)))
        label, prob, maps = label[sl], prob[..., sl[0], sl[1], sl[2]], [t[sl] for t in maps]
    return UncertaintyMaps(label, prob, *maps)


def test_single_case_uncertainty(models, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None, mc_passes=1,
                                 seed=0):
    """`single_case_uncertainty_device` as numpy arrays: `UncertaintyMaps` with label int64 (w, h, d), prob float32 (C, w, h, d) and
    the four float32 maps."""
    out = single_case_uncertainty_device(models, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device, blend=blend,
                                         mc_passes=mc_passes, seed=seed)
    return UncertaintyMaps(out.label.cpu().numpy().astype(np.int64), *(t.cpu().numpy() for t in out[1:]))


test_single_case_uncertainty.__test__ = False        # an evaluator name in the reference's style, not a pytest case


# ---------------------------------------------------------------- calibration
def calibration_summary(n, correct, conf_sum, brier_sum, nll_sum, unc_hist=None):
    """Host arithmetic on the K-sized outputs of `dycon_calibration_counts`.  n, correct: (K,) counts per confidence bin; conf_sum:
    (K,) sums of the confidences; brier_sum, nll_sum: sums over the N = n.sum() scored voxels; unc_hist: None or (2, K) counts of
    the correct [0] and the wrong [1] voxels per uncertainty bin, low uncertainty first.  Returns a dict:

      ece          sum_b n_b / N * |acc_b - conf_b| over the non-empty bins (Guo et al. 2017)
      mce          max_b |acc_b - conf_b| over the non-empty bins
      brier, nll   the sums over N;  accuracy = correct.sum() / N;  n = N
      reliability  (K, 3) float64: count, accuracy, mean confidence per bin (an empty bin: 0, 0, 0)
      error_auroc  (with unc_hist) area under the ROC curve of "this voxel is wrong" scored by its uncertainty bin: the threshold
                   walks the bins from the most uncertain down, trapezoid over the K + 1 points (ties inside a bin count half);
                   nan when no voxel is wrong or none is correct
      aurc         (with unc_hist) area under the risk-coverage curve: voxels are accepted bin by bin from the least uncertain; after
                   each bin the coverage is the accepted share and the risk the error rate among the accepted; trapezoid over
                   the points of the non-empty prefixes, from coverage 0 at the risk of the first one
    Every ratio is nan when N == 0."""
    n, correct = np.asarray(n, np.int64), np.asarray(correct, np.int64)
    conf_sum = np.asarray(conf_sum, np.float64)
    N = int(n.sum())
    nz = n > 0
    acc = np.divide(correct, n, out=np.zeros(len(n)), where=nz)
    conf = np.divide(conf_sum, n, out=np.zeros(len(n)), where=nz)
    gap = np.abs(acc - conf)
    nan = float("nan")
    out = {"ece": float((n[nz] / N * gap[nz]).sum()) if N else nan, "mce": float(gap[nz].max()) if N else nan,
           "brier": float(brier_sum) / N if N else nan, "nll": float(nll_sum) / N if N else nan,
           "accuracy": int(correct.sum()) / N if N else nan, "n": N,
           "reliability": np.stack([n.astype(np.float64), acc, conf], 1)}
    if unc_hist is not None:
        hist = np.asarray(unc_hist, np.int64).reshape(2, -1)
        right, wrong = hist[0].astype(np.float64), hist[1].astype(np.float64)
        if right.sum() > 0 and wrong.sum() > 0:
            tpr = np.concatenate([[0.0], np.cumsum(wrong[::-1]) / wrong.sum()])
            fpr = np.concatenate([[0.0], np.cumsum(right[::-1]) / right.sum()])
            out["error_auroc"] = float(((fpr[1:] - fpr[:-1]) * (tpr[1:] + tpr[:-1]) / 2).sum())
        else:
            out["error_auroc"] = nan
        taken, missed = np.cumsum(right + wrong), np.cumsum(wrong)
        keep = taken > 0
        if keep.any():
            cov = np.concatenate([[0.0], taken[keep] / taken[-1]])
            risk = missed[keep] / taken[keep]
            risk = np.concatenate([risk[:1], risk])
            out["aurc"] = float(((cov[1:] - cov[:-1]) * (risk[1:] + risk[:-1]) / 2).sum())
        else:
            out["aurc"] = nan
    return out


def _check_calibration_args(prob, label, bins, mask, uncertainty, u_max):
    """the argument errors of `calibration` that need no device; returns (C, K, u_max)"""
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must be an integer in 1..{MAX_BINS}, got {bins!r}")
    shape = tuple(prob.shape)
    if len(shape) < 2 or not 2 <= shape[0] <= 8:
        raise ValueError(f"prob is (C, ...) with C in 2..8, got shape {shape}")
    for name, a in (("label", label), ("mask", mask), ("uncertainty", uncertainty)):
        if a is not None and tuple(a.shape) != shape[1:]:
            raise ValueError(f"{name} has shape {tuple(a.shape)}, prob has {shape[1:]} voxels")
    if uncertainty is None:
        if u_max is not None:
            raise ValueError("u_max is the upper bound of `uncertainty`, which was not given")
        return shape[0], int(bins), 1.0
    u_max = math.log(shape[0]) if u_max is None else float(u_max)
    if not (math.isfinite(u_max) and u_max > 0):
        raise ValueError(f"u_max must be a positive finite number, got {u_max!r}")
    return shape[0], int(bins), u_max


def _to_device(a, dev, dtype):
    t = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
    return t.to(device=dev, dtype=dtype).contiguous()


def calibration(prob, label, bins=15, mask=None, uncertainty=None, u_max=None):
    """Calibration and error detection of a probability map against a label map: the dict of `calibration_summary`.

    prob: (C, ...) float32 probabilities, C in 2..8; label: (...) integer labels in [0, C); CUDA tensors or numpy arrays (moved to
    the device of `prob`, or to cuda:0).  mask: optional (...), only voxels with mask != 0 are scored.  bins = K in 1..64
    equal-width confidence bins: a voxel's confidence c = max_k prob[k] falls in bin min(K - 1, int(c * K)) with c * K in float32.
    uncertainty: optional (...) float32 map, e.g. a map of `single_case_uncertainty_device`, with upper bound u_max (default ln C,
    the bound of the entropies): it is binned the same way as u / u_max * K and gives `error_auroc` and `aurc`.

    One counting pass on the device (`dycon_calibration_counts`: integer counts, fp64 sums in a fixed order, the same bits on every
    run); the rest is host arithmetic on K-sized arrays.  ValueError when a scored label lies outside [0, C)."""
    C, K, u_max = _check_calibration_args(prob, label, bins, mask, uncertainty, u_max)
    dev = prob.device if torch.is_tensor(prob) and prob.is_cuda else torch.device("cuda:0")
    p = _to_device(prob, dev, torch.float32)
    lab = torch.as_tensor(np.asarray(label)) if not torch.is_tensor(label) else label
    if lab.dtype != torch.uint8:
        lab = lab.to(dev)
        lab = torch.where((lab < 0) | (lab > 255), torch.full_like(lab, 255), lab)      # outside [0, C) either way
    lab = _to_device(lab, dev, torch.uint8)
    msk = None if mask is None else _to_device((mask if torch.is_tensor(mask) else torch.as_tensor(np.asarray(mask))) != 0, dev, torch.uint8)
    unc = None if uncertainty is None else _to_device(uncertainty, dev, torch.float32)
    V = lab.numel()
    counts = torch.empty(4 * K + 2, dtype=torch.int64, device=dev)
    sums = torch.empty(K + 2, dtype=torch.float64, device=dev)
    ws_bytes = _lib.query("dycon_calibration_workspace", V, K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    _lib.call("dycon_calibration_counts", p.data_ptr(), lab.data_ptr(), None if msk is None else msk.data_ptr(),
              None if unc is None else unc.data_ptr(), u_max, C, V, K, counts.data_ptr(), sums.data_ptr(), ws.data_ptr(), ws_bytes, _stream())
    counts, sums = counts.cpu().numpy(), sums.cpu().numpy()
    if counts[4 * K + 1]:
        raise ValueError(f"{int(counts[4 * K + 1])} scored voxels have a label outside [0, {C})")
    return calibration_summary(counts[:K], counts[K:2 * K], sums[:K], sums[K], sums[K + 1],
                               counts[2 * K:4 * K].reshape(2, K) if unc is not None else None)


SCALARS = ("ece", "mce", "brier", "nll", "accuracy", "error_auroc", "aurc")


def test_all_case_uncertainty(model, cases, num_classes, patch_size=(96, 96, 64), stride_xy=16, stride_z=4, *, blend=None, mc_passes=1,
                              seed=0, bins=15, uncertainty="entropy", batch_size=4):
    """The case loop (`case_loop.mean_over_cases`; cases as `test_all_case` takes them) of the uncertainty evaluator: every case goes
    through `single_case_uncertainty_device` and `calibration` with the map named by `uncertainty` ("entropy", "expected_entropy",
    "mutual_info": u_max = ln C; "variance": u_max = 1 - 1 / C).  The maps never leave the device: per case only the K-sized counts
    are read back.  model: one module or a sequence of 1..4 members.  Returns {"per_case": [`calibration`'s dict per case], "mean":
    dict of the scalars `SCALARS` averaged over the cases}."""
    if uncertainty not in UncertaintyMaps._fields[2:]:
        raise ValueError(f"uncertainty is one of {UncertaintyMaps._fields[2:]}, got {uncertainty!r}")
    _check_members(model, mc_passes)
    _check_calibration_args(np.empty((num_classes, 0)), None, bins, None, None, None)
    u_max = 1.0 - 1.0 / num_classes if uncertainty == "variance" else math.log(num_classes)
    per_case = []

    def one(image, label, spacing):
        maps = single_case_uncertainty_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, blend=blend,
                                              mc_passes=mc_passes, seed=seed)
        if maps.prob.shape[0] != num_classes:
            raise ValueError(f"num_classes = {num_classes}, the model has {maps.prob.shape[0]} classes")
        res = calibration(maps.prob, np.asarray(label), bins=bins, uncertainty=getattr(maps, uncertainty), u_max=u_max)
        per_case.append(res)
        return np.array([res[k] for k in SCALARS], np.float64)

    mean = case_loop.mean_over_cases(cases, one, np.zeros(len(SCALARS)), triples=True)
    return {"per_case": per_case, "mean": dict(zip(SCALARS, (float(v) for v in mean)))}


test_all_case_uncertainty.__test__ = False
