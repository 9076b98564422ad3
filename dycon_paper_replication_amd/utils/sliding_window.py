"""Sliding-window evaluation of one case (code/utils/test_3d_patch.py:293-351): the one driver behind every evaluator of the package.

`_sliding_window` runs the windows of a case through one to four models in chunks of ``batch_size`` and keeps the score and count
maps on the device.  Per chunk: one ``dycon_sw_gather`` launch (the windows straight from the unpadded volume; the origins of the
whole case are uploaded once), the forwards, one accumulate launch; one finalize launch at the end.  The accumulate entry points
all launch the kernel of csrc/sw_accumulate.h:

    one model, 2 classes     dycon_sw_accumulate          class 1 as 1 / (1 + exp(l0 - l1))
    one model, 3..8 classes  dycon_sw_accumulate_c        class 1 of the max-shifted softmax
    2..4 models              dycon_sw_accumulate_ens      the same two expressions on the mean logits
    all classes              dycon_sw_accumulate_all      every class, over the bounding box of the chunk's windows
    any of them, blend=...   dycon_sw_accumulate_weighted the same expressions, weighted and un-mirrored (`Blend`, below)

``blend=None``, the default of every evaluator, is the reference's blending: each window counts 1 for every voxel it covers and is
seen in one orientation.  ``blend=Blend(...)`` adds Gaussian importance weighting and mirror test-time augmentation; it is not in
the reference.  ``Blend("constant")`` goes through the blended entry points and gives the bits of ``blend=None``.

``single_case_device`` / ``test_single_case`` here are the class-1 evaluator of one model, and ``utils.test_3d_patch`` imports
``test_single_case`` under the reference's name.  The class count comes from the channel count of the model's logits, and class 1 of
the C-way softmax is scored, as the reference does (:337-347).  A 1-class model is refused: the reference indexes channel 1.
``utils/eval_classes.py`` (all classes) and ``utils/ensemble_eval.py`` (2..4 models) call the same driver.
"""
from __future__ import annotations

import contextlib
import ctypes
import dataclasses
import math

import numpy as np
import torch

from .. import _lib

MAX_MODELS = 4


@dataclasses.dataclass(frozen=True)
class Blend:
    """How overlapping windows are blended, beyond the reference's plain mean; the ``blend=`` option of every evaluator.

    weighting     "constant": every window counts 1 for every voxel it covers.  "gaussian": a voxel counts with the product over the
                  three window axes of exp(-0.5 * ((i - (p - 1) / 2) / (sigma_scale * p)) ** 2), i its local coordinate and p the
                  window's extent: less near the border, where zero padding makes a CNN least reliable.
    mirror_axes   subset of (0, 1, 2), the window axes (w, h, d) = dims 2, 3, 4 of the batch: every window also goes through the
                  network flipped along every combination of these axes, and the un-flipped softmaxes are averaged (mirror test-time
                  augmentation: 2 ** len(mirror_axes) forwards per window).  Stored sorted.
    """
    weighting: str = "gaussian"
    sigma_scale: float = 0.125
    mirror_axes: tuple = ()

    def __post_init__(self):
        if self.weighting not in ("constant", "gaussian"):
            raise ValueError(f"weighting is 'constant' or 'gaussian', got {self.weighting!r}")
        try:
            sigma = float(self.sigma_scale)
        except (TypeError, ValueError):
            raise ValueError(f"sigma_scale must be a positive finite number, got {self.sigma_scale!r}") from None
        if not (math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma_scale must be a positive finite number, got {self.sigma_scale!r}")
        try:
            axes = tuple(self.mirror_axes)
        except TypeError:
            raise ValueError(f"mirror_axes is a subset of (0, 1, 2), got {self.mirror_axes!r}") from None
        if any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) or a not in (0, 1, 2) for a in axes) or len(set(axes)) != len(axes):
            raise ValueError(f"mirror_axes is a subset of (0, 1, 2) without duplicates, got {self.mirror_axes!r}")
        object.__setattr__(self, "sigma_scale", sigma)
        object.__setattr__(self, "mirror_axes", tuple(sorted(int(a) for a in axes)))


def window_weights(patch_size, blend):
    """The three 1-D float32 importance tables (g0, g1, g2) of a window: a voxel at local coordinate (la, lb, lc) counts with
    (g0[la] * g1[lb]) * g2[lc] in fp32.  Every table is symmetric, so the weight does not depend on the orientation a window was run
    in.  ValueError when the smallest product falls below 1e-30: the weight sum of a voxel that one window covers must stay a normal
    fp32 number, so that score / cnt is a probability and never 0 / 0."""
    tables = []
    for p in (int(v) for v in patch_size):
        if p <= 0:
            raise ValueError(f"patch_size must be positive, got {tuple(patch_size)}")
        if blend.weighting == "constant":
            tables.append(np.ones(p, dtype=np.float32))
        else:
            i = np.arange(p, dtype=np.float64)
            tables.append(np.exp(-0.5 * ((i - (p - 1) / 2) / (blend.sigma_scale * p)) ** 2).astype(np.float32))
    corner = float(tables[0].min()) * float(tables[1].min()) * float(tables[2].min())
    if corner < 1e-30:
        raise ValueError(f"sigma_scale = {blend.sigma_scale} gives a window of {tuple(patch_size)} a corner weight of {corner:.3g} "
                         "(< 1e-30): too narrow for fp32 sums")
    return tuple(tables)


def window_entries(windows, mirror_axes):
    """The entry list of a case, int32 (n_entries, 4) rows (ox, oy, oz, mask): each window of `windows`, in order, once per flip mask
    over `mirror_axes` in ascending mask value (bit a set: axis a is flipped; mask 0, the window as it is, comes first)."""
    masks = [0]
    for a in sorted(mirror_axes):
        masks += [m | (1 << a) for m in masks]
    masks.sort()
    return np.array([(x, y, z, m) for x, y, z in windows for m in masks], dtype=np.int32).reshape(-1, 4)


def _windows(shape, patch_size, stride_xy, stride_z):
    ww, hh, dd = shape
    sx = math.ceil((ww - patch_size[0]) / stride_xy) + 1      # :319-321
    sy = math.ceil((hh - patch_size[1]) / stride_xy) + 1
    sz = math.ceil((dd - patch_size[2]) / stride_z) + 1
    out = []
    for x in range(sx):
        xs = min(stride_xy * x, ww - patch_size[0])
        for y in range(sy):
            ys = min(stride_xy * y, hh - patch_size[1])
            for z in range(sz):
                out.append((xs, ys, min(stride_z * z, dd - patch_size[2])))
    return out


def _center_pads(shape, patch_size):
    """:297-316, :418-437: (front, back) zero pad of every axis shorter than the window"""
    pads = []
    for size, p in zip(shape, patch_size):
        pad = max(p - size, 0)
        pads.append((pad // 2, pad - pad // 2))
    return pads


def _logits_of(out):
    """a 3-tuple (this package's nets: tanh map, logits, features) gives element 1; a 2-tuple gives element 0, as the reference
    unpacks ``y1_l, _ = model_l(x)`` (:460)"""
    if isinstance(out, (tuple, list)):
        if len(out) == 3:
            return out[1]
        if len(out) == 2:
            return out[0]
        raise ValueError(f"a model returns (tanh, logits, features) or (logits, features), got {len(out)} outputs")
    return out


def chunk_box(chunk, patch_size):
    """Bounding box (lo, hi), hi exclusive, of the windows of one chunk: the part of the volume dycon_sw_accumulate_all sweeps."""
    org = np.asarray(chunk, dtype=np.int64).reshape(-1, 3)
    return tuple(int(v) for v in org.min(0)), tuple(int(v) for v in org.max(0) + np.asarray(patch_size))


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _eval_static(models):
    """The models in eval mode with static weights inside the block; each one's `training` flag and `weights_static` are put back."""
    saved = [(m, m.training, getattr(m, "weights_static", None)) for m in models]
    try:
        for m, _, was_static in saved:
            m.eval()
            if was_static is not None:
                m.weights_static = True      # no parameter changes between the windows: pack the weights once (networks/_base.py)
        yield
    finally:
        for m, was_training, was_static in saved:
            m.train(was_training)
            if was_static is not None:
                m.weights_static = was_static


def _sliding_window(models, forwards, image, stride_xy, stride_z, patch_size, batch_size, dev, all_classes=False, blend=None):
    """The windows of `image` ((w, h, d) numpy array or tensor) through `forwards`, one callable per model of `models` that maps the
    (nb, 1, p0, p1, p2) windows of a chunk to (nb, C, p0, p1, p2) logits; the callers validate the models' outputs in there.  The
    models are in eval mode with static weights meanwhile.  Returns CUDA tensors: (label uint8 (w, h, d), prob float32 (w, h, d)) of
    class 1, label = prob > 0.5; with all_classes (label = argmax, prob (C, w, h, d)).

    blend: None, the reference's plain mean over the windows, or a `Blend`.  Then the chunks are `batch_size` consecutive ENTRIES
    (`window_entries`: a window in one orientation, so a chunk may split a window's orientations), gathered by
    `dycon_sw_gather_mirror` and accumulated by `dycon_sw_accumulate_weighted` over the bounding box of the chunk's windows."""
    if blend is not None and not isinstance(blend, Blend):
        raise TypeError(f"blend is None or a sliding_window.Blend, got {type(blend).__name__}")
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))).to(dtype=torch.float32)
    w, h, d = img.shape
    p0, p1, p2 = (int(v) for v in patch_size)
    pads = _center_pads((w, h, d), (p0, p1, p2))               # the pad lives in the gather's index arithmetic: vol stays UNPADDED
    vol = img.to(dev).contiguous()
    ww, hh, dd = (n + lo + hi for n, (lo, hi) in zip((w, h, d), pads))
    wins = _windows((ww, hh, dd), (p0, p1, p2), stride_xy, stride_z)
    if blend is None:
        origins = torch.tensor(wins, dtype=torch.int32).to(dev)     # every window of the case, uploaded once
        n_rows = len(wins)
    else:
        tables = [torch.from_numpy(g).to(dev) for g in window_weights((p0, p1, p2), blend)]
        entries = window_entries(wins, blend.mirror_axes)
        origins = torch.from_numpy(entries).to(dev)                 # every entry of the case, uploaded once
        n_rows = len(entries)
    cnt = torch.zeros((ww, hh, dd), dtype=torch.float32, device=dev)
    score = None
    int3 = ctypes.c_int * 3
    with _eval_static(models), torch.no_grad():
        for i in range(0, n_rows, batch_size):
            nb = min(batch_size, n_rows - i)
            patches = torch.empty((nb, 1, p0, p1, p2), dtype=torch.float32, device=dev)
            _lib.call("dycon_sw_gather" if blend is None else "dycon_sw_gather_mirror", vol.data_ptr(), w, h, d, origins.data_ptr(),
                      n_rows, i, nb, p0, p1, p2, patches.data_ptr(), _stream())
            # (nb, C, p0, p1, p2) channels-last-3D views -> NDHWC fp32 (free for the HIP nets' outputs)
            lgs = [f(patches).permute(0, 2, 3, 4, 1).contiguous().float() for f in forwards]
            C = lgs[0].shape[-1]
            if score is None:
                score = torch.zeros(((C,) if all_classes else ()) + (ww, hh, dd), dtype=torch.float32, device=dev)
            if blend is not None:
                lo, hi = chunk_box(entries[i:i + nb, :3], (p0, p1, p2))
                ptrs = [t.data_ptr() for t in lgs] + [None] * (MAX_MODELS - len(lgs))
                _lib.call("dycon_sw_accumulate_weighted", *ptrs, len(lgs), C, int(all_classes), nb, p0, p1, p2,
                          origins.data_ptr() + 16 * i, *(g.data_ptr() for g in tables), score.data_ptr(), cnt.data_ptr(), ww, hh, dd,
                          int3(*lo), int3(*hi), _stream())
                continue
            maps = (nb, p0, p1, p2, origins.data_ptr() + 12 * i, score.data_ptr(), cnt.data_ptr(), ww, hh, dd)
            if all_classes:
                lo, hi = chunk_box(wins[i:i + nb], (p0, p1, p2))
                _lib.call("dycon_sw_accumulate_all", lgs[0].data_ptr(), C, *maps, int3(*lo), int3(*hi), _stream())
            elif len(lgs) > 1:
                ptrs = [t.data_ptr() for t in lgs] + [None] * (MAX_MODELS - len(lgs))
                _lib.call("dycon_sw_accumulate_ens", *ptrs, len(lgs), C, *maps, _stream())
            elif C == 2:
                _lib.call("dycon_sw_accumulate", lgs[0].data_ptr(), *maps, _stream())
            else:
                _lib.call("dycon_sw_accumulate_c", lgs[0].data_ptr(), C, *maps, _stream())
    label = torch.empty((ww, hh, dd), dtype=torch.uint8, device=dev)
    if all_classes:
        prob = score                                            # the probabilities replace the sums in place
        _lib.call("dycon_sw_finalize_argmax", score.data_ptr(), cnt.data_ptr(), C, cnt.numel(), label.data_ptr(), prob.data_ptr(),
                  _stream())
    else:
        prob = torch.empty_like(score)
        _lib.call("dycon_sw_finalize", score.data_ptr(), cnt.data_ptr(), score.numel(), 0.5, label.data_ptr(), prob.data_ptr(), _stream())
    if any(lo or hi for lo, hi in pads):
        sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, (w, h, d)))
        label, prob = label[sl], prob[..., sl[0], sl[1], sl[2]]
    return label, prob


def single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=4, device=None, *, blend=None):
    """The device-resident form of `test_single_case`: (label uint8 (w, h, d), prob float32 (w, h, d)) as CUDA tensors, the same
    launches in the same order without the copies to the host.  label = prob > 0.5 of the class-1 probability; 2..8 classes.  image:
    (w, h, d) numpy array or tensor.  blend: None or a `Blend`."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the model to 'cuda'")

    def forward(patches):
        logits = model(patches)[1]
        if logits.shape[1] < 2:
            raise ValueError("test_single_case scores class 1 of the softmax (:337): the model needs at least 2 classes")
        return logits

    return _sliding_window([model], [forward], image, stride_xy, stride_z, patch_size, batch_size, dev, blend=blend)


def test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=1, batch_size=4, device=None, *, blend=None):
    """image: (w, h, d) numpy array or tensor.  Returns (label_map int64 (w,h,d), score_map float32 (num_classes,w,h,d)) as numpy,
    like the reference; the class-1 probability fills every channel of score_map (the reference's broadcast, :338-339), and
    label_map = score > 0.5 (:345).  The model may have 2..8 classes.

    ``batch_size`` windows go through the network per launch sequence (the reference runs them one by one).  blend: None, the
    reference's plain mean over the windows, or a `Blend`."""
    label, prob = single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device, blend=blend)
    label_map = label.cpu().numpy().astype(np.int64)
    score_map = np.broadcast_to(prob.cpu().numpy()[None], (num_classes,) + label_map.shape).copy()
    return label_map, score_map


test_single_case.__test__ = False        # the reference's name, not a pytest case
