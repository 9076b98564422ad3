"""Sliding-window evaluation of one case (code/utils/test_3d_patch.py:293-351): the one driver behind every evaluator of the package.

`_sliding_window` runs the windows of a case through one to four models in chunks of ``batch_size`` and keeps the score and count
maps on the device.  Per chunk: one ``dycon_sw_gather`` launch (the windows straight from the unpadded volume; the origins of the
whole case are uploaded once), the forwards, one accumulate launch; one finalize launch at the end.  The accumulate entry points
all launch the kernel of csrc/sw_accumulate.h:

    one model, 2 classes     dycon_sw_accumulate          class 1 as 1 / (1 + exp(l0 - l1))
    one model, 3..8 classes  dycon_sw_accumulate_c        class 1 of the max-shifted softmax
    2..4 models              dycon_sw_accumulate_ens      the same two expressions on the mean logits
    all classes              dycon_sw_accumulate_all      every class, over the bounding box of the chunk's windows

``single_case_device`` / ``test_single_case`` here are the class-1 evaluator of one model, and ``utils.test_3d_patch`` imports
``test_single_case`` under the reference's name.  The class count comes from the channel count of the model's logits, and class 1 of
the C-way softmax is scored, as the reference does (:337-347).  A 1-class model is refused: the reference indexes channel 1.
``utils/eval_classes.py`` (all classes) and ``utils/ensemble_eval.py`` (2..4 models) call the same driver.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .. import _lib

MAX_MODELS = 4


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


def _sliding_window(models, forwards, image, stride_xy, stride_z, patch_size, batch_size, dev, all_classes=False):
    """The windows of `image` ((w, h, d) numpy array or tensor) through `forwards`, one callable per model of `models` that maps the
    (nb, 1, p0, p1, p2) windows of a chunk to (nb, C, p0, p1, p2) logits; the callers validate the models' outputs in there.  The
    models are in eval mode with static weights meanwhile.  Returns CUDA tensors: (label uint8 (w, h, d), prob float32 (w, h, d)) of
    class 1, label = prob > 0.5; with all_classes (label = argmax, prob (C, w, h, d))."""
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))).to(dtype=torch.float32)
    w, h, d = img.shape
    p0, p1, p2 = (int(v) for v in patch_size)
    pads = _center_pads((w, h, d), (p0, p1, p2))               # the pad lives in the gather's index arithmetic: vol stays UNPADDED
    vol = img.to(dev).contiguous()
    ww, hh, dd = (n + lo + hi for n, (lo, hi) in zip((w, h, d), pads))
    wins = _windows((ww, hh, dd), (p0, p1, p2), stride_xy, stride_z)
    origins = torch.tensor(wins, dtype=torch.int32).to(dev)     # every window of the case, uploaded once
    cnt = torch.zeros((ww, hh, dd), dtype=torch.float32, device=dev)
    score = None
    int3 = ctypes.c_int * 3
    saved = [(m, m.training, getattr(m, "weights_static", None)) for m in models]
    try:
        for m, _, was_static in saved:
            m.eval()
            if was_static is not None:
                m.weights_static = True      # no parameter changes between the windows: pack the weights once (networks/_base.py)
        with torch.no_grad():
            for i in range(0, len(wins), batch_size):
                nb = min(batch_size, len(wins) - i)
                patches = torch.empty((nb, 1, p0, p1, p2), dtype=torch.float32, device=dev)
                _lib.call("dycon_sw_gather", vol.data_ptr(), w, h, d, origins.data_ptr(), len(wins), i, nb, p0, p1, p2,
                          patches.data_ptr(), _stream())
                # (nb, C, p0, p1, p2) channels-last-3D views -> NDHWC fp32 (free for the HIP nets' outputs)
                lgs = [f(patches).permute(0, 2, 3, 4, 1).contiguous().float() for f in forwards]
                C = lgs[0].shape[-1]
                if score is None:
                    score = torch.zeros(((C,) if all_classes else ()) + (ww, hh, dd), dtype=torch.float32, device=dev)
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
    finally:
        for m, was_training, was_static in saved:
            m.train(was_training)
            if was_static is not None:
                m.weights_static = was_static
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


def single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=4, device=None):
    """The device-resident form of `test_single_case`: (label uint8 (w, h, d), prob float32 (w, h, d)) as CUDA tensors, the same
    launches in the same order without the copies to the host.  label = prob > 0.5 of the class-1 probability; 2..8 classes.  image:
    (w, h, d) numpy array or tensor."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the model to 'cuda'")

    def forward(patches):
        logits = model(patches)[1]
        if logits.shape[1] < 2:
            raise ValueError("test_single_case scores class 1 of the softmax (:337): the model needs at least 2 classes")
        return logits

    return _sliding_window([model], [forward], image, stride_xy, stride_z, patch_size, batch_size, dev)


def test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=1, batch_size=4, device=None):
    """image: (w, h, d) numpy array or tensor.  Returns (label_map int64 (w,h,d), score_map float32 (num_classes,w,h,d)) as numpy,
    like the reference; the class-1 probability fills every channel of score_map (the reference's broadcast, :338-339), and
    label_map = score > 0.5 (:345).  The model may have 2..8 classes.

    ``batch_size`` windows go through the network per launch sequence (the reference runs them one by one)."""
    label, prob = single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device)
    label_map = label.cpu().numpy().astype(np.int64)
    score_map = np.broadcast_to(prob.cpu().numpy()[None], (num_classes,) + label_map.shape).copy()
    return label_map, score_map


test_single_case.__test__ = False        # the reference's name, not a pytest case
