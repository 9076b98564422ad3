"""Sliding-window evaluation of one case for models with any class count (code/utils/test_3d_patch.py:293-351).

``utils/test_3d_patch.py`` holds the evaluator for 2-class models and is left as it is; a model that declares ``n_classes == 2``
(every 2-class net of this package) still runs through it.  ``test_single_case`` here is what the package binds under the
reference's name (``utils.test_3d_patch.test_single_case``, see ``utils/__init__.py``): it takes the class count from the model
(or, for a module that does not declare one, from the channel count of its logits) and scores class 1 of the C-way softmax, as the
reference does (:337-347): ``dycon_sw_accumulate_c`` for 3..8 classes.  A 1-class model is refused: the reference indexes channel 1.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from . import test_3d_patch as _two
from .test_3d_patch import _windows

_two_class_single_case = _two.test_single_case        # the function written in test_3d_patch.py (bound before utils/__init__ rebinds the name)
assert _two_class_single_case.__module__ == _two.__name__


def single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=4, device=None):
    """The device-resident form of `test_single_case`: (label uint8 (w, h, d), prob float32 (w, h, d)) as CUDA tensors, the same
    launches in the same order without the copies to the host.  label = prob > 0.5 of the class-1 probability; 2..8 classes.  image:
    (w, h, d) numpy array or tensor."""
    dev = torch.device(device) if device is not None else next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError("the sliding window runs on the MI355X only: move the model to 'cuda'")
    img = (image if torch.is_tensor(image) else torch.as_tensor(np.asarray(image))).to(dtype=torch.float32)
    w, h, d = img.shape
    pads = []
    for size, p in zip((w, h, d), patch_size):                 # :297-316: centre-pad volumes smaller than the window
        pad = max(p - size, 0)
        pads.append((pad // 2, pad - pad // 2))
    add_pad = any(lo or hi for lo, hi in pads)
    vol = img.to(dev)
    if add_pad:
        vol = torch.nn.functional.pad(vol, (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    vol = vol.contiguous()
    ww, hh, dd = vol.shape
    wins = _windows((ww, hh, dd), patch_size, stride_xy, stride_z)
    score = torch.zeros((ww, hh, dd), dtype=torch.float32, device=dev)
    cnt = torch.zeros_like(score)
    p0, p1, p2 = patch_size
    stream = lambda: torch.cuda.current_stream().cuda_stream   # noqa: E731
    was_training = model.training
    was_static = getattr(model, "weights_static", None)
    model.eval()
    if was_static is not None:
        model.weights_static = True      # no parameter changes between the windows: pack the weights once (networks/_base.py)
    try:
        with torch.no_grad():
            for i in range(0, len(wins), batch_size):
                chunk = wins[i:i + batch_size]
                patches = torch.stack([vol[x:x + p0, y:y + p1, z:z + p2] for x, y, z in chunk]).unsqueeze(1).contiguous()
                logits = model(patches)[1]                                        # (nb, C, p0, p1, p2), channels-last-3D view
                C = logits.shape[1]
                if C < 2:
                    raise ValueError("test_single_case scores class 1 of the softmax (:337): the model needs at least 2 classes")
                lg = logits.permute(0, 2, 3, 4, 1).contiguous().float()          # NDHWC (free for the HIP nets' outputs)
                org = torch.tensor(chunk, dtype=torch.int32).to(dev)
                if C == 2:
                    _lib.call("dycon_sw_accumulate", lg.data_ptr(), len(chunk), p0, p1, p2, org.data_ptr(), score.data_ptr(),
                              cnt.data_ptr(), ww, hh, dd, stream())
                else:
                    _lib.call("dycon_sw_accumulate_c", lg.data_ptr(), C, len(chunk), p0, p1, p2, org.data_ptr(), score.data_ptr(),
                              cnt.data_ptr(), ww, hh, dd, stream())
    finally:
        model.train(was_training)
        if was_static is not None:
            model.weights_static = was_static
    label = torch.empty((ww, hh, dd), dtype=torch.uint8, device=dev)
    prob = torch.empty_like(score)
    _lib.call("dycon_sw_finalize", score.data_ptr(), cnt.data_ptr(), score.numel(), 0.5, label.data_ptr(), prob.data_ptr(), stream())
    if add_pad:
        sl = tuple(slice(lo, lo + n) for (lo, _), n in zip(pads, (w, h, d)))
        label, prob = label[sl], prob[sl]
    return label, prob


def test_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=1, batch_size=4, device=None):
    """image: (w, h, d) numpy array or tensor.  Returns (label_map int64 (w,h,d), score_map float32 (num_classes,w,h,d)) as numpy,
    like the reference; the class-1 probability fills every channel of score_map (the reference's broadcast, :338-339), and
    label_map = score > 0.5 (:345).  The model may have 2..8 classes.

    ``batch_size`` windows go through the network per launch sequence (the reference runs them one by one)."""
    if getattr(model, "n_classes", None) == 2:
        return _two_class_single_case(model, image, stride_xy, stride_z, patch_size, num_classes=num_classes, batch_size=batch_size,
                                      device=device)
    label, prob = single_case_device(model, image, stride_xy, stride_z, patch_size, batch_size=batch_size, device=device)
    label_map = label.cpu().numpy().astype(np.int64)
    score_map = np.broadcast_to(prob.cpu().numpy()[None], (num_classes,) + label_map.shape).copy()
    return label_map, score_map


test_single_case.__test__ = False        # the reference's name, not a pytest case
