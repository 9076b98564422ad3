"""Device-resident training data: the whole training set cached in HBM, batches assembled by one HIP launch.

    DeviceVolumeCache(samples, device, pre, max_bytes)        every case once: images fp32, labels uint8, two arenas in HBM
    draw_plan(shapes, indices, patch_size, rot_flip, center, order)   host: the crops / rotations / flips RandomCrop + RandomRotFlip
                                                              would draw, crop first (BraTS, Pancreas, ISLES) or rot/flip first (LA)
    apply_plan_host(plan, images, labels)                     host: numpy restatement of the kernel (the CPU-testable twin)
    assemble_batch(cache, plan, out, label_dtype)             device: dycon_assemble_batch, one launch per 16 samples
    DeviceBatchLoader(cache, batch_sampler, patch_size, ...)  iterates a batch sampler, yields {"image", "label"} device batches
                                                              (rot / onehot / noise_sigma: RandomRot, CreateOnehotLabel and
                                                              RandomNoise on the same path, device_augment.py)

The training pipelines of the reference's three scripts are `[SagittalToAxial ->] RandomCrop -> RandomRotFlip -> ToTensor`
(train_DyCON_BraTS19.py:238-242, train_DyCON_Pancreas.py:150-167, train_DyCON_ISLES22.py:165-190) in DataLoader worker processes.
A conditional zero pad, a crop, a rotation by k * 90 degrees about the first two axes and a flip of axis 0 or 1 are gathers, so the
kernel (csrc/datapath.hip) writes the (B, 1, w, h, d) batch and its labels straight from the cached volumes -- the padded array of
the reference never exists, a source index outside the stored volume reads as 0.

What is equal to what.  For a seeded ``np.random`` the loader yields, bit for bit, what
``DataLoader(dataset_with_the_transform_chain, batch_sampler=..., num_workers=0)`` yields with the transforms of
dataloaders/brats19.py: `draw_plan` consumes ``np.random`` exactly as RandomCrop then RandomRotFlip do for each index in order
(three randint for the crop with bounds from the padded shape, then k, then the axis), between the batch sampler's own draws.
The reference's multi-worker stream (num_workers=4, every worker with its own copy of the generator state) is not reproducible by
anything, this loader included.
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib, ops

#: one output sample: the case, the crop origin in STORED coordinates (crop offset - pad: negative where the reference pads), the
#: np.rot90 count, the flipped axis (-1: none) and the patch it belongs to
PLAN_DTYPE = np.dtype([("case", "<i8"), ("origin", "<i4", (3,)), ("k", "<i4"), ("flip_axis", "<i4"), ("patch", "<i4", (3,))])

# dycon_crop_job_t (include/dycon_hip.h), field for field
_JOB_DTYPE = np.dtype([("image_off", "<i8"), ("label_off", "<i8"), ("X", "<i4"), ("Y", "<i4"), ("Z", "<i4"),
                       ("ox", "<i4"), ("oy", "<i4"), ("oz", "<i4"), ("k", "<i4"), ("flip_axis", "<i4")], align=True)
JOBS_PER_LAUNCH = 16           # DYCON_CROP_JOBS_MAX
_ALIGN = 16                    # bytes: every case starts at a 16-byte-aligned offset of its arena


def _host_label(label):
    """labels as uint8: integers 0..255 in any integer / bool / float dtype (ISLES stores its mask as float64)"""
    a = np.asarray(label)
    if a.dtype == np.uint8:
        return a
    if a.dtype == np.bool_:
        return a.astype(np.uint8)
    if not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"labels must be integers in 0..255, got dtype {a.dtype}")
    if a.size and not (a.min() >= 0 and a.max() <= 255):        # also rejects NaN
        raise ValueError(f"labels must be integers in 0..255, got values in [{a.min()}, {a.max()}]")
    u = a.astype(np.uint8)
    if np.issubdtype(a.dtype, np.floating) and not np.array_equal(u, a):
        raise ValueError("labels must be integers in 0..255, got non-integral values")
    return u


class DeviceVolumeCache:
    """Every case of `samples` (an iterable of {"image", "label"} host arrays: a dataset of this package built with
    ``transform=None`` qualifies) resident on `device`: images as fp32 in one arena, labels as uint8 in another, each case
    C-contiguous at a 16-byte-aligned offset.

    pre: an optional DETERMINISTIC transform applied on the host once per case before it is stored -- meant for
    ``SagittalToAxial()``, so that the cached orientation is the one whose last axis the crop keeps contiguous.
    max_bytes: upper bound of `nbytes`; exceeded -> ValueError before anything is allocated on the device.

    The image is cast to fp32 at insertion.  ToTensor casts after the gathers (crop, rot90, flip and the zero pad move or insert
    values, they compute none), and a cast applied to every element commutes with a gather, so the bits are the same.
    Labels must be integers in 0..255 (any integer, bool or float dtype); anything else raises ValueError."""

    def __init__(self, samples, device=None, pre=None, max_bytes=None):
        self.device = torch.device("cuda" if device is None else device)
        images, labels, self._shapes = [], [], []
        img_off, lab_off, ni, nl = [], [], 0, 0
        for s in samples:
            if pre is not None:
                s = pre(s)
            img = np.ascontiguousarray(np.asarray(s["image"]), dtype=np.float32)
            lab = np.ascontiguousarray(_host_label(s["label"]))
            if img.ndim != 3 or img.shape != lab.shape:
                raise ValueError(f"a case is a 3-D image with a label of its shape, got {img.shape} and {lab.shape}")
            img_off.append(ni)
            lab_off.append(nl)
            ni += -(-img.size // (_ALIGN // 4)) * (_ALIGN // 4)
            nl += -(-lab.size // _ALIGN) * _ALIGN
            if max_bytes is not None and 4 * ni + nl > max_bytes:
                raise ValueError(f"the cache needs more than max_bytes = {max_bytes} (at case {len(images)}: {4 * ni + nl} bytes)")
            images.append(img)
            labels.append(lab)
            self._shapes.append(tuple(int(v) for v in img.shape))
        if not images:
            raise ValueError("no cases to cache")
        self._nbytes = 4 * ni + nl
        self._img_off = np.asarray(img_off, dtype=np.int64)
        self._lab_off = np.asarray(lab_off, dtype=np.int64)
        self._shape_arr = np.asarray(self._shapes, dtype=np.int32)
        self.images = torch.zeros(ni, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(nl, dtype=torch.uint8, device=self.device)
        for img, lab, oi, ol in zip(images, labels, img_off, lab_off):
            self.images[oi:oi + img.size].copy_(torch.from_numpy(img.reshape(-1)))
            self.labels[ol:ol + lab.size].copy_(torch.from_numpy(lab.reshape(-1)))

    def __len__(self):
        return len(self._shapes)

    @property
    def shapes(self):
        """stored (X, Y, Z) of every case (after `pre`)"""
        return list(self._shapes)

    @property
    def nbytes(self):
        """bytes of the two arenas"""
        return self._nbytes

    def host_case(self, idx):
        """(image fp32, label uint8) of one case as host arrays: what the kernel reads (tests, apply_plan_host)"""
        n = int(np.prod(self._shapes[idx]))
        oi, ol = int(self._img_off[idx]), int(self._lab_off[idx])
        return (self.images[oi:oi + n].cpu().numpy().reshape(self._shapes[idx]),
                self.labels[ol:ol + n].cpu().numpy().reshape(self._shapes[idx]))

    @classmethod
    def from_device_cases(cls, images, labels, max_bytes=None):
        """A cache of cases that already live on the device (the outputs of preprocessing.preprocess_*_volume): `images` and
        `labels` are equally long lists of CUDA tensors, a 3-D image and a label of its shape per case.  The two arenas are filled
        with device-to-device copies on the current stream; offsets, alignment and contents are those `__init__` gives the same
        cases from the host.  Images are cast to fp32; labels are uint8 or bool as they are, other integer and float dtypes are
        converted on the device and must hold integers in 0..255 (checked by one device reduction per such case, read back)."""
        images, labels = list(images), list(labels)
        if not images:
            raise ValueError("no cases to cache")
        if len(images) != len(labels):
            raise ValueError(f"{len(images)} images and {len(labels)} labels")
        self = cls.__new__(cls)
        self.device = images[0].device
        self._shapes, img_off, lab_off, ni, nl, labs = [], [], [], 0, 0, []
        for n, (img, lab) in enumerate(zip(images, labels)):
            if not (torch.is_tensor(img) and torch.is_tensor(lab) and img.is_cuda and img.device == self.device
                    and lab.device == self.device):
                raise ValueError(f"case {n}: images and labels are CUDA tensors on one device (host cases go through __init__)")
            if img.dim() != 3 or img.shape != lab.shape:
                raise ValueError(f"a case is a 3-D image with a label of its shape, got {tuple(img.shape)} and {tuple(lab.shape)}")
            if lab.dtype not in (torch.uint8, torch.bool):
                if lab.dtype.is_complex:
                    raise ValueError(f"labels must be integers in 0..255, got dtype {lab.dtype}")
                u = lab.to(torch.uint8)
                if lab.numel() and not bool(((lab >= 0) & (lab <= 255) & (u == lab)).all()):        # also rejects NaN
                    raise ValueError("labels must be integers in 0..255")
                lab = u
            labs.append(lab)
            img_off.append(ni)
            lab_off.append(nl)
            ni += -(-img.numel() // (_ALIGN // 4)) * (_ALIGN // 4)
            nl += -(-lab.numel() // _ALIGN) * _ALIGN
            if max_bytes is not None and 4 * ni + nl > max_bytes:
                raise ValueError(f"the cache needs more than max_bytes = {max_bytes} (at case {n}: {4 * ni + nl} bytes)")
            self._shapes.append(tuple(int(v) for v in img.shape))
        self._nbytes = 4 * ni + nl
        self._img_off = np.asarray(img_off, dtype=np.int64)
        self._lab_off = np.asarray(lab_off, dtype=np.int64)
        self._shape_arr = np.asarray(self._shapes, dtype=np.int32)
        self.images = torch.zeros(ni, dtype=torch.float32, device=self.device)
        self.labels = torch.zeros(nl, dtype=torch.uint8, device=self.device)
        for img, lab, oi, ol in zip(images, labs, img_off, lab_off):
            self.images[oi:oi + img.numel()].copy_(img.reshape(-1))
            self.labels[ol:ol + lab.numel()].copy_(lab.reshape(-1))
        return self


def _pads(shape, patch):
    """_pad_to of dataloaders/brats19.py as the reference has it: as soon as ANY axis is <= the patch, ALL three axes are padded by
    (size - shape)//2 + 3 per side, clamped at 0"""
    if shape[0] <= patch[0] or shape[1] <= patch[1] or shape[2] <= patch[2]:
        return tuple(max((patch[a] - shape[a]) // 2 + 3, 0) for a in range(3))
    return (0, 0, 0)


ORDERS = ("crop_rotflip", "rotflip_crop")


def _rotflip_crop_record(shape, patch):
    """One sample of the LA order, ``RandomRotFlip()`` then ``RandomCrop(patch)``: draws k, the axis, then the three crop offsets
    with bounds from the ROTATED, then padded shape -> (origin in stored coordinates, k, axis).

    A crop of a rotated and flipped array is the rotation and flip of a crop of the stored array at a mapped origin, and the
    symmetric zero pad commutes with both, so the record is one the kernel already executes.  With r = flip(rot90(x, k), axis) of
    shape (R0, R1, Z) and the crop at (u, v) of r (offset - pad), the flip turns the origin of its axis into R - u - P, and rot90
    maps the pair (U, V) to stored (U, V) | (V, Y - U - P1) | (X - U - P0, Y - V - P1) | (X - V - P0, U) for k = 0 | 1 | 2 | 3."""
    X, Y, Z = shape
    k = np.random.randint(0, 4)
    axis = np.random.randint(0, 2)
    R = (Y, X, Z) if k & 1 else (X, Y, Z)
    pad = _pads(R, patch)
    w, h, d = (R[a] + 2 * pad[a] for a in range(3))
    w1 = np.random.randint(0, w - patch[0])
    h1 = np.random.randint(0, h - patch[1])
    d1 = np.random.randint(0, d - patch[2])
    u, v = w1 - pad[0], h1 - pad[1]
    U = R[0] - u - patch[0] if axis == 0 else u
    V = R[1] - v - patch[1] if axis == 1 else v
    ox, oy = ((U, V), (V, Y - U - patch[1]), (X - U - patch[0], Y - V - patch[1]), (X - V - patch[0], U))[k]
    return (ox, oy, d1 - pad[2]), k, axis


def _plan_args(patch_size, rot_flip, center, order):
    """-> the patch as a tuple of ints; ValueError for arguments draw_plan rejects"""
    patch = tuple(int(v) for v in patch_size)
    if len(patch) != 3 or min(patch) <= 0:
        raise ValueError(f"patch_size must be three positive sizes, got {patch_size}")
    if order not in ORDERS:
        raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
    if order == "rotflip_crop" and (center or not rot_flip):
        raise ValueError("order='rotflip_crop' is the order of RandomRotFlip and RandomCrop: it needs rot_flip=True and center=False")
    return patch


def _draw_record(shape, patch, rot_flip, center, order):
    """One sample of either order (the drawing code of draw_plan, shared with device_augment.draw_plan_rot)
    -> (origin in stored coordinates, k, axis)"""
    if order == "rotflip_crop":
        origin, k, axis = _rotflip_crop_record(shape, patch)
    else:
        pad = _pads(shape, patch)
        w, h, d = (shape[a] + 2 * pad[a] for a in range(3))
        k, axis = 0, -1
        if center:
            w1, h1, d1 = (int(round((s - o) / 2.)) for s, o in zip((w, h, d), patch))
        else:
            w1 = np.random.randint(0, w - patch[0])
            h1 = np.random.randint(0, h - patch[1])
            d1 = np.random.randint(0, d - patch[2])
            if rot_flip:
                k = np.random.randint(0, 4)
                axis = np.random.randint(0, 2)
        origin = (w1 - pad[0], h1 - pad[1], d1 - pad[2])
    if (k & 1) and patch[0] != patch[1]:
        raise ValueError(f"rot90 by k = {k} of a {patch[0]} x {patch[1]} crop does not give a {patch[0]} x {patch[1]} patch")
    return origin, k, axis


def draw_plan(shapes, indices, patch_size, rot_flip=True, center=False, order="crop_rotflip"):
    """The plan of one batch: a PLAN_DTYPE record per entry of `indices` (case numbers into `shapes`).

    Pure host code.  Consumes ``np.random`` exactly as ``RandomCrop(patch_size)`` followed by ``RandomRotFlip()`` do for each index
    in order: three randint for the crop, bounds from the PADDED shape, then k, then the axis (rot_flip=False: the crop only,
    k = 0, no flip).  center=True gives the CenterCrop origin and draws nothing.  An odd k with patch_size[0] != patch_size[1]
    raises ValueError: the rotated crop would not have the patch's shape (the reference could not stack such a batch either).

    order="rotflip_crop" is the LA pipelines' ``RandomRotFlip()`` BEFORE ``RandomCrop(patch_size)``: k, the axis, then the three
    crop offsets from the rotated, then padded shape, translated into the same records (`_rotflip_crop_record`).  It needs
    rot_flip=True and center=False (without the rotation, or with a drawn-nothing centre crop, there is one order only); an odd k
    still needs a square patch, because the kernel rotates the crop."""
    patch = _plan_args(patch_size, rot_flip, center, order)
    plan = np.zeros(len(indices), dtype=PLAN_DTYPE)
    for n, idx in enumerate(indices):
        plan[n] = (idx, *_draw_record(shapes[idx], patch, rot_flip, center, order), patch)
    return plan


def _check_plan(plan, ncases):
    """-> the patch of a well-formed plan; ValueError otherwise (the library rejects the same things: this names them earlier)"""
    plan = np.asarray(plan)
    if plan.dtype != PLAN_DTYPE or plan.ndim != 1 or len(plan) == 0:
        raise ValueError("a plan is a non-empty 1-D array of PLAN_DTYPE records (draw_plan)")
    patch = tuple(int(v) for v in plan["patch"][0])
    if (plan["patch"] != plan["patch"][0]).any() or min(patch) <= 0:
        raise ValueError("all samples of a batch share one positive patch size")
    if plan["case"].min() < 0 or plan["case"].max() >= ncases:
        raise ValueError(f"plan names case {plan['case'].max()} of {ncases}")
    if plan["k"].min() < 0 or plan["k"].max() > 3 or plan["flip_axis"].min() < -1 or plan["flip_axis"].max() > 1:
        raise ValueError("k must be in 0..3 and flip_axis in {-1, 0, 1}")
    if patch[0] != patch[1] and (plan["k"] & 1).any():
        raise ValueError(f"an odd k needs a square patch in the first two axes, got {patch[0]} x {patch[1]}")
    return patch


def apply_plan_host(plan, images, labels):
    """What the kernel does with a plan, in numpy: images / labels are the per-case host arrays in the CACHED orientation.
    -> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8} host arrays."""
    P0, P1, P2 = _check_plan(plan, len(images))
    B = len(plan)
    out_i = np.zeros((B, 1, P0, P1, P2), dtype=np.float32)
    out_l = np.zeros((B, P0, P1, P2), dtype=np.uint8)
    i, j = np.meshgrid(np.arange(P0), np.arange(P1), indexing="ij")
    z = np.arange(P2)
    for n, rec in enumerate(plan):
        img, lab = np.asarray(images[rec["case"]]), np.asarray(labels[rec["case"]])
        X, Y, Z = img.shape
        fi = P0 - 1 - i if rec["flip_axis"] == 0 else i          # undo the flip ...
        fj = P1 - 1 - j if rec["flip_axis"] == 1 else j
        a, b = {0: (fi, fj), 1: (fj, P1 - 1 - fi), 2: (P0 - 1 - fi, P1 - 1 - fj), 3: (P0 - 1 - fj, fi)}[int(rec["k"])]   # ... and the rot90
        sx, sy, sz = rec["origin"][0] + a, rec["origin"][1] + b, rec["origin"][2] + z
        ok = ((sx >= 0) & (sx < X) & (sy >= 0) & (sy < Y))[:, :, None] & ((sz >= 0) & (sz < Z))[None, None, :]
        cx, cy, cz = np.clip(sx, 0, X - 1)[:, :, None], np.clip(sy, 0, Y - 1)[:, :, None], np.clip(sz, 0, Z - 1)[None, None, :]
        out_i[n, 0] = np.where(ok, img[cx, cy, cz], 0).astype(np.float32)
        out_l[n] = np.where(ok, lab[cx, cy, cz], 0).astype(np.uint8)
    return {"image": out_i, "label": out_l}


def assemble_batch(cache, plan, out=None, label_dtype=torch.uint8):
    """-> {"image": (B, 1, w, h, d) float32, "label": (B, w, h, d) uint8 | int64} on the cache's device, enqueued on the current
    stream: one launch of dycon_assemble_batch per 16 samples, no allocation when `out` (a dict of such tensors) is given, no host
    synchronisation.  There is no host fallback: a cache that is not on a GPU raises."""
    P0, P1, P2 = _check_plan(plan, len(cache))
    if label_dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"label_dtype must be torch.uint8 or torch.int64, got {label_dtype}")
    if cache.device.type != "cuda":
        raise _lib.DyconLibraryError("assemble_batch runs on the GPU only (the cache is on %s)" % cache.device)
    B = len(plan)
    if out is None:
        out = {"image": torch.empty((B, 1, P0, P1, P2), dtype=torch.float32, device=cache.images.device),
               "label": torch.empty((B, P0, P1, P2), dtype=label_dtype, device=cache.images.device)}
    image, label = out["image"], out["label"]
    if not (tuple(image.shape) == (B, 1, P0, P1, P2) and image.dtype == torch.float32 and tuple(label.shape) == (B, P0, P1, P2)
            and label.dtype == label_dtype and image.is_contiguous() and label.is_contiguous()
            and image.device == cache.images.device and label.device == cache.images.device):
        raise ValueError("out: contiguous (B, 1, w, h, d) float32 and (B, w, h, d) label_dtype tensors on the cache's device")
    case = plan["case"]
    jobs = np.empty(B, dtype=_JOB_DTYPE)
    jobs["image_off"], jobs["label_off"] = cache._img_off[case], cache._lab_off[case]
    jobs["X"], jobs["Y"], jobs["Z"] = cache._shape_arr[case].T
    jobs["ox"], jobs["oy"], jobs["oz"] = plan["origin"].T
    jobs["k"], jobs["flip_axis"] = plan["k"], plan["flip_axis"]
    vox, lb = P0 * P1 * P2, label.element_size()
    stream = ops._s()
    for n0 in range(0, B, JOBS_PER_LAUNCH):
        n = min(JOBS_PER_LAUNCH, B - n0)
        _lib.call("dycon_assemble_batch", cache.images.data_ptr(), cache.labels.data_ptr(), jobs.ctypes.data + n0 * _JOB_DTYPE.itemsize,
                  n, P0, P1, P2, image.data_ptr() + 4 * vox * n0, label.data_ptr() + lb * vox * n0, lb, stream)
    return out


class DeviceBatchLoader:
    """Iterating walks `batch_sampler` (any sampler of this package: TwoStreamBatchSampler, ThreeStreamBatchSampler, ...): for each
    batch of case indices the plan is drawn (draw_plan) and the batch assembled on the current stream into a ring of TWO output
    buffer pairs, so a yielded batch stays valid until the next-but-one is produced.  ``DyconTrainer.step(b["image"], b["label"])``
    takes the tensors as they are.

    For a seeded ``np.random`` the batches equal those of ``DataLoader(dataset, batch_sampler=batch_sampler, num_workers=0)`` with
    ``transform = Compose([RandomCrop(patch_size), RandomRotFlip(), ToTensor()])`` bit for bit (label_dtype=torch.int64 for
    ToTensor's dtype; `pre=SagittalToAxial()` on the cache for the BraTS chain; rot_flip=False leaves RandomRotFlip out).  The
    reference's multi-worker stream is not reproducible by anything.  order="rotflip_crop": the LA chain
    ``Compose([RandomRotFlip(), RandomCrop(patch_size), ToTensor()])`` (dataloaders/la_heart.py) instead, see `draw_plan`.

    The remaining augmentations of the reference's loader modules (dataloaders/device_augment.py); with their defaults nothing of
    the above changes, calls, draws and bits:
      rot=True          ``RandomRot()`` in front of either chain (scipy's nearest-neighbour rotation by randint(-20, 20) degrees),
                        still bit for bit the host chain: `draw_plan_rot` / `assemble_batch_rot`.
      onehot=C          adds "onehot_label" (B, C, w, h, d) of onehot_dtype (int64 as ToTensor leaves it, uint8 or float32):
                        ``CreateOnehotLabel(C)`` in front of ToTensor, written by the same launch.
      noise_sigma=s     the reference's ``RandomNoise(0, s)``: image + clip(s * N(0, 1), -2 s, 2 s).  The normal deviates are the
                        library's counter-based Philox stream, NOT ``np.random.randn``'s, so this one is equal in distribution
                        only: the image of batch number n of the loader's life is
                        ``ops.add_noise(image, None, s, 2 * s, noise_seed, n << 32)`` of the noise-free image.  A non-zero mu is
                        not offered.  The noisy image is written into the ring buffer, so the two-batch lifetime holds.

    Interpolating augmentations, not in the reference (dataloaders/device_warp.py); with both None nothing of the above changes,
    calls, draws and bits:
      warp=Warp(...)    random scale and rotation about all three axes with linear interpolation (labels: nearest) and elastic
                        deformation, as scipy's affine_transform / map_coordinates compute them: `draw_plan_warp` /
                        `assemble_batch_warp`.
      intensity=Intensity(...)   Gaussian blur (scipy's gaussian_filter) of the drawn samples, then gain, bias and gamma.
    Neither goes together with rot=True (ValueError): Warp has its own rotation.
    Order within a batch: warp-assemble, blur, gain / bias / gamma, then noise_sigma.  The elastic field of batch number n is
    ``elastic_field(B, patch, alpha, sigma, aug_seed, n << 32)`` for the drawn samples: Philox-based like the noise, so a run is
    reproducible but the field equals no host stream.  All of it runs on the current stream into the ring buffers, with no host
    synchronisation and no allocation after the first two batches."""

    def __init__(self, cache, batch_sampler, patch_size, rot_flip=True, label_dtype=torch.uint8, order="crop_rotflip",
                 rot=False, onehot=None, onehot_dtype=torch.int64, noise_sigma=None, noise_seed=0, warp=None, intensity=None,
                 aug_seed=0):
        if order not in ORDERS:
            raise ValueError(f"order must be one of {ORDERS}, got {order!r}")
        if order == "rotflip_crop" and not rot_flip:
            raise ValueError("order='rotflip_crop' needs rot_flip=True")
        if noise_sigma is not None and not noise_sigma > 0:
            raise ValueError(f"noise_sigma must be None or positive, got {noise_sigma}")
        self.cache, self.batch_sampler, self.rot_flip, self.label_dtype = cache, batch_sampler, rot_flip, label_dtype
        self.order = order
        self.rot, self.onehot, self.onehot_dtype = bool(rot), onehot, onehot_dtype
        self.noise_sigma, self.noise_seed = noise_sigma, int(noise_seed)
        self.patch_size = tuple(int(v) for v in patch_size)
        self._ring, self._n, self._clean = [None, None], 0, None
        self.warp, self.intensity, self._aug = warp, intensity, None
        if warp is not None or intensity is not None:
            from .device_warp import Intensity, LoaderAugment, Warp
            if rot:
                raise ValueError("rot=True is the reference's chain on its own: warp has its own rotation, and intensity goes with "
                                 "the warp plan (Warp(p_affine=0) moves nothing)")
            if not (warp is None or isinstance(warp, Warp)) or not (intensity is None or isinstance(intensity, Intensity)):
                raise ValueError("warp must be None or a Warp, intensity None or an Intensity")
            self._aug = LoaderAugment(aug_seed, cache.device)

    def __len__(self):
        return len(self.batch_sampler)

    def plans(self):
        """the host side of an epoch on its own: the plan of every batch, in order (draws as iterating the loader does)"""
        shapes = self.cache.shapes
        if self.rot:
            from .device_augment import draw_plan_rot
        if self._aug is not None:
            from .device_warp import draw_plan_warp
        for batch in self.batch_sampler:
            if self._aug is not None:
                yield draw_plan_warp(shapes, [int(i) for i in batch], self.patch_size, self.warp, self.intensity,
                                     rot_flip=self.rot_flip, order=self.order)
            elif self.rot:
                yield draw_plan_rot(shapes, [int(i) for i in batch], self.patch_size, rot_flip=self.rot_flip, order=self.order)
            else:
                yield draw_plan(shapes, [int(i) for i in batch], self.patch_size, rot_flip=self.rot_flip, order=self.order)

    def _assemble(self, plan, out):
        if self._aug is not None:
            from .device_warp import assemble_batch_warp
            out = assemble_batch_warp(self.cache, plan, out=out, displacement=self._aug.field(plan, self._n),
                                      label_dtype=self.label_dtype, onehot=self.onehot, onehot_dtype=self.onehot_dtype)
            if self.intensity is not None:
                self._aug.values(plan, out["image"], *self.intensity.range)
            return out
        if self.rot or self.onehot is not None:
            from .device_augment import assemble_batch_rot
            return assemble_batch_rot(self.cache, plan, out=out, label_dtype=self.label_dtype, onehot=self.onehot,
                                      onehot_dtype=self.onehot_dtype)
        return assemble_batch(self.cache, plan, out=out, label_dtype=self.label_dtype)

    def __iter__(self):
        for plan in self.plans():
            slot = self._n & 1
            buf = self._ring[slot]
            if buf is None or buf["image"].shape[0] != len(plan):
                buf = None
            if self.noise_sigma is None:
                self._ring[slot] = buf = self._assemble(plan, buf)
            else:
                # the batch is assembled with its image in a buffer of the loader's own, the noisy image goes into the ring
                if buf is None:
                    buf = self._assemble(plan, None)
                    self._clean, buf["image"] = buf["image"], torch.empty_like(buf["image"])
                else:
                    if self._clean.shape != buf["image"].shape:
                        self._clean = torch.empty_like(buf["image"])
                    self._assemble(plan, {**buf, "image": self._clean})
                clean, s = self._clean, float(self.noise_sigma)
                _lib.call("dycon_add_noise", clean.data_ptr(), None, buf["image"].data_ptr(), _lib.F32, clean.numel(), s, 2 * s,
                          self.noise_seed, self._n << 32, ops._s())
                self._ring[slot] = buf
            self._n += 1
            yield buf
