#!/usr/bin/env python3
"""Golden fixture of the reference's two preprocessing scripts (code/BraTS19_DataPreprocessing.py, code/ISLES22_DataPreprocessing.py)
by IMPORTING them on the CPU (the stub-module recipe of make_golden_sdf.py).  Both import h5py, nibabel and tqdm at the top, none of
which is installed: stand-ins go into sys.modules.  The stand-in `nib.load` serves in-memory arrays by file name, the stand-in
`h5py.File` captures the datasets and attributes written, so process_brats_case and process_isles_bids_case run end to end over a
temporary tree of empty files.  Their target shapes are literals inside the functions, (192, 192, 64) and (112, 112, 64); to keep the
fixture small the functions are run with that one constant of their code objects replaced by resample_ref.GOLDEN_TARGET -- every
instruction is still the reference's.

Stores data only (preprocess.npz), for every volume of resample_ref.golden_volumes():
  vol.<name>.image, vol.<name>.seg          the float64 arrays get_fdata hands over
  norm.<name>                               normalize_image(image), float32 (both scripts: asserted equal)      (BraTS :8-31)
  brats.<name>.image, brats.<name>.label    the datasets process_brats_case writes, float32 / uint8            (BraTS :127-217)
  isles.<name>.image, isles.<name>.mask     the datasets process_isles_bids_case writes, float64 / float64     (ISLES :110-223)
and
  brats.attrs, isles.attrs                  the attributes written for the first volume, as "key=value" strings
  split.cases, split.train, split.val, split.train_list, split.val_list     create_split_files(SPLIT_NAMES): the returned case
                                            lists and the lines of train.list / val.list                        (ISLES :226-262)
  api.brats, api.isles                      "name(parameters)" of the scripts' public functions

    python tests/golden/make_golden_preprocess.py
"""
import contextlib
import importlib
import inspect
import io
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = "/root/reference/code"

import resample_ref as R  # noqa: E402

ARRAYS, WRITTEN = {}, []


class _Image:
    def __init__(self, path):
        self.path = path

    def get_fdata(self):
        return ARRAYS[os.path.basename(self.path)].copy()


class _H5File:
    def __init__(self, path, mode):
        assert mode == "w"
        self.path, self.datasets, self.attrs = path, {}, {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        WRITTEN.append(self)
        return False

    def create_dataset(self, name, data, compression=None):
        self.datasets[name] = np.array(data)


nib, h5py, tqdm = types.ModuleType("nibabel"), types.ModuleType("h5py"), types.ModuleType("tqdm")
nib.load, h5py.File, tqdm.tqdm = _Image, _H5File, lambda it, **kw: it
sys.modules.update(nibabel=nib, h5py=h5py, tqdm=tqdm)
sys.path.insert(0, REF)
brats = importlib.import_module("BraTS19_DataPreprocessing")
isles = importlib.import_module("ISLES22_DataPreprocessing")


def with_target(fn, literal):
    code = fn.__code__
    assert literal in code.co_consts
    consts = tuple(R.GOLDEN_TARGET if c == literal else c for c in code.co_consts)
    return types.FunctionType(code.replace(co_consts=consts), fn.__globals__, fn.__name__, fn.__defaults__, fn.__closure__)


process_brats = with_target(brats.process_brats_case, (192, 192, 64))
process_isles = with_target(isles.process_isles_bids_case, (112, 112, 64))


def touch(*parts):
    os.makedirs(os.path.join(*parts[:-1]), exist_ok=True)
    open(os.path.join(*parts), "w").close()


out = {}
quiet = contextlib.redirect_stdout(io.StringIO())
with tempfile.TemporaryDirectory() as tmp, quiet:
    for n, (name, (image, seg)) in enumerate(R.golden_volumes().items()):
        out[f"vol.{name}.image"], out[f"vol.{name}.seg"] = image, seg
        norm = brats.normalize_image(image)
        assert norm.dtype == np.float32 and np.array_equal(norm, isles.normalize_image(image))
        out[f"norm.{name}"] = norm

        case = f"BraTS19_TEST_{n}_1"
        ARRAYS[f"{case}_t2.nii.gz"], ARRAYS[f"{case}_seg.nii.gz"] = image, seg
        for kind in ("t2", "seg", "flair"):
            touch(tmp, "b", "HGG", case, f"{case}_{kind}.nii.gz")
        os.makedirs(os.path.join(tmp, "bo"), exist_ok=True)
        assert process_brats(os.path.join(tmp, "b"), case, os.path.join(tmp, "bo")) is True
        f = WRITTEN.pop()
        assert f.path.endswith(f"{case}.h5") and f.datasets["image"].dtype == np.float32 and f.datasets["label"].dtype == np.uint8
        assert f.datasets["image"].shape == R.GOLDEN_TARGET
        out[f"brats.{name}.image"], out[f"brats.{name}.label"] = f.datasets["image"], f.datasets["label"]
        if n == 0:
            out["brats.attrs"] = np.array(sorted(f"{k}={v}" for k, v in f.attrs.items()))

        case = f"sub-strokecase{n + 1:04d}"
        ARRAYS[f"{case}_ses-0001_dwi.nii.gz"], ARRAYS[f"{case}_ses-0001_msk.nii.gz"] = image, seg
        touch(tmp, "i", case, "ses-0001", "dwi", f"{case}_ses-0001_dwi.nii.gz")
        touch(tmp, "i", "derivatives", case, "ses-0001", f"{case}_ses-0001_msk.nii.gz")
        os.makedirs(os.path.join(tmp, "io"), exist_ok=True)
        assert process_isles(os.path.join(tmp, "i"), case, os.path.join(tmp, "io")) is True
        f = WRITTEN.pop()
        assert f.path.endswith(f"case_{n + 1:04d}.h5") and f.datasets["image"].dtype == np.float64 == f.datasets["mask"].dtype
        assert f.datasets["image"].shape == R.GOLDEN_TARGET
        out[f"isles.{name}.image"], out[f"isles.{name}.mask"] = f.datasets["image"], f.datasets["mask"]
        if n == 0:
            out["isles.attrs"] = np.array(sorted(f"{k}={v}" for k, v in f.attrs.items()))

    train, val = isles.create_split_files(list(R.SPLIT_NAMES), tmp)
    out["split.cases"], out["split.train"], out["split.val"] = np.array(R.SPLIT_NAMES), np.array(train), np.array(val)
    for which in ("train", "val"):
        out[f"split.{which}_list"] = np.array(open(os.path.join(tmp, f"{which}.list")).read().split("\n"))

for key, mod in (("brats", brats), ("isles", isles)):
    out[f"api.{key}"] = np.array(sorted(f"{n}{inspect.signature(f)}" for n, f in vars(mod).items()
                                        if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_")))

path = os.path.join(HERE, "preprocess.npz")
np.savez_compressed(path, **out)
print({k: v.shape for k, v in out.items()}, os.path.getsize(path))
