"""Preprocessing without a GPU: the numpy restatement (tests/resample_ref.py) against scipy and against the reference's recorded
outputs (tests/golden/preprocess.npz, written by tests/golden/make_golden_preprocess.py), the name mirrors' signatures, split files
and file finding, the C ABI of csrc/resample.hip, and the refusals that come before the library is touched.

Tolerances, measured here on this CPU and asserted below (the GPU tests import the constants):
  ZOOM1_SCIPY_F64 / _F32   largest |scipy.ndimage.zoom(order=1) - resample_ref.zoom| over the 15 shape pairs and the three unit-normal
                           volumes per shape that the GPU test batches (resample_ref.zoom_input, seeds 0..2): 6.67e-16 (fp64
                           output), 1.20e-7 (fp32 output: one ulp of a value in [1, 2), where the two fp64 sums fall on either
                           side of a rounding boundary).  The only source is scipy's summation order (separable, axis by axis);
                           the bound of a comparison with scipy is twice that.
  NORM_REF_F64             largest |recorded reference normalize_image (float32) - the same function in fp64| over the fixture
                           volumes: 7.27e-8.  A device result may be twice that far from a recorded image: the reference's float32
                           pairwise mean cannot be reproduced in bits.
  STATS_ORDER_REL          largest relative |numpy fp64 mean / std - the same sums in the kernels' order of additions|
                           (resample_ref.device_stats) over resample_ref.stats_volumes(): 0 -- numpy's pairwise sums and the
                           kernels' trees round alike on these volumes, below what the format resolves.  The bound is therefore
                           the format's resolution, one fp64 ulp (2^-52 = 2.22e-16, relative); the device statistics may be
                           twice that far from numpy's (they equal device_stats bit for bit).
"""
import inspect
import os
import re

import numpy as np
import pytest
from scipy import ndimage

import resample_ref as R
from conftest import ROOT, load_golden

from dycon_paper_replication_amd import BraTS19_DataPreprocessing as BR
from dycon_paper_replication_amd import ISLES22_DataPreprocessing as IS
from dycon_paper_replication_amd import _lib, preprocessing
from dycon_paper_replication_amd.dataloaders import device_cache

ZOOM1_SCIPY_F64, ZOOM1_SCIPY_F32 = 6.67e-16, 1.20e-7
ZOOM_SEEDS = (0, 1, 2)
NORM_REF_F64 = 7.27e-8
STATS_ORDER_REL = 2.0 ** -52
INVALID = -22                                   # DYCON_ERR_INVALID

ALL_PAIRS = R.SHAPE_PAIRS + R.EXTRA_PAIRS
NEW_ABI = {"dycon_volume_stats_workspace", "dycon_volume_stats", "dycon_normalize_apply", "dycon_zoom_workspace", "dycon_zoom"}


def _factors(si, so):
    return [t / s for t, s in zip(so, si)]


@pytest.mark.parametrize("si,so", ALL_PAIRS)
def test_order0_is_scipy_bit_for_bit(si, so):
    x = R.zoom_input(si)
    for a in (x.astype(np.float32), (40 * x).astype(np.uint8)):
        want = ndimage.zoom(a, _factors(si, so), order=0)
        got = R.zoom(a, so, 0)
        assert want.shape == so and got.dtype == want.dtype and np.array_equal(got, want)


def test_order0_2d_and_ties():
    x = R.zoom_input((7, 9)).astype(np.float32)
    assert np.array_equal(R.zoom(x[:, :, None], (12, 5, 1), 0)[:, :, 0], ndimage.zoom(x, (12 / 7, 5 / 9), order=0))
    assert R.axis_nearest(4, 11).tolist() == [0, 0, 1, 1, 1, 2, 2, 2, 2, 3, 3]          # 4 -> 11: c = 1.5 at i = 5 goes up


def test_order1_against_scipy_within_the_measured_bound():
    worst = {np.float64: 0.0, np.float32: 0.0}
    for si, so in ALL_PAIRS:
        for seed in ZOOM_SEEDS:
            x32 = R.zoom_input(si, seed).astype(np.float32)
            for x, dtype in ((R.zoom_input(si, seed), np.float64), (x32.astype(np.float64), np.float64), (x32, np.float32)):
                want, got = ndimage.zoom(x, _factors(si, so), order=1), R.zoom(x, so, 1)
                assert got.dtype == want.dtype == dtype and got.shape == want.shape == so
                worst[dtype] = max(worst[dtype], float(np.abs(want - got).max()))
    print("order 1, largest |scipy - restatement|:", worst)
    assert 0 < worst[np.float64] <= ZOOM1_SCIPY_F64 and 0 < worst[np.float32] <= ZOOM1_SCIPY_F32


def test_restatement_reproduces_the_recorded_reference():
    g = load_golden("preprocess")
    worst = 0.0
    for name, (image, seg) in R.golden_volumes().items():
        assert np.array_equal(image, g[f"vol.{name}.image"]) and np.array_equal(seg, g[f"vol.{name}.seg"])
        ref = g[f"norm.{name}"]
        assert ref.dtype == np.float32
        worst = max(worst, float(np.abs(ref.astype(np.float64) - R.normalize_image64(image)).max()))
        assert np.abs(R.normalize_image(image) - ref).max() <= 2 * NORM_REF_F64
        for key, thr, lab in (("brats", 0.0, "label"), ("isles", 0.5, "mask")):
            img, label = R.preprocess(image, seg, R.GOLDEN_TARGET, thr)
            assert img.dtype == np.float32 and label.dtype == np.uint8
            assert np.array_equal(label, g[f"{key}.{name}.{lab}"])
            assert np.abs(img.astype(np.float64) - g[f"{key}.{name}.image"]).max() <= 2 * NORM_REF_F64
    print("normalize_image, largest |recorded float32 - fp64 restatement|:", worst)
    assert 0 < worst <= NORM_REF_F64


def test_edge_rules_are_the_references():
    g = load_golden("preprocess")
    rec = {name: R.norm_record(R.volume_stats(image)) for name, (image, _) in R.golden_volumes().items()}
    assert (rec["zero"][0], rec["zero"][3]) == (0, 0) and not g["norm.zero"].any()                   # unchanged
    assert (rec["nopos"][0], rec["nopos"][3]) == (0, 1) and g["norm.nopos"].min() == 0 and g["norm.nopos"].max() == 1
    assert (rec["const"][0], rec["const"][3]) == (0, 1) and set(np.unique(g["norm.const"])) == {0.0, 1.0}
    assert (rec["flat"][0], rec["flat"][3]) == (0, 0) and (g["norm.flat"] == 3).all()                # hi == lo: unchanged
    assert (rec["mri"][0], rec["mri"][3]) == (1, 1)
    for name in ("zero", "nopos", "const", "flat"):                                                  # exact: no mean is involved
        assert np.array_equal(R.normalize_image(g[f"vol.{name}.image"]), g[f"norm.{name}"]), name


def test_stats_order_distance():
    worst = 0.0
    for name, x in R.stats_volumes().items():
        a, b = R.volume_stats(x), R.device_stats(x)
        for f in ("mean", "std"):
            if a[f]:
                worst = max(worst, abs(a[f] - b[f]) / abs(a[f]))
            else:
                assert b[f] == 0
    print("statistics, largest relative |numpy fp64 - kernel order|:", worst)
    assert worst <= STATS_ORDER_REL
    assert R.device_stats(R.stats_volumes()["equal"])["std"] == 0                                    # a constant sums exactly


def test_mirror_names_and_parameter_lists():
    g = load_golden("preprocess")
    for mod, key in ((BR, "api.brats"), (IS, "api.isles")):
        for entry in g[key].tolist():
            name = entry.split("(")[0]
            assert f"{name}{inspect.signature(getattr(mod, name))}" == entry
    assert preprocessing.__all__ == ["VolumeStats", "volume_stats", "normalize_image", "zoom", "preprocess_brats_volume",
                                     "preprocess_isles_volume"]
    assert inspect.signature(preprocessing.preprocess_brats_volume).parameters["target_shape"].default == (192, 192, 64)
    assert inspect.signature(preprocessing.preprocess_isles_volume).parameters["target_shape"].default == (112, 112, 64)
    assert callable(device_cache.DeviceVolumeCache.from_device_cases)


def test_create_split_files(tmp_path):
    g = load_golden("preprocess")
    train, val = IS.create_split_files(g["split.cases"].tolist(), str(tmp_path))
    assert train == g["split.train"].tolist() and val == g["split.val"].tolist()
    for which in ("train", "val"):
        assert (tmp_path / f"{which}.list").read_text().split("\n") == g[f"split.{which}_list"].tolist()


def test_file_finding(tmp_path):
    def touch(*parts):
        p = tmp_path.joinpath(*parts)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")
        return str(p)

    base = str(tmp_path / "b")
    a = {k: touch("b", "HGG", "BraTS19_A_1", f"BraTS19_A_1_{k}.nii.gz") for k in ("t1", "t1ce", "t2", "flair", "seg")}
    touch("b", "LGG", "BraTS19_B_1", "BraTS19_B_1_t2.nii")
    b_seg = touch("b", "LGG", "BraTS19_B_1", "BraTS19_B_1_seg.nii")
    b_flair = touch("b", "LGG", "BraTS19_B_1", "scan_FLAIR_v2.nii.gz")
    touch("b", "LGG", "notes", "readme.txt")
    (tmp_path / "b" / "BraTS19_C_1").mkdir()
    assert BR.find_case_directory(base, "BraTS19_A_1") == os.path.join(base, "HGG", "BraTS19_A_1")
    assert BR.find_case_directory(base, "BraTS19_B_1") == os.path.join(base, "LGG", "BraTS19_B_1")
    assert BR.find_case_directory(base, "BraTS19_C_1") == os.path.join(base, "BraTS19_C_1")
    assert BR.find_case_directory(base, "BraTS19_D_1") is None
    assert BR.find_case_files(os.path.join(base, "HGG", "BraTS19_A_1"), "BraTS19_A_1") == tuple(a[k] for k in ("t1", "t1ce", "t2", "flair", "seg"))
    got = BR.find_case_files(os.path.join(base, "LGG", "BraTS19_B_1"), "BraTS19_B_1")        # two standard names: the keyword pass too
    assert got == (None, None, os.path.join(base, "LGG", "BraTS19_B_1", "BraTS19_B_1_t2.nii"), b_flair, b_seg)
    assert BR.find_case_files(os.path.join(base, "BraTS19_C_1"), "BraTS19_C_1") == (None,) * 5
    assert BR.find_case_files(os.path.join(base, "nowhere"), "x") == (None,) * 5
    assert BR.get_all_available_cases(base) == ["BraTS19_A_1", "BraTS19_B_1"]
    assert BR.process_brats_case(base, "BraTS19_D_1", str(tmp_path)) is False

    ib = str(tmp_path / "i")
    c1, c2 = "sub-strokecase0001", "sub-strokecase0002"
    dwi = touch("i", c1, "ses-0001", "dwi", f"{c1}_ses-0001_dwi.nii.gz")
    adc = touch("i", c1, "ses-0001", "dwi", f"{c1}_ses-0001_adc.nii.gz")
    msk = touch("i", "derivatives", c1, "ses-0001", f"{c1}_ses-0001_msk.nii.gz")
    flair = touch("i", c2, "ses-0001", "anat", f"{c2}_ses-0001_FLAIR.nii.gz")
    touch("i", "sub-strokecase-notes.txt")
    assert IS.get_case_list(ib) == [c1, c2]
    assert IS.find_isles_bids_files(ib, c1) == (dwi, msk)
    assert IS.find_isles_bids_files(ib, c1, "ADC") == (adc, msk)
    assert IS.find_isles_bids_files(ib, c1, "flair") == (dwi, msk)                             # missing: the first other one
    assert IS.find_isles_bids_files(ib, c2) == (flair, None)
    assert IS.find_isles_bids_files(ib, "sub-strokecase0003") == (None, None)
    assert IS.process_isles_bids_case(ib, c2, str(tmp_path)) is False                          # no mask (or no nibabel): reported


def test_abi_names():
    hdr = open(os.path.join(ROOT, "include", "dycon_hip.h")).read()
    declared = set(re.findall(r"\b(dycon_[a-z0-9_]+)\s*\(", hdr))
    assert NEW_ABI <= declared and NEW_ABI <= set(_lib.SIGNATURES)
    assert "BraTS19_DataPreprocessing.py:8-31" in hdr and "ISLES22_DataPreprocessing.py:10-33, :141-159" in hdr
    assert "global: dycon_*;" in open(os.path.join(ROOT, "dycon_paper_replication_amd", "csrc", "exports.map")).read()
    assert "resample.hip" in open(os.path.join(ROOT, "dycon_paper_replication_amd", "csrc", "Makefile")).read()
    lib = _lib.load()
    for name in NEW_ABI:
        assert hasattr(lib, name)
    assert lib.dycon_zoom_workspace(1, 9, 11, 6) == 26 * (2 * 8 + 2 * 4)                     # two weights and two indices per entry
    assert lib.dycon_zoom_workspace(2, 9, 11, 6) == 0 and lib.dycon_zoom_workspace(0, 9, 0, 6) == 0
    assert lib.dycon_volume_stats_workspace(3, 5 * 7 * 4) == 3 * (2 * 8 + 32)                # one workgroup per sample
    assert lib.dycon_volume_stats_workspace(1, 40 * 40 * 30) == 12 * 2 * 8 + 32
    assert lib.dycon_volume_stats_workspace(0, 10) == 0
    assert preprocessing.STATS_BYTES == 48 and preprocessing.RECORD_BYTES == 24


def test_library_rejects_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail differently"""
    lib = _lib.load()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data

    def zoom(order=1, shape=(4, 4, 4), target=(4, 4, 4), ws=4096, src_bytes=4, out_bytes=4):
        return lib.dycon_zoom(p, src_bytes, 1, *shape, *target, order, None, 0, 0.0, p, out_bytes, p, ws, None)

    for kw, msg in ((dict(order=2), "order 2"), (dict(order=-1), "order -1"), (dict(shape=(4, 0, 4)), "every axis"),
                    (dict(target=(4, 4, -1)), "every axis"), (dict(ws=16), "workspace of 16 bytes"),
                    (dict(src_bytes=1), "uint8 with order 0"), (dict(order=0, out_bytes=1), "keeps the type")):
        assert zoom(**kw) == INVALID and msg in lib.dycon_last_error().decode(), kw
    assert lib.dycon_volume_stats(p, 1, 0, p, p, p, 4096, None) == INVALID and "at least 1 voxel" in lib.dycon_last_error().decode()
    assert lib.dycon_volume_stats(p, 1, 64, p, p, p, 8, None) == INVALID and "workspace of 8 bytes" in lib.dycon_last_error().decode()
    assert lib.dycon_normalize_apply(p, 1, 64, None, p, None) == INVALID and "null" in lib.dycon_last_error().decode()


def test_refusals_come_before_the_library(monkeypatch):
    import torch

    def touched(*a, **k):
        raise AssertionError("the library was touched")

    for name in ("load", "call", "query"):
        monkeypatch.setattr(_lib, name, touched)
    with pytest.raises(ValueError, match="order"):
        preprocessing.zoom(np.zeros((4, 4, 4), np.float32), (4, 4, 4), 3)
    with pytest.raises(ValueError, match="CUDA"):
        preprocessing.zoom(torch.zeros(4, 4, 4), (4, 4, 4), 1)
    with pytest.raises(ValueError, match="CUDA"):
        preprocessing.normalize_image(torch.zeros(4, 4, 4))
    with pytest.raises(ValueError, match="no cases"):
        device_cache.DeviceVolumeCache.from_device_cases([], [])
    with pytest.raises(ValueError, match="CUDA"):
        device_cache.DeviceVolumeCache.from_device_cases([torch.zeros(2, 2, 2)], [torch.zeros(2, 2, 2, dtype=torch.uint8)])
