"""csrc/resample.hip and preprocessing.py on the GPU: order-0 zoom against the restatement and scipy bit for bit; order-1 zoom against
the restatement bit for bit (fp64 and fp32 outputs: an FMA contraction or another tap order would show) and against scipy within the
CPU-measured bound; the statistics against their restatement (bit for bit in the kernels' order of additions, within the measured
bound of numpy's fp64) and run to run; normalise-on-load against the numpy fp32 expressions; the pipelines against the reference's
recorded outputs; DeviceVolumeCache.from_device_cases against the host-built cache; the library's refusals.

Tolerances (measured on the CPU by tests/test_preprocess_cpu.py, which asserts them; doubled here as the issue of record sets):
  order 1 vs scipy          2 * 6.67e-16 (fp64 output), 2 * 1.20e-7 (fp32 output), absolute, the same unit-normal volumes
  images vs recorded        2 * 7.27e-8 absolute on [0, 1] (the reference's float32 pairwise mean and std are not reproducible in bits)
  mean / std vs numpy fp64  2 * 2^-52 relative (measured distance 0: the bound is the format's resolution)
"""
import ctypes
import functools
import sys
import types

import numpy as np
import pytest
import torch
from scipy import ndimage

import device_cache_ref as DR
import resample_ref as R
from conftest import load_golden
from test_preprocess_cpu import INVALID, NORM_REF_F64, STATS_ORDER_REL, ZOOM1_SCIPY_F32, ZOOM1_SCIPY_F64, ZOOM_SEEDS

from dycon_paper_replication_amd import BraTS19_DataPreprocessing as BR
from dycon_paper_replication_amd import ISLES22_DataPreprocessing as IS
from dycon_paper_replication_amd import _lib
from dycon_paper_replication_amd import preprocessing as P
from dycon_paper_replication_amd.dataloaders import DeviceVolumeCache, assemble_batch, draw_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

RECORD = np.dtype([("apply_z", "<i4"), ("mean32", "<f4"), ("std32", "<f4"), ("apply_mm", "<i4"), ("lo32", "<f4"), ("hi32", "<f4")])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _records(stats):
    """the records of a VolumeStats as a list of norm_record-style tuples"""
    return [tuple(r) for r in stats.record.cpu().numpy().view(RECORD).reshape(-1)]


def _same_bits(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(f"u{got.itemsize}"), want.view(f"u{want.itemsize}"))


@functools.lru_cache(maxsize=None)
def _batch(si, B):
    return np.stack([R.zoom_input(si, seed) for seed in ZOOM_SEEDS[:B]])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("si,so", R.SHAPE_PAIRS)
def test_zoom_order0(si, so, B):
    x = _batch(si, B)
    for a in (x.astype(np.float32), (40 * x).astype(np.uint8)):
        got = P.zoom(_dev(a), so, 0)
        assert got.is_cuda and tuple(got.shape) == (B,) + so
        assert _same_bits(got, R.zoom(a, so, 0))
        for b in range(B):
            assert np.array_equal(got[b].cpu().numpy(), ndimage.zoom(a[b], [t / s for t, s in zip(so, si)], order=0))
    assert _same_bits(P.zoom(x[0].astype(np.float32), so, 0), R.zoom(x[0].astype(np.float32), so, 0))       # a host array, no batch axis


def test_zoom_order0_2d_bool_and_binarize():
    x = R.zoom_input((7, 9)).astype(np.float32)
    for a in (x, (40 * x).astype(np.uint8)):
        got = P.zoom(a, (12, 5), 0)
        assert tuple(got.shape) == (12, 5) and _same_bits(got, ndimage.zoom(a, (12 / 7, 5 / 9), order=0))
    m = x > 0.3
    assert _same_bits(P.zoom(_dev(m), (12, 5), 0), ndimage.zoom(m.astype(np.uint8), (12 / 7, 5 / 9), order=0))
    v = R.zoom_input((13, 9, 11)).astype(np.float32)
    for src, thr in ((v, 0.25), ((3 * np.abs(v)).astype(np.uint8), 0.0), ((3 * np.abs(v)).astype(np.uint8), 1.0)):
        got = P.zoom(_dev(src), (7, 6, 8), 0, binarize=thr)
        assert _same_bits(got, R.zoom((src > thr).astype(np.uint8), (7, 6, 8), 0))


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("si,so", R.SHAPE_PAIRS)
def test_zoom_order1(si, so, B):
    x = _batch(si, B).astype(np.float32)
    xd = _dev(x)
    got64, got32 = P.zoom(xd, so, 1, out_dtype=torch.float64), P.zoom(xd, so, 1)
    assert _same_bits(got64, R.zoom(x, so, 1, out_dtype=np.float64))
    assert _same_bits(got32, R.zoom(x, so, 1))
    f = [t / s for t, s in zip(so, si)]
    for b in range(B):
        d64 = np.abs(got64[b].cpu().numpy() - ndimage.zoom(x[b].astype(np.float64), f, order=1)).max()
        d32 = np.abs(got32[b].cpu().numpy() - ndimage.zoom(x[b], f, order=1)).max()
        print(f"order 1 {si} -> {so} sample {b}: |device - scipy| fp64 {d64:.3e} fp32 {d32:.3e}")
        assert d64 <= 2 * ZOOM1_SCIPY_F64 and d32 <= 2 * ZOOM1_SCIPY_F32


def _raw_zoom(src, so, order, out, norm=None):
    """dycon_zoom straight into `out`, a view that may start at any element"""
    B, X, Y, Z = src.shape
    ws = torch.empty(int(_lib.load().dycon_zoom_workspace(order, *so)), dtype=torch.uint8, device=DEV)
    _lib.call("dycon_zoom", src.data_ptr(), src.element_size(), B, X, Y, Z, *so, order, None if norm is None else norm.data_ptr(), 0, 0.0,
              out.data_ptr(), out.element_size(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("so", [(11, 4, 16), (9, 5, 8)])
def test_zoom_unaligned_output_takes_the_element_stores(so):
    """Zo % 4 == 0 and the output one element past a 16-byte (uint8: 4-byte) boundary: the same bits, nothing outside the output"""
    si = (4, 11, 6)
    x = _batch(si, 2)
    n = 2 * int(np.prod(so))
    for a, order, dtype in ((x.astype(np.float32), 0, torch.float32), ((40 * x).astype(np.uint8), 0, torch.uint8),
                            (x.astype(np.float32), 1, torch.float32), (x.astype(np.float32), 1, torch.float64)):
        buf = torch.full((n + 8,), 77, dtype=dtype, device=DEV)
        assert buf.data_ptr() % 16 == 0
        _raw_zoom(_dev(a), so, order, buf[1:])
        want = R.zoom(a, so, order, out_dtype=np.float64 if dtype == torch.float64 else None)
        assert _same_bits(buf[1:n + 1].reshape((2,) + so), want)
        assert (buf[0] == 77).item() and (buf[n + 1:] == 77).all().item()
        _raw_zoom(_dev(a), so, order, buf)                                                   # aligned: the vector stores
        assert _same_bits(buf[:n].reshape((2,) + so), want) and (buf[n + 1:] == 77).all().item()


@functools.lru_cache(maxsize=None)
def _stats_case(name):
    x = R.stats_volumes()[name]
    return x, R.volume_stats(x), R.device_stats(x)


@pytest.mark.parametrize("name", list(R.stats_volumes()))
def test_volume_stats(name):
    x, ref, order = _stats_case(name)
    st = P.volume_stats(_dev(x))
    again = P.volume_stats(x)                                                                # the host array, uploaded
    assert torch.equal(st.raw, again.raw) and torch.equal(st.record, again.record)            # run to run: the same bits
    assert int(st.n_pos[0]) == ref["n_pos"] and int(st.any_nonpos[0]) == ref["any_nonpos"]
    for f in ("min_pos", "max_pos", "min_all", "max_all"):
        assert getattr(st, f)[0].item() == float(ref[f]), f
    mean, std = st.mean[0].item(), st.std[0].item()
    print(f"{name}: mean {mean!r} (numpy {ref['mean']!r}) std {std!r} (numpy {ref['std']!r})")
    assert (mean, std) == (order["mean"], order["std"])                                      # the kernels' order, restated
    assert abs(mean - ref["mean"]) <= 2 * STATS_ORDER_REL * abs(ref["mean"])
    assert abs(std - ref["std"]) <= 2 * STATS_ORDER_REL * abs(ref["std"])
    (got,) = _records(st)
    want = R.norm_record(order)
    assert got[0] == want[0] and got[3] == want[3] and _same_bits(np.array(got, np.float32), np.array(want, np.float32))


def test_volume_stats_batch_and_unaligned_input():
    """every sample has its own statistics; a sample that starts off a 16-byte boundary (odd voxel count) gives the same bits"""
    x = np.stack([R.stats_volumes()["normal17x9x33"], R.stats_volumes()["equal"], -R.stats_volumes()["normal17x9x33"]])
    st = P.volume_stats(_dev(x))
    for b in range(3):
        one = P.volume_stats(_dev(x[b]))
        assert torch.equal(st.raw[b], one.raw[0]) and torch.equal(st.record[b], one.record[0])
    assert _records(st)[1][0] == 0 and _records(st)[0][0] == 1
    v = R.stats_volumes()["normal40x40x30"]                                                  # V % 4 == 0: 16-byte loads when aligned
    buf = torch.zeros(v.size + 4, dtype=torch.float32, device=DEV)
    buf[1:v.size + 1] = _dev(v).reshape(-1)
    shifted, aligned = P.volume_stats(buf[1:v.size + 1].reshape(v.shape)), P.volume_stats(_dev(v))
    assert buf.data_ptr() % 16 == 0 and torch.equal(shifted.raw, aligned.raw) and torch.equal(shifted.record, aligned.record)
    assert torch.equal(P.normalize_image(buf[1:v.size + 1].reshape(v.shape)), P.normalize_image(_dev(v)))


def _apply_np(x, recs):
    return np.stack([R.normalize_apply(v, r) for v, r in zip(x, recs)])


@pytest.mark.parametrize("name", ["normal5x7x4", "normal17x9x33", "brain", "zero", "nopos", "one", "equal"])
def test_normalize_image_is_the_fp32_expressions(name):
    x = R.stats_volumes()[name]
    st = P.volume_stats(_dev(x))
    (rec,) = _records(st)
    assert _same_bits(P.normalize_image(_dev(x)), R.normalize_apply(x, rec))
    so = tuple(max(1, (3 * n) // 4) for n in x.shape)
    assert _same_bits(P.zoom(_dev(x), so, 1, norm=st), R.zoom(x, so, 1, norm=rec))
    assert _same_bits(P.zoom(_dev(x), so, 1, norm=st.record, out_dtype=torch.float64), R.zoom(x, so, 1, norm=rec, out_dtype=np.float64))
    assert _same_bits(P.zoom(_dev(x), so, 0, norm=st), R.zoom(x, so, 0, norm=rec))


def test_normalize_on_load_batch():
    x = np.stack([R.stats_volumes()[k] for k in ("normal17x9x33", "equal")])
    st = P.volume_stats(_dev(x))
    recs = _records(st)
    assert _same_bits(P.normalize_image(x), _apply_np(x, recs))
    want = np.stack([R.zoom(v, (12, 9, 16), 1, norm=r) for v, r in zip(x, recs)])
    assert _same_bits(P.zoom(x, (12, 9, 16), 1, norm=st), want)


@pytest.mark.parametrize("name", ["zero", "nopos", "const", "flat"])
def test_edge_rules_return_what_the_reference_returns(name):
    g = load_golden("preprocess")
    got = P.normalize_image(g[f"vol.{name}.image"])                                           # float64 in, as get_fdata hands it over
    assert _same_bits(got, g[f"norm.{name}"])
    assert _same_bits(torch.from_numpy(BR.normalize_image(g[f"vol.{name}.image"])), g[f"norm.{name}"])
    assert torch.equal(IS.normalize_image(_dev(g[f"vol.{name}.image"])), got)


@pytest.mark.parametrize("name", list(R.golden_volumes()))
def test_pipelines_against_the_recorded_reference(name):
    g = load_golden("preprocess")
    image, seg = g[f"vol.{name}.image"], g[f"vol.{name}.seg"]
    d = np.abs(P.normalize_image(image).cpu().numpy().astype(np.float64) - g[f"norm.{name}"]).max()
    print(f"{name}: normalize_image |device - recorded| {d:.3e}")
    assert d <= 2 * NORM_REF_F64
    for fn, key, lab, args in ((P.preprocess_brats_volume, "brats", "label", (_dev(image), _dev(seg))),
                               (P.preprocess_isles_volume, "isles", "mask", (image, seg))):
        img, label = fn(*args, target_shape=R.GOLDEN_TARGET)
        assert img.is_cuda and img.dtype == torch.float32 and label.dtype == torch.uint8 and tuple(img.shape) == R.GOLDEN_TARGET
        assert np.array_equal(label.cpu().numpy(), g[f"{key}.{name}.{lab}"])
        d = np.abs(img.cpu().numpy().astype(np.float64) - g[f"{key}.{name}.image"]).max()
        print(f"{name}: {key} image |device - recorded| {d:.3e}")
        assert d <= 2 * NORM_REF_F64
        want_i, want_l = R.preprocess(image, seg, R.GOLDEN_TARGET, 0.0 if key == "brats" else 0.5)
        (rec,) = _records(P.volume_stats(image))
        assert _same_bits(img, R.zoom(image.astype(np.float32), R.GOLDEN_TARGET, 1, norm=rec)) and _same_bits(label, want_l)


def test_pipeline_batch_and_integer_labels():
    g = load_golden("preprocess")
    names = ("mri", "const")
    image = np.stack([g[f"vol.{n}.image"] for n in names])
    seg = np.stack([g[f"vol.{n}.seg"] for n in names]).astype(np.int64)
    img, label = P.preprocess_brats_volume(image, _dev(seg), target_shape=R.GOLDEN_TARGET)
    for b, n in enumerate(names):
        one_i, one_l = P.preprocess_brats_volume(image[b], seg[b].astype(np.uint8), target_shape=R.GOLDEN_TARGET)
        assert torch.equal(img[b], one_i) and torch.equal(label[b], one_l)
        assert np.array_equal(label[b].cpu().numpy(), g[f"brats.{n}.label"])


def test_case_functions_end_to_end(tmp_path, monkeypatch):
    """process_brats_case / process_isles_bids_case over a tree of empty files with stand-ins for nibabel and h5py, as the fixture's
    maker drives the reference's: the datasets written are the recorded ones at the functions' own target shapes"""
    arrays, written = {}, []

    class Image:
        def __init__(self, path):
            self.path = path

        def get_fdata(self):
            return arrays[self.path.rsplit("/", 1)[-1]]

    class File:
        def __init__(self, path, mode):
            self.path, self.datasets, self.attrs = path, {}, {}

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            written.append(self)

        def create_dataset(self, name, data, compression=None):
            self.datasets[name] = np.array(data)

    nib, h5py = types.ModuleType("nibabel"), types.ModuleType("h5py")
    nib.load, h5py.File = Image, File
    monkeypatch.setitem(sys.modules, "nibabel", nib)
    monkeypatch.setitem(sys.modules, "h5py", h5py)
    monkeypatch.setattr(BR, "TARGET_SHAPE", R.GOLDEN_TARGET)
    monkeypatch.setattr(IS, "TARGET_SHAPE", R.GOLDEN_TARGET)
    g = load_golden("preprocess")

    def touch(*parts):
        p = tmp_path.joinpath(*parts)
        p.parent.mkdir(parents=True, exist_ok=True)
        p.write_bytes(b"")

    case = "BraTS19_TEST_0_1"
    arrays[f"{case}_t2.nii.gz"], arrays[f"{case}_seg.nii.gz"] = g["vol.mri.image"], g["vol.mri.seg"]
    for kind in ("t2", "seg", "flair"):
        touch("b", "HGG", case, f"{case}_{kind}.nii.gz")
    assert BR.process_brats_case(str(tmp_path / "b"), case, str(tmp_path)) is True
    f = written.pop()
    assert f.path == str(tmp_path / f"{case}.h5") and f.datasets["image"].dtype == np.float32 and f.datasets["label"].dtype == np.uint8
    assert np.array_equal(f.datasets["label"], g["brats.mri.label"])
    assert np.abs(f.datasets["image"].astype(np.float64) - g["brats.mri.image"]).max() <= 2 * NORM_REF_F64
    assert sorted(f"{k}={v}" for k, v in f.attrs.items()) == g["brats.attrs"].tolist()

    case = "sub-strokecase0001"
    arrays[f"{case}_ses-0001_dwi.nii.gz"], arrays[f"{case}_ses-0001_msk.nii.gz"] = g["vol.mri.image"], g["vol.mri.seg"]
    touch("i", case, "ses-0001", "dwi", f"{case}_ses-0001_dwi.nii.gz")
    touch("i", "derivatives", case, "ses-0001", f"{case}_ses-0001_msk.nii.gz")
    assert IS.process_isles_bids_case(str(tmp_path / "i"), case, str(tmp_path)) is True
    f = written.pop()
    assert f.path == str(tmp_path / "case_0001.h5") and f.datasets["image"].dtype == np.float64 == f.datasets["mask"].dtype
    assert np.array_equal(f.datasets["mask"], g["isles.mri.mask"])
    assert np.abs(f.datasets["image"] - g["isles.mri.image"]).max() <= 2 * NORM_REF_F64
    assert sorted(f"{k}={v}" for k, v in f.attrs.items()) == g["isles.attrs"].tolist()


def test_from_device_cases_equals_the_host_built_cache():
    cases = DR.make_cases([(13, 11, 9), (20, 17, 16), (6, 11, 9)], 21, image_dtype=np.float64)
    host = DeviceVolumeCache(cases, device=DEV)
    dev = DeviceVolumeCache.from_device_cases([_dev(c["image"]) for c in cases], [_dev(c["label"]) for c in cases])
    assert torch.equal(dev.images, host.images) and torch.equal(dev.labels, host.labels)
    assert dev.shapes == host.shapes and dev.nbytes == host.nbytes and len(dev) == len(host) and dev.device == host.device
    assert np.array_equal(dev._img_off, host._img_off) and np.array_equal(dev._lab_off, host._lab_off)
    assert np.array_equal(dev._shape_arr, host._shape_arr) and dev._shape_arr.dtype == host._shape_arr.dtype
    for label_dtype in (torch.int64, torch.bool, torch.float64):                             # converted on the device
        other = DeviceVolumeCache.from_device_cases([_dev(c["image"]).float() for c in cases],
                                                    [_dev(c["label"]).to(label_dtype) if label_dtype != torch.bool
                                                     else _dev(c["label"]) > 0 for c in cases])
        want = host.labels if label_dtype != torch.bool else (host.labels > 0).to(torch.uint8)
        assert torch.equal(other.labels, want) and torch.equal(other.images, host.images)
    np.random.seed(3)
    plan = draw_plan(host.shapes, [0, 1, 2, 1, 0], (8, 8, 6))
    a, b = assemble_batch(host, plan), assemble_batch(dev, plan)
    assert torch.equal(a["image"], b["image"]) and torch.equal(a["label"], b["label"])
    with pytest.raises(ValueError, match="0..255"):
        DeviceVolumeCache.from_device_cases([_dev(cases[0]["image"])], [_dev(cases[0]["label"]).float() + 0.5])
    with pytest.raises(ValueError, match="shape"):
        DeviceVolumeCache.from_device_cases([_dev(cases[0]["image"])], [_dev(cases[1]["label"])])
    with pytest.raises(ValueError, match="max_bytes"):
        DeviceVolumeCache.from_device_cases([_dev(cases[0]["image"])], [_dev(cases[0]["label"])], max_bytes=100)


def test_preprocessed_cases_go_into_the_cache():
    g = load_golden("preprocess")
    outs = [P.preprocess_brats_volume(g[f"vol.{n}.image"], g[f"vol.{n}.seg"], target_shape=R.GOLDEN_TARGET) for n in ("mri", "const")]
    cache = DeviceVolumeCache.from_device_cases([o[0] for o in outs], [o[1] for o in outs])
    for n, (img, lab) in enumerate(outs):
        hi, hl = cache.host_case(n)
        assert np.array_equal(hi, img.cpu().numpy()) and np.array_equal(hl, lab.cpu().numpy())


def test_library_rejects_before_any_launch():
    lib = _lib.load()
    x = torch.zeros(4 * 4 * 4, dtype=torch.float32, device=DEV)
    out = torch.full((4 * 4 * 4,), 5.0, dtype=torch.float32, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def zoom(order=1, shape=(4, 4, 4), target=(4, 4, 4), ws_bytes=4096):
        return lib.dycon_zoom(x.data_ptr(), 4, 1, *shape, *target, order, None, 0, 0.0, out.data_ptr(), 4, ws.data_ptr(), ws_bytes, s)

    for kw, msg in ((dict(order=2), "order 2"), (dict(order=-1), "order -1"), (dict(shape=(4, 0, 4)), "every axis"),
                    (dict(target=(4, -4, 4)), "every axis"), (dict(ws_bytes=lib.dycon_zoom_workspace(1, 4, 4, 4) - 1), "workspace")):
        assert zoom(**kw) == INVALID and msg in lib.dycon_last_error().decode(), kw
    assert lib.dycon_volume_stats(x.data_ptr(), 1, 64, out.data_ptr(), None, ws.data_ptr(), lib.dycon_volume_stats_workspace(1, 64) - 1,
                                  s) == INVALID
    assert "workspace" in lib.dycon_last_error().decode()
    torch.cuda.synchronize()
    assert (out == 5.0).all().item() and not ws.any().item()                                 # nothing ran
    assert zoom() == 0
    torch.cuda.synchronize()
    assert not out.any().item()
    with pytest.raises(ValueError, match="positive"):
        P.zoom(x.reshape(4, 4, 4), (4, 4, 0), 1)
