"""Name mirror of the reference's code/BraTS19_DataPreprocessing.py: its public names with its parameter lists, the arithmetic on the
device (preprocessing.py, csrc/resample.hip).

    normalize_image(image)                                   numpy in, numpy out (a CUDA tensor in, a CUDA tensor out)
    find_case_directory(base_dir, case_name)                 <base>/HGG/<case>, <base>/LGG/<case> or <base>/<case>
    find_case_files(case_path, case_name)                    (t1, t1ce, t2, flair, seg) paths, None where a file is missing
    process_brats_case(base_dir, case_name, output_path)     one case -> <output_path>/<case>.h5, True on success
    get_all_available_cases(base_dir)                        sorted BraTS19* directories under HGG and LGG
    preprocess_brats2019(input_dir, output_dir, split_file_path)

The file and path logic is host code restated here; nibabel, h5py and tqdm are imported inside the functions that touch files, so
the module imports without them.  The I/O itself is "parity unpinned" like the h5 readers of dataloaders/: the libraries are not
installed where the tests run, which drive these functions with stand-ins.
"""
import os

import numpy as np
import torch

from . import preprocessing as _pre

TARGET_SHAPE = (192, 192, 64)
_MODALITIES = ("t1", "t1ce", "t2", "flair", "seg")
_LABELS = {"t1": "T1", "t1ce": "T1ce", "t2": "T2", "flair": "FLAIR", "seg": "seg"}


def normalize_image(image):
    """z-score over the voxels > 0, then min-max to [0, 1] (reference lines 8-31), computed on the device"""
    if torch.is_tensor(image):
        return _pre.normalize_image(image)
    return _pre.normalize_image(np.asarray(image)).cpu().numpy()


def find_case_directory(base_dir, case_name):
    for parts in (("HGG", case_name), ("LGG", case_name), (case_name,)):
        path = os.path.join(base_dir, *parts)
        if os.path.exists(path):
            return path
    return None


def find_case_files(case_path, case_name):
    none = (None,) * 5
    if not os.path.exists(case_path):
        return none
    volumes = [f for f in os.listdir(case_path) if f.endswith((".nii.gz", ".nii"))]
    if not volumes:
        print(f"No .nii or .nii.gz files found in {case_path}")
        return none
    found = {}
    for key in _MODALITIES:                                   # the standard names: <case>_<modality>.nii.gz, else .nii
        for ext in (".nii.gz", ".nii"):
            path = os.path.join(case_path, f"{case_name}_{key}{ext}")
            if os.path.exists(path):
                found[_LABELS[key]] = path
                break
    if len(found) < 3:                                        # other naming schemes: match by keyword, one label per file
        print(f"Standard naming not found for {case_name}. Available files:")
        for f in volumes:
            print(f"  - {f}")
        for f in volumes:
            low = f.lower()
            if "_t1." in f and "_t1c" not in low:
                label = "T1"
            elif "_t1c" in low or "t1gd" in low:
                label = "T1ce"
            elif "_t2." in f and "flair" not in low:
                label = "T2"
            elif "flair" in low:
                label = "FLAIR"
            elif "seg" in low:
                label = "seg"
            else:
                continue
            found[label] = os.path.join(case_path, f)
    return tuple(found.get(_LABELS[key]) for key in _MODALITIES)


def process_brats_case(base_dir, case_name, output_path):
    try:
        import h5py
        import nibabel as nib

        case_path = find_case_directory(base_dir, case_name)
        if case_path is None:
            print(f"Case directory not found: {case_name}")
            return False
        case_type = "HGG" if "/HGG/" in case_path else "LGG" if "/LGG/" in case_path else "Unknown"
        t1, t1ce, t2, flair, seg = find_case_files(case_path, case_name)
        if seg is None:
            print(f"No segmentation file found for {case_name}")
            return False
        for path, modality in ((t2, "T2"), (flair, "FLAIR"), (t1ce, "T1ce"), (t1, "T1")):      # the first one that exists
            if path and os.path.exists(path):
                break
        else:
            print(f"No suitable image modality found for {case_name}")
            return False
        image = nib.load(path).get_fdata()
        seg_data = nib.load(seg).get_fdata()
        if image.size == 0 or seg_data.size == 0:
            print(f"Empty data for {case_name}")
            return False
        image_dev, label_dev = _pre.preprocess_brats_volume(image, seg_data, TARGET_SHAPE)
        with h5py.File(os.path.join(output_path, f"{case_name}.h5"), "w") as h5f:
            h5f.create_dataset("image", data=image_dev.cpu().numpy(), compression="gzip")
            h5f.create_dataset("label", data=label_dev.cpu().numpy(), compression="gzip")
            h5f.attrs["modality"] = modality
            h5f.attrs["case_type"] = case_type
            h5f.attrs["original_shape"] = image.shape
            h5f.attrs["case_name"] = case_name
        print(f"{case_name} ({case_type}): {image.shape} -> {TARGET_SHAPE} ({modality})")
        return True
    except Exception as e:                                   # the reference reports and goes on to the next case
        print(f"Error processing {case_name}: {e}")
        return False


def get_all_available_cases(base_dir):
    cases = []
    for grade in ("HGG", "LGG"):
        root = os.path.join(base_dir, grade)
        if os.path.exists(root):
            here = [d for d in os.listdir(root) if d.startswith("BraTS19") and os.path.isdir(os.path.join(root, d))]
            print(f"Found {len(here)} cases in {grade}")
            cases += here
    return sorted(cases)


def preprocess_brats2019(input_dir, output_dir, split_file_path):
    if not os.path.exists(input_dir):
        print(f"Input directory not found: {input_dir}")
        return
    data_dir = os.path.join(output_dir, "data")
    os.makedirs(data_dir, exist_ok=True)
    if not os.path.exists(split_file_path):
        print(f"Split file not found: {split_file_path}")
        available = get_all_available_cases(input_dir)
        for case in available[:10]:
            print(f"  - {case}")
        if len(available) > 10:
            print(f"  ... and {len(available) - 10} more cases")
        return
    with open(split_file_path) as fh:
        wanted = [line.strip() for line in fh if line.strip()]
    available = set(get_all_available_cases(input_dir))
    todo = [c for c in wanted if c in available]
    missing = [c for c in wanted if c not in available]
    print(f"{len(wanted)} cases in the split file, {len(todo)} of them in {input_dir}, {len(missing)} missing {missing[:5]}")
    from tqdm import tqdm

    done = sum(bool(process_brats_case(input_dir, case, data_dir)) for case in tqdm(todo, desc="Processing cases"))
    print(f"Successful: {done}  Failed: {len(todo) - done}  H5 files saved to: {data_dir}")
