"""Name mirror of the reference's code/ISLES22_DataPreprocessing.py: its public names with its parameter lists, the arithmetic on the
device (preprocessing.py, csrc/resample.hip).

    normalize_image(image)                                                numpy in, numpy out (a CUDA tensor in, a CUDA tensor out)
    find_isles_bids_files(base_dir, case_name, modality='dwi')            (image path, mask path) of a BIDS case, None where missing
    get_case_list(base_dir)                                               sorted sub-strokecase* directories
    process_isles_bids_case(base_dir, case_name, output_path, modality='dwi')   one case -> <output_path>/case_<number>.h5
    create_split_files(cases, output_dir, train_ratio=0.8)                train.list / val.list from np.random.seed(42)
    preprocess_isles22_bids(input_dir, output_dir, modality='dwi', process_cases=None)

The reference's centre crop / pad for a zoom result that misses the target shape is not built: scipy's output shape for the factors
t / s is the target for every shape (preprocessing.zoom asserts it).  nibabel, h5py and tqdm are imported inside the functions that
touch files; the I/O is "parity unpinned" like the h5 readers of dataloaders/.
"""
import os

import numpy as np
import torch

from . import preprocessing as _pre

TARGET_SHAPE = (112, 112, 64)
_SESSION = "ses-0001"
# modality -> (folder of the session, suffix of the file name); also the order in which the others are tried
_IMAGES = {"dwi": ("dwi", "dwi"), "adc": ("dwi", "adc"), "flair": ("anat", "FLAIR")}


def normalize_image(image):
    """z-score over the voxels > 0, then min-max to [0, 1] (reference lines 10-33), computed on the device"""
    if torch.is_tensor(image):
        return _pre.normalize_image(image)
    return _pre.normalize_image(np.asarray(image)).cpu().numpy()


def _image_path(base_dir, case_name, key):
    folder, suffix = _IMAGES[key]
    return os.path.join(base_dir, case_name, _SESSION, folder, f"{case_name}_{_SESSION}_{suffix}.nii.gz")


def find_isles_bids_files(base_dir, case_name, modality='dwi'):
    asked = modality.lower()
    image_path = None
    if asked in _IMAGES and os.path.exists(_image_path(base_dir, case_name, asked)):
        image_path = _image_path(base_dir, case_name, asked)
    else:
        for key in _IMAGES:                                  # the asked-for modality is missing: the first other one that exists
            if key != asked and os.path.exists(_image_path(base_dir, case_name, key)):
                image_path = _image_path(base_dir, case_name, key)
                print(f"  Using {key.upper()} as fallback for {case_name}")
                break
    mask_path = os.path.join(base_dir, "derivatives", case_name, _SESSION, f"{case_name}_{_SESSION}_msk.nii.gz")
    return image_path, (mask_path if os.path.exists(mask_path) else None)


def get_case_list(base_dir):
    return sorted(d for d in os.listdir(base_dir) if d.startswith("sub-strokecase") and os.path.isdir(os.path.join(base_dir, d)))


def _case_number(case_name):
    return case_name.replace("sub-strokecase", "").zfill(3)


def process_isles_bids_case(base_dir, case_name, output_path, modality='dwi'):
    try:
        import h5py
        import nibabel as nib

        image_path, mask_path = find_isles_bids_files(base_dir, case_name, modality)
        if image_path is None:
            print(f"No suitable image modality found for {case_name}")
            return False
        if mask_path is None:
            print(f"No mask file found for {case_name}")
            return False
        image = nib.load(image_path).get_fdata()
        mask = nib.load(mask_path).get_fdata()
        if image.size == 0 or mask.size == 0:
            print(f"Empty data for {case_name}")
            return False
        image_dev, mask_dev = _pre.preprocess_isles_volume(image, mask, TARGET_SHAPE)
        number = _case_number(case_name)
        used = os.path.basename(image_path).split("_")[-1].replace(".nii.gz", "")
        with h5py.File(os.path.join(output_path, f"case_{number}.h5"), "w") as h5f:
            h5f.create_dataset("image", data=image_dev.cpu().numpy().astype(np.float64), compression="gzip")      # stored as float64
            h5f.create_dataset("mask", data=mask_dev.cpu().numpy().astype(np.float64), compression="gzip")
            h5f.attrs["original_shape"] = image.shape
            h5f.attrs["case_name"] = case_name
            h5f.attrs["case_number"] = number
            h5f.attrs["modality"] = used
            h5f.attrs["image_file"] = os.path.basename(image_path)
            h5f.attrs["mask_file"] = os.path.basename(mask_path)
        print(f"{case_name}: {image.shape} -> {TARGET_SHAPE} ({used})")
        return True
    except Exception as e:                                   # the reference reports and goes on to the next case
        print(f"Error processing {case_name}: {e}")
        return False


def create_split_files(cases, output_dir, train_ratio=0.8):
    """train.list / val.list (one `case_<number>` per line) from a permutation drawn after np.random.seed(42); -> (train, val) names"""
    np.random.seed(42)
    order = np.random.permutation(len(cases))
    n_train = int(len(cases) * train_ratio)
    split = {"train": [cases[i] for i in order[:n_train]], "val": [cases[i] for i in order[n_train:]]}
    for name, members in split.items():
        with open(os.path.join(output_dir, f"{name}.list"), "w") as fh:
            fh.writelines(f"case_{_case_number(c)}\n" for c in members)
    print(f"{len(cases)} cases: {len(split['train'])} -> train.list, {len(split['val'])} -> val.list in {output_dir}")
    return split["train"], split["val"]


def preprocess_isles22_bids(input_dir, output_dir, modality='dwi', process_cases=None):
    os.makedirs(output_dir, exist_ok=True)
    cases = get_case_list(input_dir)
    if not cases:
        print("No cases found! Check your input directory path.")
        return
    if process_cases is None:
        create_split_files(cases, output_dir)
    else:
        cases = [c for c in cases if c in process_cases]
    from tqdm import tqdm

    done = sum(bool(process_isles_bids_case(input_dir, c, output_dir, modality)) for c in tqdm(cases, desc="Processing ISLES22 cases"))
    print(f"Successful: {done}  Failed: {len(cases) - done}  H5 files saved to: {output_dir}  (primary modality {modality.upper()})")
