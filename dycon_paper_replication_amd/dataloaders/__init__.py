"""Data path mirror; device_cache: the training set resident in HBM, batches assembled by one HIP launch;
device_augment: RandomRot, CreateOnehotLabel and RandomNoise on that path; device_warp: affine / elastic warps with interpolation,
Gaussian blur and gain / bias / gamma on that path (not in the reference)."""
from .device_augment import (ROT_PLAN_DTYPE, apply_rot_plan_host, assemble_batch_rot, draw_plan_rot, rotate_nearest,   # noqa: F401
                             rotation_of)
from .device_cache import (PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, apply_plan_host, assemble_batch,   # noqa: F401
                           draw_plan)
from .device_warp import (WARP_PLAN_DTYPE, Intensity, Warp, affine_of, apply_warp_plan_host, assemble_batch_warp,   # noqa: F401
                          draw_plan_warp, elastic_field, intensity_augment, intensity_host, warp_volume, warp_volume_host)
