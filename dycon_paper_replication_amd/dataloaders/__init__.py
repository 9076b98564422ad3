"""Data path mirror; device_cache: the training set resident in HBM, batches assembled by one HIP launch."""
from .device_cache import (PLAN_DTYPE, DeviceBatchLoader, DeviceVolumeCache, apply_plan_host, assemble_batch,   # noqa: F401
                           draw_plan)
