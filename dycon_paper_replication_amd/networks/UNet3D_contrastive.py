"""3D U-Net with projection head (the model the reference's run scripts train), on the HIP executor.

Topology and state_dict keys follow code/networks/UNet3D_contrastive.py:207-316 with feature_scale=4
(filters 16..256), InstanceNorm3d blocks (networks/utils.py:99-123), MaxPool3d(2), trilinear x2 +
concat decoder (networks/utils.py:260-276), Dropout(0.3) at the bottleneck and before the heads.
use_aspp=True puts ASPP3D(256, 256, output_stride=16) (networks/assp.py) between the bottleneck and the projection head
(UNet3D_contrastive.py:304-305), as the reference's UNet3D does by default; the package's default stays False, as in
net_factory_3d.  The ASPP exists on the HIP path only: without a visible GPU, use_aspp=True is refused at construction
(NotImplementedError), as a host-only build of the package has always refused it -- there is no CPU fallback.
"""
import torch

from ._base import HipSegNet


class UNet3D(HipSegNet):
    net_type = "unet_3D"

    def __init__(self, in_channels=1, feature_scale=4, n_classes=2, scale_factor=2, use_aspp=False, **kw):
        if feature_scale != 4:
            raise NotImplementedError("feature_scale is fixed to 4 (filters 16, 32, 64, 128, 256)")
        if use_aspp and not torch.cuda.is_available():
            raise NotImplementedError("UNet3D(use_aspp=True) runs on the MI355X only (the ASPP is a HIP path, no CPU fallback): "
                                      "no GPU is visible")
        super().__init__(in_channels=in_channels, n_classes=n_classes, scale_factor=scale_factor, has_dropout=True,
                         use_aspp=use_aspp, **kw)
