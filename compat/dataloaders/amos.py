"""`from dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store`: the on-device data feed for
train_inherent_consistent_unet_3D_AMOS22.py -> icl_amd.dataloaders.amos."""
from icl_amd.dataloaders.amos import (AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store, draw_amos_params)  # noqa: F401
