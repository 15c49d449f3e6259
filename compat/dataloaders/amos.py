"""`from dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store`: the on-device data feed for
train_inherent_consistent_unet_3D_AMOS22.py, and `ForegroundIndex, OnDeviceAugmentPosNeg` for the
RandCropByPosNegLabeld loader of utils/data_utils.py -> icl_amd.dataloaders.amos."""
from icl_amd.dataloaders.amos import (AMOSDeviceLoader, ForegroundIndex, OnDeviceAugmentAMOS, OnDeviceAugmentPosNeg,  # noqa: F401
                                      amos_volume_store, draw_amos_params, draw_posneg_params)
