"""`from dataloaders.amos import AMOSDeviceLoader, OnDeviceAugmentAMOS, amos_volume_store`: the on-device data feed for
train_inherent_consistent_unet_3D_AMOS22.py, `ForegroundIndex, OnDeviceAugmentPosNeg` for the
RandCropByPosNegLabeld loader of utils/data_utils.py, `affine_matrix` for the random rotation and zoom both feeds can add, and the
cached prefix on the device (`amos_prefix`, `amos_volume_store_from_raw`, `amos_val_cases_from_raw`, `restore_label`)
-> icl_amd.dataloaders.amos."""
from icl_amd.dataloaders.amos import (AMOSDeviceLoader, ForegroundIndex, OnDeviceAugmentAMOS, OnDeviceAugmentPosNeg,  # noqa: F401
                                      PrefixPlan, affine_matrix, amos_prefix, amos_val_cases_from_raw, amos_volume_store,
                                      amos_volume_store_from_raw, draw_amos_params, draw_posneg_params, orientation_from_affine,
                                      orientation_from_axcodes, plan_prefix, restore_label)
