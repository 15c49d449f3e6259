"""`from dataloaders.intensity import IntensityAugment, draw_intensity_params`: the intensity stage of the 3-D device feed (Gaussian
noise, blur, simulated low resolution, contrast, gamma), handed to `OnDeviceAugment`, `OnDeviceAugmentAMOS` or
`OnDeviceAugmentPosNeg` as `intensity=` -> icl_amd.dataloaders.intensity."""
from icl_amd.dataloaders.intensity import (IntensityAugment, blur_radius, blur_weights, draw_intensity_params,  # noqa: F401
                                           lowres_extents)
