"""`from dataloaders.dataset import BaseDataSets, RandomGenerator, TwoStreamBatchSampler`
(train_inherent_consistent_unet_2D.py:17, train_inherent_consistent_swinunet_2D.py:17) -> icl_amd.dataloaders.dataset."""
from icl_amd.dataloaders.dataset import (BaseDataSets, DeviceSliceStore, OnDeviceAugment2D, RandomGenerator,  # noqa: F401
                                         TwoStreamBatchSampler, draw_generator, random_rot_flip, random_rotate)
