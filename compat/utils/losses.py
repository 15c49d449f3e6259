"""`from utils import losses` (train_inherent_consistent_unet_3D_BraTS.py:22) -> icl_amd.utils.losses."""
from icl_amd.utils.losses import *  # noqa: F401,F403
from icl_amd.utils.losses import (AuxLoss, AuxLoss3D, DiceLoss, FocalLoss, PseudoSoftLoss, PseudoSoftLoss3D, compute_kl_loss,  # noqa: F401
                                  dice_loss, dice_loss1, entropy_loss, entropy_loss_map, entropy_map, entropy_minmization,
                                  softmax_dice_loss, softmax_kl_loss, softmax_mse_loss)
