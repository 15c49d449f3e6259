"""Loss functions of the ICL trainers with the reference's names and signatures
(/root/reference/code/utils/losses.py: DiceLoss :195-231, AuxLoss3D :254-271, PseudoSoftLoss3D :287-299,
softmax_mse_loss :68-90, softmax_dice_loss :42-59, dice_loss1 :22-30).  Every function returns a 0-dim fp32
tensor attached to autograd.

Differences from the reference that do not change results: no per-class ``.item()`` host syncs
(losses.py:229 forces nc device→host round trips per call), and the trilinear resize runs on the HIP kernel.

The rest of the reference's module — softmax_kl_loss :93-112, compute_kl_loss :334-346, entropy_loss :33-39, entropy_loss_map :62-65,
entropy_minmization :321-325, entropy_map :328-331, FocalLoss :149-183 — runs on the voxel-wise kernels (ops.softmax_kl, ops.entropy,
ops.focal_loss); dice_loss :11-19 is a torch expression like dice_loss1.

Out of scope: KD_Loss, symmetric_mse_loss, cos_sim_loss and EAMLoss (their loops index element 0 or keep only the last iterate in the
reference, and no trainer calls them), and the ``sigmoid=True`` branches.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
from torch.nn.modules.loss import CrossEntropyLoss

from .. import ops


def dice_loss1(score, target):
    """losses.py:22-30 — plain sums in the denominator."""
    target = target.float()
    smooth = 1e-5
    intersect = torch.sum(score * target)
    return 1 - (2 * intersect + smooth) / (torch.sum(score) + torch.sum(target) + smooth)


def dice_loss(score, target):
    """losses.py:11-19 — squared sums in the denominator."""
    target = target.float()
    smooth = 1e-5
    intersect = torch.sum(score * target)
    return 1 - (2 * intersect + smooth) / (torch.sum(score * score) + torch.sum(target * target) + smooth)


def softmax_dice_loss(input_logits, target_logits):
    """losses.py:42-59."""
    assert input_logits.size() == target_logits.size()
    return ops.soft_dice_loss(input_logits, target_logits)


def _mean_of(leaves):
    """Mean of a list of 0-dim loss terms in one launch (ops.combine_scalars) instead of a chain of one-element adds and a divide."""
    if len(leaves) == 1:
        return leaves[0]
    return ops.combine_scalars(leaves, [[1.0 / len(leaves)] * len(leaves)])[0]


def softmax_mse_leaves(input_logits, target_logits):
    """The per-scale terms of softmax_mse_loss (each enters the loss with weight 1 / len)."""
    return [ops.softmax_mse(a, b.detach()) for a, b in zip(input_logits, target_logits)]


def softmax_mse_loss(input_logits, target_logits, sigmoid=False):
    """losses.py:68-90: lists of per-scale maps; targets detached; mean over scales."""
    if sigmoid:
        raise NotImplementedError("the ICL trainers never pass sigmoid=True")
    return _mean_of(softmax_mse_leaves(input_logits, target_logits))


def softmax_kl_loss(input_logits, target_logits, sigmoid=False):
    """losses.py:93-112: F.kl_div(log_softmax(input, 1), softmax(target, 1), reduction='mean'), the mean over ALL elements.  The
    reference does not detach its target, whatever its docstring says: ``target_logits`` gets a gradient when it requires one."""
    assert input_logits.size() == target_logits.size()
    if sigmoid:
        raise NotImplementedError("softmax_kl_loss(sigmoid=True) is not built")
    return ops.softmax_kl(input_logits, target_logits, 1.0, 0.0, dim=1)


def softmax_kl_leaves(input_logits, target_logits):
    """Per-scale KL consistency terms against detached targets (the trainer's consistency="kl")."""
    return [ops.softmax_kl(a, b.detach()) for a, b in zip(input_logits, target_logits)]


def compute_kl_loss(p, q):
    """losses.py:334-346: lists of logits, soft-max over the last axis; per pair (mean KL(q||p) + mean KL(p||q)) / 2, then the mean
    over the list.  Gradients reach both arguments."""
    return _mean_of([ops.softmax_kl(a, b, 0.5, 0.5, dim=-1) for a, b in zip(p, q)])


def entropy_loss(p, C=2):
    """losses.py:33-39: mean over the voxels of -sum_c p log(p + 1e-6) / log C; ``p`` holds probabilities [N, C, ...]."""
    return ops.entropy(p, scale=1.0 / math.log(C), want="mean")


def entropy_loss_map(p, C=2):
    """losses.py:62-65: the [N, 1, ...] map of -sum_c p log(p + 1e-6) / log C."""
    return ops.entropy(p, scale=1.0 / math.log(C), want="map")


def entropy_minmization(p):
    """losses.py:321-325 (the reference's spelling): mean over the voxels of -sum_c p log(p + 1e-6)."""
    return ops.entropy(p, want="mean")


def entropy_map(p):
    """losses.py:328-331: the [N, 1, ...] map of -sum_c p log(p + 1e-6)."""
    return ops.entropy(p, want="map")


class FocalLoss(nn.Module):
    """losses.py:149-183.  A float ``alpha`` becomes [alpha, 1 - alpha], a list is used as given; input [N, C, ...] or [M, C], target
    integer class ids, one per voxel.  (1 - pt)^gamma is a constant of the backward pass, as in the reference (pt from ``.data``).
    A label outside [0, C) adds 0 to the value and to the gradient and still counts in the mean; the reference's gather raises on it on
    the CPU."""

    def __init__(self, gamma=2, alpha=None, size_average=True):
        super().__init__()
        self.gamma = gamma
        self.alpha = alpha
        if isinstance(alpha, (float, int)):
            self.alpha = torch.Tensor([alpha, 1 - alpha])
        if isinstance(alpha, list):
            self.alpha = torch.Tensor(alpha)
        self.size_average = size_average

    def forward(self, input, target):
        if self.alpha is not None and (self.alpha.device != input.device or self.alpha.dtype != torch.float32):
            self.alpha = self.alpha.to(device=input.device, dtype=torch.float32)      # once, as the reference's type_as
        return ops.focal_loss(input, target.long(), self.gamma, self.alpha, self.size_average)


class DiceLoss(nn.Module):
    """losses.py:195-231.  ``target`` is [B,1,...] class indices; one-hot by equality."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        assert inputs.shape[1] == self.n_classes and inputs.shape[0] == target.shape[0] \
            and inputs.shape[2:] == target.shape[2:], \
            "predict {} & target {} shape do not match".format(inputs.size(), target.size())
        return ops.dice_loss(inputs, target[:, 0], self.n_classes, softmax, weight)


def _resize(t, size):
    return ops.trilinear_resize(t.float(), size)


def _resize2d(t, size):
    return ops.bilinear_resize(t.float(), size)


class AuxLoss(nn.Module):
    """2-D twin of AuxLoss3D (losses.py:233-251): bilinear resize to ``resize``, CE + Dice(softmax=True) per map."""

    def __init__(self, n_classes, resize=(224, 224)):
        super().__init__()
        self.n_classes = n_classes
        self.ce_loss = CrossEntropyLoss()
        self.dice_loss = DiceLoss(n_classes)
        self.resize = tuple(resize)

    def leaves(self, feat_maps, labels):
        """[ce_0, dice_0, ce_1, dice_1, ...]: the loss is their sum / len(feat_maps)."""
        out = []
        for fm in feat_maps:
            out += list(ops.cross_entropy_dice_parts(_resize2d(fm, self.resize), labels.long(), self.n_classes))
        return out

    def forward(self, feat_maps, labels):
        lv = self.leaves(feat_maps, labels)
        return ops.combine_scalars(lv, [[1.0 / len(feat_maps)] * len(lv)])[0]


class PseudoSoftLoss(nn.Module):
    """2-D twin of PseudoSoftLoss3D (losses.py:273-285)."""

    def __init__(self, n_classes, resize=(224, 224)):
        super().__init__()
        self.resize = tuple(resize)

    def leaves(self, feat_maps, predicts):
        tgt = predicts.detach()
        return [softmax_dice_loss(_resize2d(fm, self.resize), tgt) for fm in feat_maps]

    def forward(self, feat_maps, predicts):
        return _mean_of(self.leaves(feat_maps, predicts))


class AuxLoss3D(nn.Module):
    """losses.py:254-271 (resize hard-coded to 96^3 there; exposed as an argument with that default)."""

    def __init__(self, n_classes, resize=(96, 96, 96)):
        super().__init__()
        self.n_classes = n_classes
        self.ce_loss = CrossEntropyLoss()
        self.dice_loss = DiceLoss(n_classes)
        self.resize = tuple(resize)

    def leaves(self, feat_maps, labels):
        """[ce_0, dice_0, ce_1, dice_1, ...] (CE + Dice(softmax=True) per map): the loss is their sum / len(feat_maps)."""
        out = []
        for fm in feat_maps:
            out += list(ops.cross_entropy_dice_parts(_resize(fm, self.resize), labels.long(), self.n_classes))
        return out

    def terms(self, feat_maps, labels):
        """The same terms as (logits, target, mode) triples for ops.fused_losses (all loss terms of a step in one launch per pass)."""
        return [(_resize(fm, self.resize), labels, 1) for fm in feat_maps]

    def forward(self, feat_maps, labels):
        lv = self.leaves(feat_maps, labels)
        return ops.combine_scalars(lv, [[1.0 / len(feat_maps)] * len(lv)])[0]


class PseudoSoftLoss3D(nn.Module):
    """losses.py:287-299: soft Dice against the detached unlabeled prediction."""

    def __init__(self, n_classes, resize=(96, 96, 96)):
        super().__init__()
        self.resize = tuple(resize)

    def leaves(self, feat_maps, predicts):
        tgt = predicts.detach()
        return [softmax_dice_loss(_resize(fm, self.resize), tgt) for fm in feat_maps]

    def terms(self, feat_maps, predicts):
        tgt = predicts.detach()
        return [(_resize(fm, self.resize), tgt, 2) for fm in feat_maps]

    def forward(self, feat_maps, predicts):
        return _mean_of(self.leaves(feat_maps, predicts))
