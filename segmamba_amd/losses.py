"""The reference's nnU-Net training loss (light_training/loss/): Dice, cross entropy and top-k cross entropy under the reference's names.

  * `SoftDiceLoss`, `MemoryEfficientSoftDiceLoss` (dice.py:9-116), `RobustCrossEntropyLoss`, `TopKLoss` (robust_ce_loss.py:6-32),
    `DC_and_CE_loss`, `DC_and_topk_loss` (compound_losses.py:8-57, 103-151), `DeepSupervisionWrapper` (deepsupervision.py:5-36) and
    `softmax_helper_dim1` (helpers.py), with the reference's constructor signatures;
  * both Dice classes and the CE term of `DC_and_CE_loss` are built on five sums, `dice_ce_sums`: per (b, c) I = sum m p_c [y = c],
    P = sum m p_c, G = sum m [y = c] and, per b, the cross-entropy sum and the number of valid voxels.  SoftDiceLoss' tp, fp, fn are
    I, P - I, G - I; what follows the sums (batch_dice, do_bg, smooth, clip_tp, the clip of the denominator, the mean, the weights) is
    arithmetic on (B, C) tensors;
  * the sums are computed in ATen for CPU tensors only.  The library has no kernel for them, and no ATen fall-back on the device:
    everything that needs the sums refuses device tensors with NotImplementedError;
  * on the device run `RobustCrossEntropyLoss` (on `train_ops.cross_entropy`), `TopKLoss` (on `train_ops.topk_cross_entropy`: the
    per-voxel map, an exact radix selection, a per-voxel backward - csrc/topk_ce.hip) and `DC_and_topk_loss` with `weight_dice=0`,
    which never asks for the sums.

Stated deviations from the reference: sum_gt is an integer count for both Dice classes; a batch whose voxels are all ignored gives 0
for the CE term (the reference's `num_fg > 0` rule; the top-k term needs no rule: its map is all zeros); a voxel the CE term of
`DC_and_CE_loss` ignores is left out of the Dice term too; a label outside [0, classes) that is not ignored gives NaN instead of an
indexing error; `TopKLoss` raises ValueError where k selects no voxel (the reference returns the NaN of an empty mean), and among
voxels tied with the k-th largest loss each gets an equal share of the gradient where `torch.topk` picks some of them (same value).
Not here: DC_and_BCE_loss, AutoDeepSupervision, class weights, label smoothing, one-hot targets, double backward.
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
from torch import nn

from . import train_ops


def softmax_helper_dim1(x: torch.Tensor) -> torch.Tensor:
    return torch.softmax(x, 1)


# ---------------------------------------------------------------------------------------------------------
# the five sums
# ---------------------------------------------------------------------------------------------------------
def _labels_of(x: torch.Tensor, target: torch.Tensor, what: str) -> torch.Tensor:
    """(B, 1, *spatial) or (B, *spatial) target -> (B, *spatial) as int64 / int16 / uint8 / float32"""
    if target.dim() == x.dim():
        if tuple(target.shape) == tuple(x.shape) and x.shape[1] != 1:
            raise NotImplementedError(f"{what}: one-hot targets (target shape == logits shape) are not supported; pass a label map "
                                      "of shape (B, 1, ...) or (B, ...)")
        if target.shape[1] != 1:
            raise ValueError(f"{what}: target must be (B, 1, *spatial) or (B, *spatial), got {tuple(target.shape)} for {tuple(x.shape)}")
        target = target[:, 0]
    if tuple(target.shape) != (x.shape[0],) + tuple(x.shape[2:]):
        raise ValueError(f"{what}: target {tuple(target.shape)} does not match logits {tuple(x.shape)}")
    if target.dtype in (torch.int64, torch.int16, torch.uint8, torch.float32):
        return target
    return target.to(torch.float32 if target.is_floating_point() else torch.int64)


def _mask_of(x: torch.Tensor, loss_mask: Optional[torch.Tensor], what: str) -> Optional[torch.Tensor]:
    """bool / uint8 / 0-1 float (B, 1, *spatial) or (B, *spatial) -> uint8 (B, *spatial)"""
    if loss_mask is None:
        return None
    if loss_mask.dim() == x.dim():
        if loss_mask.shape[1] != 1:
            raise ValueError(f"{what}: loss_mask must be (B, 1, *spatial), got {tuple(loss_mask.shape)}")
        loss_mask = loss_mask[:, 0]
    if tuple(loss_mask.shape) != (x.shape[0],) + tuple(x.shape[2:]):
        raise ValueError(f"{what}: loss_mask {tuple(loss_mask.shape)} does not match logits {tuple(x.shape)}")
    if loss_mask.dtype == torch.uint8:
        return loss_mask
    if loss_mask.dtype == torch.bool:
        return loss_mask.contiguous().view(torch.uint8)
    return (loss_mask != 0).contiguous().view(torch.uint8)


def _sums_aten(x, labels, mask, ignore_label, nonlin):
    """the five sums in ATen (CPU tensors): -> (I, P, G, ce_sum or None, count); ce_sum only under the softmax"""
    B, C = x.shape[:2]
    xf = x.float().reshape(B, C, -1)
    lf = labels.reshape(B, -1)
    if lf.is_floating_point():                                # a float label that is no integer is a wrong label, never ignored
        whole = lf == lf.floor()
        y = torch.where(whole, lf, torch.full_like(lf, -1)).long()
    else:
        whole, y = torch.ones_like(lf, dtype=torch.bool), lf.long()
    valid = torch.ones_like(y, dtype=torch.bool)
    if ignore_label is not None:
        valid = valid & ~(whole & (y == int(ignore_label)))
    if mask is not None:
        valid = valid & (mask.reshape(B, -1) != 0)
    oob = valid & ((y < 0) | (y >= C) | ~whole)
    onehot = (y.unsqueeze(1) == torch.arange(C, device=x.device).view(1, C, 1)) & valid.unsqueeze(1)
    m = valid.unsqueeze(1).to(xf.dtype)
    p = xf if nonlin is None else nonlin(xf)
    poison = torch.where(oob.any(1), float("nan"), 0.0).to(xf.dtype)         # a wrong label stays loud, as in segm_cross_entropy
    intersect = (p * onehot).sum(2) + poison[:, None]
    sum_pred = (p * m).sum(2) + poison[:, None]
    sum_gt = onehot.sum(2)
    ce_sum = None
    if nonlin is softmax_helper_dim1:
        x_y = torch.gather(xf, 1, y.clamp(0, C - 1).unsqueeze(1))[:, 0]
        ce_sum = ((torch.logsumexp(xf, 1) - x_y) * valid).sum(1) + poison
    return intersect, sum_pred, sum_gt, ce_sum, valid.sum(1)


def dice_ce_sums(x: torch.Tensor, target: torch.Tensor, loss_mask: Optional[torch.Tensor] = None, ignore_label: Optional[int] = None,
                 apply_nonlin: Optional[Callable] = softmax_helper_dim1, _what: str = "dice_ce_sums"):
    """-> (intersect (B, C), sum_pred (B, C), sum_gt (B, C) integer, ce_sum (B), count (B)) of softmax(x) against the label map
    `target`; differentiable in x through intersect, sum_pred and ce_sum.  CPU tensors only (see the module docstring)."""
    from . import lib as L
    labels = _labels_of(x, target, _what)
    mask = _mask_of(x, loss_mask, _what)
    if not L.on_device(x):
        return _sums_aten(x, labels, mask, ignore_label, apply_nonlin)
    raise NotImplementedError(f"{_what}: the library has no kernel for the Dice sums and no ATen fall-back on the device - use CPU "
                              "tensors, or train_ops.cross_entropy / RobustCrossEntropyLoss, which run on the library's kernel")


# ---------------------------------------------------------------------------------------------------------
# ddp=True, batch_dice=True: the sums over all ranks
# ---------------------------------------------------------------------------------------------------------
class _SumOverRanks(torch.autograd.Function):
    """all-reduce (sum) whose backward sums the incoming gradient over the ranks: the reference's AllGatherGrad.apply(t).sum(0)"""

    @staticmethod
    def forward(ctx, t):
        import torch.distributed as dist
        out = t.clone()
        dist.all_reduce(out)
        return out

    @staticmethod
    def backward(ctx, g):
        import torch.distributed as dist
        g = g.clone()
        dist.all_reduce(g)
        return g


def _sum_over_ranks(t: torch.Tensor) -> torch.Tensor:
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return t
    return _SumOverRanks.apply(t)


# ---------------------------------------------------------------------------------------------------------
# the reference's classes
# ---------------------------------------------------------------------------------------------------------
class _DiceBase(nn.Module):
    def __init__(self, apply_nonlin, batch_dice, do_bg, smooth, ddp):
        super().__init__()
        self.apply_nonlin, self.batch_dice, self.do_bg, self.smooth, self.ddp = apply_nonlin, batch_dice, do_bg, smooth, ddp

    def forward(self, x, y, loss_mask=None):
        intersect, sum_pred, sum_gt, _, _ = dice_ce_sums(x, y, loss_mask, None, self.apply_nonlin, _what=type(self).__name__)
        return self.from_sums(intersect, sum_pred, sum_gt)

    def _reduced(self, intersect, sum_pred, sum_gt):
        sum_gt = sum_gt.to(intersect.dtype)
        if self.batch_dice:
            intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
            if self.ddp:
                intersect, sum_pred, sum_gt = _sum_over_ranks(intersect), _sum_over_ranks(sum_pred), _sum_over_ranks(sum_gt)
        return intersect, sum_pred, sum_gt

    def _mean(self, dc):
        if not self.do_bg:
            dc = dc[1:] if self.batch_dice else dc[:, 1:]
        return -dc.mean()


class SoftDiceLoss(_DiceBase):
    """reference dice.py:9-56 on the three sums: tp = I, fp = P - I, fn = G - I"""

    def __init__(self, apply_nonlin: Callable = None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.,
                 ddp: bool = True, clip_tp: float = None):
        super().__init__(apply_nonlin, batch_dice, do_bg, smooth, ddp)
        self.clip_tp = clip_tp

    def from_sums(self, intersect, sum_pred, sum_gt):
        intersect, sum_pred, sum_gt = self._reduced(intersect, sum_pred, sum_gt)
        tp = intersect
        denominator = sum_pred + sum_gt                                      # 2 tp + fp + fn
        if self.clip_tp is not None:
            tp = torch.clip(intersect, min=self.clip_tp, max=None)
            denominator = 2 * tp + (sum_pred - intersect) + (sum_gt - intersect)
        return self._mean((2 * tp + self.smooth) / torch.clip(denominator + self.smooth, 1e-8))


class MemoryEfficientSoftDiceLoss(_DiceBase):
    """reference dice.py:58-116"""

    def __init__(self, apply_nonlin: Callable = None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.,
                 ddp: bool = True):
        super().__init__(apply_nonlin, batch_dice, do_bg, smooth, ddp)

    def from_sums(self, intersect, sum_pred, sum_gt):
        intersect, sum_pred, sum_gt = self._reduced(intersect, sum_pred, sum_gt)
        return self._mean((2 * intersect + self.smooth) / torch.clip(sum_gt + sum_pred + self.smooth, 1e-8))


def _check_ce_kwargs(weight, size_average, reduce, reduction, label_smoothing, what):
    if weight is not None:
        raise NotImplementedError(f"{what}: class weights are not supported (the cross-entropy kernel has none)")
    if label_smoothing:
        raise NotImplementedError(f"{what}: label_smoothing is not supported (the cross-entropy kernel has none)")
    if reduction != "mean" or size_average is not None or reduce is not None:
        raise NotImplementedError(f"{what}: only reduction='mean' is supported (the kernel sums; the mean is taken over the counted voxels)")


class RobustCrossEntropyLoss(nn.Module):
    """reference robust_ce_loss.py:6-16 on train_ops.cross_entropy: takes the float (B, 1, ...) target"""

    def __init__(self, weight=None, size_average=None, ignore_index: int = -100, reduce=None, reduction: str = "mean",
                 label_smoothing: float = 0.0):
        super().__init__()
        _check_ce_kwargs(weight, size_average, reduce, reduction, label_smoothing, "RobustCrossEntropyLoss")
        self.ignore_index = ignore_index

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if target.dim() == input.dim():
            if target.shape[1] != 1:
                raise ValueError(f"RobustCrossEntropyLoss: target must be (B, 1, *spatial) or (B, *spatial), got {tuple(target.shape)}")
            target = target[:, 0]
        return train_ops.cross_entropy(input, target.long(), self.ignore_index)


class TopKLoss(nn.Module):
    """reference robust_ce_loss.py:19-32 on train_ops.topk_cross_entropy: the mean of the largest k % of the per-voxel cross entropies,
    the ignored voxels counted with loss 0.  Takes the float (B, 1, ...) target, or (B, ...)."""

    def __init__(self, weight=None, ignore_index: int = -100, k: float = 10, label_smoothing: float = 0):
        super().__init__()
        _check_ce_kwargs(weight, None, None, "mean", label_smoothing, "TopKLoss")
        self.ignore_index, self.k = ignore_index, k

    def forward(self, inp: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if target.dim() == inp.dim():
            if target.shape[1] != 1:
                raise ValueError(f"TopKLoss: target must be (B, 1, *spatial) or (B, *spatial), got {tuple(target.shape)}")
            target = target[:, 0]
        return train_ops.topk_cross_entropy(inp, target.long(), self.k, self.ignore_index)


class DC_and_CE_loss(nn.Module):
    """reference compound_losses.py:8-57.  Both terms come from the same five sums; `ignore_label` goes into them instead of a mask and
    a cloned target, and the CE term is ce_sum / max(count, 1): 0 when every voxel is ignored."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None, dice_class=SoftDiceLoss):
        super().__init__()
        ce_kwargs = dict(ce_kwargs)
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice, self.weight_ce, self.ignore_label = weight_dice, weight_ce, ignore_label
        # kept under the reference's attribute name: it validates ce_kwargs and holds ignore_index; forward() takes the CE term from
        # the same five sums as the Dice term and does not call it
        self.ce = RobustCrossEntropyLoss(**ce_kwargs)
        self.dc = dice_class(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)
        if not isinstance(self.dc, _DiceBase):
            raise NotImplementedError("DC_and_CE_loss: dice_class must be SoftDiceLoss or MemoryEfficientSoftDiceLoss of this module")

    def forward(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.ignore_label is not None and target.dim() == net_output.dim() and target.shape[1] != 1:
            raise NotImplementedError("DC_and_CE_loss: ignore_label needs a label map (B, 1, ...), not a one-hot target")
        intersect, sum_pred, sum_gt, ce_sum, count = dice_ce_sums(net_output, target, None, self.ce.ignore_index, softmax_helper_dim1,
                                                                  _what="DC_and_CE_loss")
        result = intersect.new_zeros(())                       # a tensor also when both weights are 0
        if self.weight_ce != 0:
            result = self.weight_ce * (ce_sum.sum() / count.sum().clamp(min=1))
        if self.weight_dice != 0:
            result = result + self.weight_dice * self.dc.from_sums(intersect, sum_pred, sum_gt)
        return result


class DC_and_topk_loss(nn.Module):
    """reference compound_losses.py:103-151.  The Dice term is `SoftDiceLoss` on the sums (CPU tensors; it refuses device tensors),
    with the ignored voxels masked out as the reference does; it is skipped when `weight_dice == 0`, which then runs on the device.
    The reference's `num_fg > 0` rule needs no readback: if every voxel is ignored the map is all zeros and the top-k mean is 0."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None):
        super().__init__()
        ce_kwargs = dict(ce_kwargs)
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice, self.weight_ce, self.ignore_label = weight_dice, weight_ce, ignore_label
        self.ce = TopKLoss(**ce_kwargs)
        self.dc = SoftDiceLoss(apply_nonlin=softmax_helper_dim1, **soft_dice_kwargs)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        mask = None
        if self.ignore_label is not None:
            if target.dim() != net_output.dim() or target.shape[1] != 1:
                raise NotImplementedError("DC_and_topk_loss: ignore_label needs a label map (B, 1, ...), not a one-hot target")
            mask = target != self.ignore_label
        result = None
        if self.weight_ce != 0:
            result = self.weight_ce * self.ce(net_output, target)
        if self.weight_dice != 0:
            dc_loss = self.weight_dice * self.dc(net_output, target, loss_mask=mask)
            result = dc_loss if result is None else result + dc_loss
        return net_output.new_zeros((), dtype=torch.float32) if result is None else result


class DeepSupervisionWrapper(nn.Module):
    """reference deepsupervision.py:5-36: sum_i w_i loss(arg0[i], arg1[i], ...) over tuples / lists of equal length; w_i = 1 without
    weight_factors"""

    def __init__(self, loss, weight_factors=None):
        super().__init__()
        self.weight_factors = weight_factors
        self.loss = loss

    def forward(self, *args):
        for a in args:
            if not isinstance(a, (tuple, list)):
                raise TypeError(f"DeepSupervisionWrapper: every argument must be a tuple or a list, got {type(a)}")
        weights = [1] * len(args[0]) if self.weight_factors is None else self.weight_factors
        total = None
        for w, inputs in zip(weights, zip(*args)):
            term = w * self.loss(*inputs)
            total = term if total is None else total + term
        return total
