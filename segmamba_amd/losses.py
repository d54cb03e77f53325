"""The reference's nnU-Net training loss (light_training/loss/): Dice, cross entropy, top-k cross entropy and the region-based
sigmoid Dice + BCE under the reference's names.

  * `SoftDiceLoss`, `MemoryEfficientSoftDiceLoss` (dice.py:9-116), `RobustCrossEntropyLoss`, `TopKLoss` (robust_ce_loss.py:6-32),
    `DC_and_CE_loss`, `DC_and_topk_loss` (compound_losses.py:8-57, 103-151), `DeepSupervisionWrapper` (deepsupervision.py:5-36) and
    `softmax_helper_dim1` (helpers.py), with the reference's constructor signatures;
  * both Dice classes and the CE term of `DC_and_CE_loss` are built on five sums, `dice_ce_sums`: per (b, c) I = sum m p_c [y = c],
    P = sum m p_c, G = sum m [y = c] and, per b, the cross-entropy sum and the number of valid voxels.  SoftDiceLoss' tp, fp, fn are
    I, P - I, G - I; what follows the sums (batch_dice, do_bg, smooth, clip_tp, the clip of the denominator, the mean, the weights) is
    arithmetic on (B, C) tensors;
  * `dice_ce_sums` computes these softmax sums in ATen, for CPU tensors only, and has no ATen fall-back on the device: by default
    everything that needs them refuses device tensors with NotImplementedError;
  * `softmax_dice_sums` is the same five sums on the device, from csrc/dice_ce.hip (one pass over the logits, the labels and the mask
    for all classes, fp64 sums in a fixed order, a one-launch backward that recomputes the softmax; CPU tensors take `dice_ce_sums`'
    ATen formulas).  The opt-in keyword `device_sums=True` of `SoftDiceLoss`, `MemoryEfficientSoftDiceLoss`, `DC_and_CE_loss` and
    `DC_and_topk_loss` sends device tensors under `apply_nonlin=softmax_helper_dim1` there; the loss is then returned as float32.
    The default `device_sums=False` keeps every refusal;
  * on the device run `RobustCrossEntropyLoss` (on `train_ops.cross_entropy`), `TopKLoss` (on `train_ops.topk_cross_entropy`: the
    per-voxel map, an exact radix selection, a per-voxel backward - csrc/topk_ce.hip) and `DC_and_topk_loss` - with `weight_dice=0`,
    which never asks for the sums, or with `device_sums=True`, which takes them from `softmax_dice_sums`;
  * `DC_and_BCE_loss` (compound_losses.py:60-100), the region-based loss - one sigmoid output per region, Dice on the sigmoids plus
    BCEWithLogitsLoss - runs on the device on `region_sums`: per (b, r) I = sum m p t, P = sum m p, G = sum m t,
    E = sum m (max(x, 0) - x t + log1p(exp(-|x|))) and per b N = sum m, from csrc/region_loss.hip (one pass over the logits and the
    target for all regions, fp64 sums in a fixed order, a one-launch backward that recomputes the sigmoid).  Two target modes: the
    reference's one-hot planes (B, R, ...) - or (B, R + 1, ...) with `use_ignore_label`, the last plane being the ignore mask - and,
    with `regions=`, a label map (B, ...) as the feeders produce it: a region is a set of labels (`BRATS_REGIONS`: TC, WT, ET of
    3_train.py:68-72), the region target is never built.  `region_targets` is `convert_labels` for CPU callers and tests.  The Dice
    term goes through `from_sums` of this module's Dice classes, whose own `forward` keeps refusing device tensors.

Stated deviations from the reference: sum_gt is an integer count for both Dice classes; a batch whose voxels are all ignored gives 0
for the CE term (the reference's `num_fg > 0` rule; the top-k term needs no rule: its map is all zeros); a voxel the CE term of
`DC_and_CE_loss` ignores is left out of the Dice term too; a label outside [0, classes) that is not ignored gives NaN instead of an
indexing error; `TopKLoss` raises ValueError where k selects no voxel (the reference returns the NaN of an empty mean), and among
voxels tied with the k-th largest loss each gets an equal share of the gradient where `torch.topk` picks some of them (same value).
`DC_and_BCE_loss`: in label mode a label outside [0, 32) that is not ignored, or a float label that is no integer, gives NaN; the
sums are float64 and the loss is returned as float32; `weight`, `pos_weight` and reductions other than the mean are refused.
While a graph is being captured the device paths of `region_sums` and `softmax_dice_sums` raise RuntimeError before any launch,
forward and backward: capture of these losses is unsupported (a captured loss forward + backward once ended in a segmentation fault
whose cause was never found, and nothing here captures one).
Not here: AutoDeepSupervision, class weights, label smoothing, one-hot targets for the softmax classes, double backward.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

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
    raise NotImplementedError(f"{_what}: dice_ce_sums has no ATen fall-back on the device - use CPU tensors, pass device_sums=True "
                              "(softmax_dice_sums, the library's kernel for the sums under the softmax), or "
                              "train_ops.cross_entropy / RobustCrossEntropyLoss")


class _SoftmaxDiceSums(torch.autograd.Function):
    """segm_softmax_dice_fwd / segm_softmax_dice_bwd: differentiable in x through I, P and CE"""

    @staticmethod
    def forward(ctx, x, labels, mask, ignore_label):
        from . import lib as L, ops_raw
        I, P, G, CE, N = ops_raw.softmax_dice_fwd(L.get_lib(), x, labels, mask, ignore_label)
        ctx.save_for_backward(x, labels, *(() if mask is None else (mask,)))
        ctx.ignore_label = ignore_label
        ctx.mark_non_differentiable(G, N)
        return I, P, G, CE, N

    @staticmethod
    def backward(ctx, g_i, g_p, _g_g, g_ce, _g_n):
        from . import lib as L, ops_raw
        x, labels, *rest = ctx.saved_tensors
        _refuse_capture(x, "softmax_dice_sums backward")
        B, Cc = x.shape[:2]
        coefs = [torch.zeros(shape, dtype=torch.float32, device=x.device) if g is None else g.to(torch.float32)
                 for g, shape in ((g_i, (B, Cc)), (g_p, (B, Cc)), (g_ce, (B,)))]
        dx = ops_raw.softmax_dice_bwd(L.get_lib(), x, labels, coefs[0], coefs[1], coefs[2], rest[0] if rest else None, ctx.ignore_label)
        return dx, None, None, None


def softmax_dice_sums(x: torch.Tensor, target: torch.Tensor, loss_mask: Optional[torch.Tensor] = None,
                      ignore_label: Optional[int] = None, _what: str = "softmax_dice_sums"):
    """-> (I (B, C), P (B, C), G (B, C), CE (B), N (B)): with p = softmax(x, 1), I = sum m p_c [y = c], P = sum m p_c,
    G = sum m [y = c], CE = sum m (logsumexp(x) - x_y), N = sum m, where m = 0 at a label equal to `ignore_label` and where
    `loss_mask` is 0.  Differentiable in x through I, P and CE.

    x: logits (B, C <= 16, *spatial); target: a label map (B, 1, *spatial) or (B, *spatial), float or integer; loss_mask: bool, uint8
    or 0 / 1 float of either shape.  A label outside [0, C) that counts, or a float label that is no integer, gives NaN in its
    sample's I, P, CE.  Device tensors run on csrc/dice_ce.hip and give float64 sums (fp32 arithmetic on the logits as they lie in
    memory, any batch / class / row strides; logits without unit stride along the last axis are copied first); CPU tensors take
    `dice_ce_sums`' formulas in ATen."""
    from . import lib as L
    if x.dim() < 3:
        raise ValueError(f"{_what}: logits must be (B, C, *spatial), got {tuple(x.shape)}")
    on_device = L.on_device(x)
    if on_device:
        _refuse_capture(x, _what)                             # before anything is launched, the conversions of the target included
    labels = _labels_of(x, target, _what)
    mask = _mask_of(x, loss_mask, _what)
    if not on_device:
        return _sums_aten(x, labels, mask, ignore_label, softmax_helper_dim1)
    from . import ops_raw
    if not 1 <= x.shape[1] <= L.SOFTMAX_DICE_MAX_CLASSES:
        raise NotImplementedError(f"{_what}: 1 .. {L.SOFTMAX_DICE_MAX_CLASSES} classes have a kernel, got {x.shape[1]}")
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{_what}: logits of {x.dtype} have no kernel (fp32, fp16, bf16)")
    if not ops_raw.softmax_dice_layout_supported(x):
        x = x.contiguous()
    return _SoftmaxDiceSums.apply(x, labels.contiguous(), None if mask is None else mask.contiguous(),
                                  None if ignore_label is None else int(ignore_label))


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
    def __init__(self, apply_nonlin, batch_dice, do_bg, smooth, ddp, device_sums=False):
        super().__init__()
        self.apply_nonlin, self.batch_dice, self.do_bg, self.smooth, self.ddp = apply_nonlin, batch_dice, do_bg, smooth, ddp
        self.device_sums = bool(device_sums)

    def forward(self, x, y, loss_mask=None):
        from . import lib as L
        if self.device_sums and L.on_device(x):
            if self.apply_nonlin is not softmax_helper_dim1:
                raise NotImplementedError(f"{type(self).__name__}: device_sums=True serves apply_nonlin=softmax_helper_dim1 only - the "
                                          "kernel computes the softmax itself")
            intersect, sum_pred, sum_gt, _, _ = softmax_dice_sums(x, y, loss_mask, None, _what=type(self).__name__)
            return self.from_sums(intersect, sum_pred, sum_gt).to(torch.float32)
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
    """reference dice.py:9-56 on the three sums: tp = I, fp = P - I, fn = G - I.  `device_sums=True`: device tensors under the softmax
    take the sums from `softmax_dice_sums` and the loss is float32; the default refuses them."""

    def __init__(self, apply_nonlin: Callable = None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.,
                 ddp: bool = True, clip_tp: float = None, device_sums: bool = False):
        super().__init__(apply_nonlin, batch_dice, do_bg, smooth, ddp, device_sums)
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
    """reference dice.py:58-116; `device_sums` as in `SoftDiceLoss`"""

    def __init__(self, apply_nonlin: Callable = None, batch_dice: bool = False, do_bg: bool = True, smooth: float = 1.,
                 ddp: bool = True, device_sums: bool = False):
        super().__init__(apply_nonlin, batch_dice, do_bg, smooth, ddp, device_sums)

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
    a cloned target, and the CE term is ce_sum / max(count, 1): 0 when every voxel is ignored.  `device_sums=True`: device tensors take
    the sums from `softmax_dice_sums` (csrc/dice_ce.hip) and the loss is float32; the default refuses them."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None, dice_class=SoftDiceLoss,
                 device_sums: bool = False):
        super().__init__()
        self.device_sums = bool(device_sums)
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
        from . import lib as L
        on_kernel = self.device_sums and L.on_device(net_output)
        if on_kernel:
            intersect, sum_pred, sum_gt, ce_sum, count = softmax_dice_sums(net_output, target, None, self.ce.ignore_index,
                                                                           _what="DC_and_CE_loss")
        else:
            intersect, sum_pred, sum_gt, ce_sum, count = dice_ce_sums(net_output, target, None, self.ce.ignore_index,
                                                                      softmax_helper_dim1, _what="DC_and_CE_loss")
        result = intersect.new_zeros(())                       # a tensor also when both weights are 0
        if self.weight_ce != 0:
            result = self.weight_ce * (ce_sum.sum() / count.sum().clamp(min=1))
        if self.weight_dice != 0:
            result = result + self.weight_dice * self.dc.from_sums(intersect, sum_pred, sum_gt)
        return result.to(torch.float32) if on_kernel else result


class DC_and_topk_loss(nn.Module):
    """reference compound_losses.py:103-151.  The Dice term is `SoftDiceLoss` on the sums (CPU tensors; by default it refuses device tensors),
    with the ignored voxels masked out as the reference does; it is skipped when `weight_dice == 0`, which then runs on the device.
    The reference's `num_fg > 0` rule needs no readback: if every voxel is ignored the map is all zeros and the top-k mean is 0.
    `device_sums=True`: the Dice term of device tensors comes from `softmax_dice_sums` with mask = target != ignore_label, so the
    loss runs wholly on the device."""

    def __init__(self, soft_dice_kwargs, ce_kwargs, weight_ce=1, weight_dice=1, ignore_label=None, device_sums: bool = False):
        super().__init__()
        self.device_sums = bool(device_sums)
        ce_kwargs = dict(ce_kwargs)
        if ignore_label is not None:
            ce_kwargs["ignore_index"] = ignore_label
        self.weight_dice, self.weight_ce, self.ignore_label = weight_dice, weight_ce, ignore_label
        self.ce = TopKLoss(**ce_kwargs)
        self.dc = SoftDiceLoss(apply_nonlin=softmax_helper_dim1, device_sums=self.device_sums, **soft_dice_kwargs)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        from . import lib as L
        if self.device_sums and self.weight_dice != 0 and L.on_device(net_output):
            _refuse_capture(net_output, "DC_and_topk_loss")   # the Dice sums refuse capture: say so before the top-k kernels run
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


# ---------------------------------------------------------------------------------------------------------
# the region-based loss: sigmoid Dice + BCE on five sums
# ---------------------------------------------------------------------------------------------------------
BRATS_REGIONS = ((1, 3), (1, 2, 3), (3,))          # TC, WT, ET over the BraTS labels: convert_labels of the reference's 3_train.py:68-72
_MAX_REGIONS, _MAX_LABELS = 8, 32


def _region_masks(regions, what: str):
    """((labels of region 0), ...) -> one 32-bit membership mask per region"""
    try:
        regions = tuple(tuple(int(l) for l in reg) for reg in regions)
    except TypeError:
        raise ValueError(f"{what}: regions must be a sequence of sequences of labels, got {regions!r}") from None
    if not 1 <= len(regions) <= _MAX_REGIONS:
        raise ValueError(f"{what}: 1 .. {_MAX_REGIONS} regions, got {len(regions)}")
    masks = []
    for reg in regions:
        if any(not 0 <= l < _MAX_LABELS for l in reg):
            raise ValueError(f"{what}: the labels of a region must lie in [0, {_MAX_LABELS}), got {reg}")
        masks.append(sum(1 << l for l in set(reg)))
    return masks


def region_targets(labels: torch.Tensor, regions: Sequence[Sequence[int]] = BRATS_REGIONS) -> torch.Tensor:
    """label map (B, *spatial) -> float (B, R, *spatial), plane r = 1 where the label belongs to regions[r]: the reference's
    `convert_labels` (3_train.py:68-72) for any list of regions.  ATen, on whatever device the labels lie."""
    _region_masks(regions, "region_targets")
    planes = []
    for reg in regions:
        hit = torch.zeros_like(labels, dtype=torch.bool)
        for l in set(int(l) for l in reg):
            hit = hit | (labels == l)
        planes.append(hit)
    return torch.stack(planes, 1).float()


def _region_sums_aten(x, target, masks, ignore_label, ignore_plane):
    """the five formulas in ATen (CPU tensors): fp32 per voxel, float64 sums"""
    B, R = x.shape[:2]
    xf = x.float().reshape(B, R, -1)
    if masks is not None:
        lf = target.reshape(B, -1)
        if lf.is_floating_point():                            # a float label that is no integer is a wrong label, never ignored
            whole = (lf == lf.floor()) & (lf.abs() < 4.0e18)
            y = torch.where(whole, lf, torch.full_like(lf, -1)).long()
        else:
            whole, y = torch.ones_like(lf, dtype=torch.bool), lf.long()
        valid = torch.ones_like(y, dtype=torch.bool)
        if ignore_label is not None:
            valid = ~(whole & (y == int(ignore_label)))
        oob = valid & (~whole | (y < 0) | (y >= _MAX_LABELS))
        bits = torch.tensor(masks, dtype=torch.int64, device=x.device).view(1, R, 1)
        t = ((bits >> y.clamp(0, _MAX_LABELS - 1).unsqueeze(1)) & 1).to(xf.dtype) * (~oob).unsqueeze(1)
        poison = torch.where(oob.any(1), float("nan"), 0.0).double()[:, None]
    else:
        tf = target.float().reshape(B, target.shape[1], -1)
        t = tf[:, :R]
        valid = (1 - tf[:, R]) != 0 if ignore_plane else torch.ones_like(tf[:, 0], dtype=torch.bool)
        poison = 0.0
    m = valid.unsqueeze(1).to(xf.dtype)
    p = torch.sigmoid(xf)
    bce = torch.clamp(xf, min=0) - xf * t + torch.log1p(torch.exp(-xf.abs()))
    f64 = torch.float64
    return ((m * p * t).sum(2, dtype=f64) + poison, (m * p).sum(2, dtype=f64) + poison, (m * t).sum(2, dtype=f64),
            (m * bce).sum(2, dtype=f64) + poison, valid.sum(1).to(f64))


def _refuse_capture(x: torch.Tensor, what: str) -> None:
    """the runtime is asked only where one is up: without a device the query itself raises"""
    if (x.is_cuda or torch.cuda.is_initialized()) and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what}: graph capture of this loss is not supported - call it outside the captured region")


class _RegionSums(torch.autograd.Function):
    """segm_region_loss_fwd / segm_region_loss_bwd: differentiable in x through I, P and E"""

    @staticmethod
    def forward(ctx, x, target, masks, ignore_label, ignore_plane):
        from . import lib as L, ops_raw
        I, P, G, E, N = ops_raw.region_loss_fwd(L.get_lib(), x, target, masks, ignore_label, ignore_plane)
        ctx.save_for_backward(x, target)
        ctx.mode = (masks, ignore_label, ignore_plane)
        ctx.mark_non_differentiable(G, N)
        return I, P, G, E, N

    @staticmethod
    def backward(ctx, g_i, g_p, _g_g, g_e, _g_n):
        from . import lib as L, ops_raw
        x, target = ctx.saved_tensors
        _refuse_capture(x, "region_sums backward")
        B, R = x.shape[:2]
        coefs = [torch.zeros(B, R, dtype=torch.float32, device=x.device) if g is None else g.to(torch.float32) for g in (g_i, g_p, g_e)]
        masks, ignore_label, ignore_plane = ctx.mode
        dx = ops_raw.region_loss_bwd(L.get_lib(), x, target, coefs[0], coefs[1], coefs[2], masks, ignore_label, ignore_plane)
        return dx, None, None, None, None


def region_sums(x: torch.Tensor, target: torch.Tensor, regions: Optional[Sequence[Sequence[int]]] = None,
                ignore_label: Optional[int] = None, use_ignore_label: bool = False, _what: str = "region_sums"):
    """-> (I, P, G, E, N), float64: with p = sigmoid(x), per (b, r) I = sum m p t, P = sum m p, G = sum m t,
    E = sum m (max(x, 0) - x t + log1p(exp(-|x|))), and per b N = sum m.  Differentiable in x through I, P and E.

    x: logits (B, R <= 8, *spatial).  `regions` given: target is a label map (B, *spatial) or (B, 1, *spatial), t = [label in
    regions[r]], m = [label != ignore_label]; a label outside [0, 32) that is not ignored, or a float label that is no integer, gives
    NaN in that sample's I, P, E.  `regions` None: target holds the planes (B, R, *spatial), used as they are (soft targets work) - or
    (B, R + 1, *spatial) with `use_ignore_label`, m = ((1 - target[:, -1]) != 0).  Device tensors run on csrc/region_loss.hip (fp32
    arithmetic on the logits as they lie in memory, any batch / region / row strides; logits without unit stride along the last
    axis are copied first); CPU tensors take the same formulas in ATen."""
    from . import lib as L
    if x.dim() < 3:
        raise ValueError(f"{_what}: logits must be (B, R, *spatial), got {tuple(x.shape)}")
    B, R = x.shape[:2]
    sp = tuple(x.shape[2:])
    if not 1 <= R <= _MAX_REGIONS:
        raise ValueError(f"{_what}: 1 .. {_MAX_REGIONS} regions, got {R} channels")
    plane_like = target.dim() == x.dim() and tuple(target.shape[2:]) == sp and target.shape[0] == B and target.shape[1] in (R, R + 1) \
        and target.shape[1] != 1
    masks = None
    if regions is not None:
        if plane_like:
            raise ValueError(f"{_what}: regions= selects the label-map mode, but the target {tuple(target.shape)} holds planes")
        if use_ignore_label:
            raise ValueError(f"{_what}: use_ignore_label belongs to a plane target; a label map takes ignore_label=")
        masks = _region_masks(regions, _what)
        if len(masks) != R:
            raise ValueError(f"{_what}: {len(masks)} regions for logits of {R} channels")
        if target.dim() == x.dim() and target.shape[1] == 1:
            target = target[:, 0]
        if tuple(target.shape) != (B,) + sp:
            raise ValueError(f"{_what}: target must be (B, *spatial) or (B, 1, *spatial), got {tuple(target.shape)} for {tuple(x.shape)}")
        if target.dtype not in (torch.int64, torch.int16, torch.uint8, torch.float32):
            target = target.to(torch.float32 if target.is_floating_point() else torch.int64)
    else:
        if ignore_label is not None:
            raise ValueError(f"{_what}: ignore_label belongs to a label map (pass regions=); a plane target takes use_ignore_label")
        if tuple(target.shape) != (B, R + (1 if use_ignore_label else 0)) + sp:
            raise ValueError(f"{_what}: target must be (B, *spatial) or (B, 1, *spatial) with regions=, (B, R, *spatial), or "
                             f"(B, R + 1, *spatial) with use_ignore_label; got {tuple(target.shape)} for {tuple(x.shape)}")
        if target.dtype == torch.bool:
            target = target.contiguous().view(torch.uint8)
        elif target.dtype not in (torch.uint8, torch.float32):
            target = target.float()
    if not L.on_device(x):
        return _region_sums_aten(x, target, masks, ignore_label, bool(use_ignore_label))
    _refuse_capture(x, _what)
    from . import ops_raw
    if x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise NotImplementedError(f"{_what}: logits of {x.dtype} have no kernel (fp32, fp16, bf16)")
    if not ops_raw.region_loss_layout_supported(x):
        x = x.contiguous()
    return _RegionSums.apply(x, target.contiguous(), masks, None if ignore_label is None else int(ignore_label), bool(use_ignore_label))


class DC_and_BCE_loss(nn.Module):
    """reference compound_losses.py:60-100 on `region_sums`, plus `regions` / `ignore_label`, which select the label-map mode.

    Plane mode (the reference's): target (B, R, ...) one-hot or soft, or (B, R + 1, ...) with `use_ignore_label`.  Label mode:
    `regions=BRATS_REGIONS` (or any sets of labels), target (B, ...) or (B, 1, ...), `ignore_label` optional.  The Dice term is
    `dice_class(...).from_sums(I, P, G)` - batch_dice, do_bg (drops region 0, as the reference's x[:, 1:]), smooth, clip_tp, ddp and the
    clip of the denominator are that class' arithmetic.  The BCE term is E.sum() / (B R V) without a mask and
    E.sum() / clip(N.sum(), 1e-8) with one: the reference divides the masked sum over all regions by the number of valid voxels
    (compound_losses.py:96), not by R times that number."""

    def __init__(self, bce_kwargs, soft_dice_kwargs, weight_ce=1, weight_dice=1, use_ignore_label: bool = False,
                 dice_class=MemoryEfficientSoftDiceLoss, regions: Optional[Sequence[Sequence[int]]] = None,
                 ignore_label: Optional[int] = None):
        super().__init__()
        bce_kwargs = dict(bce_kwargs)
        if bce_kwargs.get("weight") is not None or bce_kwargs.get("pos_weight") is not None:
            raise NotImplementedError("DC_and_BCE_loss: weight and pos_weight are not supported (the kernel has none)")
        if bce_kwargs.get("reduction", "mean") != "mean" or bce_kwargs.get("size_average") is not None or \
                bce_kwargs.get("reduce") is not None:
            raise NotImplementedError("DC_and_BCE_loss: only reduction='mean' is supported (use_ignore_label masks the sum itself)")
        if dice_class not in (SoftDiceLoss, MemoryEfficientSoftDiceLoss):
            raise NotImplementedError("DC_and_BCE_loss: dice_class must be SoftDiceLoss or MemoryEfficientSoftDiceLoss of this module")
        if regions is not None and use_ignore_label:
            raise ValueError("DC_and_BCE_loss: use_ignore_label belongs to a plane target; with regions= pass ignore_label=")
        if regions is None and ignore_label is not None:
            raise ValueError("DC_and_BCE_loss: ignore_label belongs to the label-map mode; pass regions= as well")
        self.weight_dice, self.weight_ce, self.use_ignore_label = weight_dice, weight_ce, use_ignore_label
        self.regions = None if regions is None else tuple(tuple(int(l) for l in reg) for reg in regions)
        if self.regions is not None:
            _region_masks(self.regions, "DC_and_BCE_loss")
        self.ignore_label = ignore_label
        # kept under the reference's attribute name: it validates bce_kwargs; forward() takes the BCE term from the sums
        self.ce = nn.BCEWithLogitsLoss(**bce_kwargs)
        self.dc = dice_class(apply_nonlin=torch.sigmoid, **soft_dice_kwargs)

    def forward(self, net_output: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        intersect, sum_pred, sum_gt, bce_sum, count = region_sums(net_output, target, self.regions, self.ignore_label,
                                                                  self.use_ignore_label, _what="DC_and_BCE_loss")
        result = intersect.new_zeros(())                       # a tensor also when both weights are 0
        if self.weight_ce != 0:
            if self.use_ignore_label or self.ignore_label is not None:
                ce_loss = bce_sum.sum() / torch.clip(count.sum(), min=1e-8)
            else:
                ce_loss = bce_sum.sum() / net_output.numel()
            result = self.weight_ce * ce_loss
        if self.weight_dice != 0:
            result = result + self.weight_dice * self.dc.from_sums(intersect, sum_pred, sum_gt)
        return result.to(torch.float32)


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
