"""Float64 restatement of the reference's Dice + cross-entropy loss (light_training/loss/dice.py, compound_losses.py, robust_ce_loss.py)
in torch, written the way the reference computes - softmax, one-hot, products, sums - so that it checks the (I, P, G) form the library
uses rather than repeating it.  TEST INFRASTRUCTURE ONLY: the reference of tests/test_losses_cpu.py."""
import numpy as np
import torch


def _f64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float64))


def sums(x, y, mask=None, ignore=None):
    """x (B, C, *sp) float64 tensor, y (B, *sp) integer array, mask (B, *sp) or None -> I, P, G (B, C), ce (B), count (B); float64.
    A valid label outside [0, C) gives NaN in I, P, ce of its sample."""
    B, C = x.shape[:2]
    xs = x.reshape(B, C, -1)
    y = torch.as_tensor(np.asarray(y)).reshape(B, -1).long()
    valid = torch.ones_like(y, dtype=torch.bool)
    if ignore is not None:
        valid &= y != ignore
    if mask is not None:
        valid &= torch.as_tensor(np.asarray(mask)).reshape(B, -1) != 0
    oob = valid & ((y < 0) | (y >= C))
    onehot = torch.zeros_like(xs)
    onehot.scatter_(1, y.clamp(0, C - 1).unsqueeze(1), 1.0)
    onehot = onehot * (valid & ~oob).unsqueeze(1)
    m = valid.unsqueeze(1).to(xs.dtype)
    p = torch.softmax(xs, 1)
    nan = torch.where(oob.any(1), float("nan"), 0.0).to(xs.dtype)
    logp = torch.log_softmax(xs, 1)
    ce = -(logp * onehot).sum((1, 2)) + nan
    return (p * onehot).sum(2) + nan[:, None], (p * m).sum(2) + nan[:, None], onehot.sum(2), ce, valid.sum(1).to(xs.dtype)


def dice(x, y, kind="mem", batch_dice=False, do_bg=True, smooth=1.0, clip_tp=None, mask=None, ignore=None):
    """-mean Dice of softmax(x) against y as dice.py computes it; kind "soft" (tp / fp / fn) or "mem" (intersect / sum_pred / sum_gt)"""
    B, C = x.shape[:2]
    xs = x.reshape(B, C, -1)
    yl = torch.as_tensor(np.asarray(y)).reshape(B, -1).long()
    valid = torch.ones_like(yl, dtype=torch.bool)
    if ignore is not None:
        valid &= yl != ignore
    if mask is not None:
        valid &= torch.as_tensor(np.asarray(mask)).reshape(B, -1) != 0
    yl = torch.where(valid, yl, torch.zeros_like(yl))
    onehot = torch.zeros_like(xs)
    onehot.scatter_(1, yl.unsqueeze(1), 1.0)
    m = valid.unsqueeze(1).to(xs.dtype)
    p = torch.softmax(xs, 1)
    axes = (0, 2) if batch_dice else (2,)
    if kind == "soft":
        tp, fp, fn = (p * onehot * m).sum(axes), (p * (1 - onehot) * m).sum(axes), ((1 - p) * onehot * m).sum(axes)
        if clip_tp is not None:
            tp = torch.clip(tp, min=clip_tp)
        dc = (2 * tp + smooth) / torch.clip(2 * tp + fp + fn + smooth, 1e-8)
    else:
        assert clip_tp is None
        dc = (2 * (p * onehot * m).sum(axes) + smooth) / torch.clip((onehot * m).sum(axes) + (p * m).sum(axes) + smooth, 1e-8)
    if not do_bg:
        dc = dc[1:] if batch_dice else dc[:, 1:]
    return -dc.mean()


def cross_entropy(x, y, ignore=None, mask=None):
    """mean over the valid voxels of -log softmax(x)[y]; 0 when there is none"""
    _, _, _, ce, n = sums(x, y, mask, ignore)
    return ce.sum() / n.sum().clamp(min=1)


def dc_and_ce(x, y, kind="mem", batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1.0, weight_dice=1.0, ignore=None, clip_tp=None,
              mask=None):
    out = 0.0
    if weight_ce != 0:
        out = out + weight_ce * cross_entropy(x, y, ignore, mask)
    if weight_dice != 0:
        out = out + weight_dice * dice(x, y, kind, batch_dice, do_bg, smooth, clip_tp, mask, ignore)
    return out


def value_and_grad(fn, logits, *args, **kw):
    """fn(x float64 leaf, *args, **kw) -> scalar: (value float, d value / d logits as a float64 array)"""
    x = _f64(logits).requires_grad_(True)
    v = fn(x, *args, **kw)
    v.backward()
    return float(v.detach()), x.grad.numpy()

