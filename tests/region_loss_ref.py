"""Float64 restatement of the reference's region-based loss (light_training/loss/compound_losses.py:60-100 with dice.py) written the
reference's way - sigmoid, one-hot products, tp / fp / fn or intersect / sum_pred / sum_gt, BCEWithLogitsLoss, the mask tiled over
the regions - so that it checks the five-sums form the library uses rather than repeating it; and the five sums and their gradient
from the definition, in numpy.  TEST INFRASTRUCTURE ONLY: the reference of tests/region_loss_checks.py and test_region_loss_cpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

BRATS = ((1, 3), (1, 2, 3), (3,))


def region_planes(labels, regions=BRATS):
    """label map (B, *sp) -> float64 (B, R, *sp): the three compares of the reference's convert_labels for any region list"""
    y = np.asarray(labels)
    return np.stack([np.isin(y, list(reg)) for reg in regions], 1).astype(np.float64)


def planes_of_masks(labels, masks):
    """label map (B, *sp) with labels in [0, 32) -> float64 (B, R, *sp): bit `label` of masks[r]"""
    y = np.asarray(labels).astype(np.int64)
    return np.stack([(np.int64(m) >> y) & 1 for m in masks], 1).astype(np.float64)


def sums(x, t, m=None):
    """x, t float64 (B, R, *sp), m (B, *sp) of 0 / 1 or None -> I, P, G, E (B, R), N (B), float64, from the definition:
    E is -(t log p + (1 - t) log(1 - p)) with log p = -logaddexp(0, -x)"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, R = x.shape[:2]
    xs, ts = x.reshape(B, R, -1), t.reshape(B, R, -1)
    ms = np.ones((B, 1, xs.shape[2])) if m is None else np.asarray(m, dtype=np.float64).reshape(B, 1, -1)
    p = 1.0 / (1.0 + np.exp(-xs))
    bce = ts * np.logaddexp(0.0, -xs) + (1.0 - ts) * np.logaddexp(0.0, xs)
    return (ms * p * ts).sum(2), (ms * p).sum(2), (ms * ts).sum(2), (ms * bce).sum(2), ms.sum((1, 2))


def sums_grad(x, t, m, g_i, g_p, g_e):
    """d (sum g_i I + g_p P + g_e E) / d x, float64, x's shape"""
    x, t = np.asarray(x, dtype=np.float64), np.asarray(t, dtype=np.float64)
    B, R = x.shape[:2]
    ex = (B, R) + (1,) * (x.ndim - 2)
    ms = np.ones((B, 1) + x.shape[2:]) if m is None else np.expand_dims(np.asarray(m, dtype=np.float64), 1)
    p = 1.0 / (1.0 + np.exp(-x))
    gi, gp, ge = (np.asarray(g, dtype=np.float64).reshape(ex) for g in (g_i, g_p, g_e))
    return ms * (p * (1.0 - p) * (gi * t + gp) + ge * (p - t))


def dc_and_bce(x, target, mask=None, kind="mem", batch_dice=False, do_bg=True, smooth=1.0, weight_ce=1.0, weight_dice=1.0):
    """x float64 tensor (B, R, *sp), target (B, R, *sp) planes, mask (B, 1, *sp) bool or None -> the loss as compound_losses.py:84-100
    and dice.py compute it"""
    t = torch.as_tensor(np.asarray(target, dtype=np.float64))
    mk = None if mask is None else torch.as_tensor(np.asarray(mask)).bool()
    p = torch.sigmoid(x)
    axes = tuple(range(2, x.dim()))
    tile = 1.0 if mk is None else mk.to(x.dtype).expand_as(x)
    if kind == "soft":
        tp, fp, fn = (p * t * tile).sum(axes), (p * (1 - t) * tile).sum(axes), ((1 - p) * t * tile).sum(axes)
        if batch_dice:
            tp, fp, fn = tp.sum(0), fp.sum(0), fn.sum(0)
        dc = (2 * tp + smooth) / torch.clip(2 * tp + fp + fn + smooth, 1e-8)
        if not do_bg:
            dc = dc[1:] if batch_dice else dc[:, 1:]
    else:
        pp, tt = (p, t) if do_bg else (p[:, 1:], t[:, 1:])
        tl = tile if mk is None or do_bg else tile[:, 1:]
        intersect, sum_pred, sum_gt = (pp * tt * tl).sum(axes), (pp * tl).sum(axes), (tt * tl).sum(axes)
        if batch_dice:
            intersect, sum_pred, sum_gt = intersect.sum(0), sum_pred.sum(0), sum_gt.sum(0)
        dc = (2 * intersect + smooth) / torch.clip(sum_gt + sum_pred + smooth, 1e-8)
    dice = -dc.mean()
    if mk is None:
        ce = F.binary_cross_entropy_with_logits(x, t)
    else:
        ce = (F.binary_cross_entropy_with_logits(x, t, reduction="none") * mk).sum() / torch.clip(mk.sum(), min=1e-8)
    return weight_ce * ce + weight_dice * dice


def value_and_grad(fn, logits, *args, **kw):
    """fn(x float64 leaf, *args, **kw) -> scalar: (value float, d value / d logits as a float64 array)"""
    x = torch.as_tensor(np.asarray(logits, dtype=np.float64)).requires_grad_(True)
    v = fn(x, *args, **kw)
    v.backward()
    return float(v.detach()), x.grad.numpy()
