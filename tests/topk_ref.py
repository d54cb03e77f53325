"""Float64 restatement of the reference's TopKLoss (light_training/loss/robust_ce_loss.py:19-32) in numpy, and the inputs of the
recorded cases (tests/golden/topk_ce.npz).  Written from the definition - log-softmax, a sort, a mean - so that it checks the
(threshold, n_gt, n_eq, sum_gt) form the library uses rather than repeating it.  Ties take the share rule of the library: every voxel
equal to the threshold gets (kk - n_gt) / n_eq of a selected voxel's gradient.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

SEED = 31
# (B, *spatial), classes, k in percent, the ignored label or None (ignored means every 7th voxel of the flattened label map)
CASES = (((2, 5, 6, 7), 4, 10, None),
         ((2, 9, 11, 13), 3, 10, 3),
         ((1, 3, 5, 7), 16, 50, None),
         ((2, 5, 6, 7), 4, 100, 4),
         ((2, 5, 6, 7), 4, 0.5, None),
         ((3, 4, 4, 4), 2, 25, None))
DICE_CASES = (0, 3, 5)                      # the cases DC_and_topk_loss is recorded for, with DICE_KWARGS
DICE_KWARGS = dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False)


def case_inputs(i):
    """-> logits float32 (B, C, *spatial) = 2 N(0, 1), labels int64 (B, *spatial); numpy's legacy generator, whose stream is frozen"""
    shape, C, _, ignore = CASES[i]
    rs = np.random.RandomState(SEED + 1000 * i)
    logits = (2.0 * rs.standard_normal((shape[0], C) + shape[1:])).astype(np.float32)
    labels = rs.randint(0, C, size=shape).astype(np.int64)
    if ignore is not None:
        labels.reshape(-1)[::7] = ignore
    return logits, labels


def kk_of(n, k):
    return int(n * k / 100)


def loss_map(logits, labels, ignore=None):
    """float64 (B, *spatial): logsumexp - x[label]; 0 where ignored; NaN where the label is outside [0, C) and not ignored"""
    x = np.asarray(logits, dtype=np.float64)
    B, C = x.shape[:2]
    xs = x.reshape(B, C, -1)
    y = np.asarray(labels).reshape(B, -1).astype(np.int64)
    mx = xs.max(1)
    lse = mx + np.log(np.exp(xs - mx[:, None]).sum(1))
    ign = np.zeros_like(y, dtype=bool) if ignore is None else y == ignore
    oob = ~ign & ((y < 0) | (y >= C))
    xy = np.take_along_axis(xs, np.clip(y, 0, C - 1)[:, None], 1)[:, 0]
    out = np.where(ign, 0.0, np.where(oob, np.nan, lse - xy))
    return out.reshape(np.asarray(labels).shape)


def select(values, kk):
    """-> (threshold, n_gt, n_eq, sum_gt) of the kk-th largest of `values` (NaN sorts above +inf, as np.sort puts it)"""
    v = np.asarray(values).reshape(-1)
    n = v.size
    thr = np.partition(v, n - kk)[n - kk]
    if np.isnan(thr):
        gt, eq = np.zeros(n, dtype=bool), np.isnan(v)
    else:
        gt, eq = (v > thr) | np.isnan(v), v == thr
    return thr, int(gt.sum()), int(eq.sum()), math.fsum(v[gt].astype(np.float64).tolist())


def softmax_minus_onehot(logits, labels, ignore=None):
    """float64 (B, C, *spatial): d loss_v / d logits; 0 where ignored; NaN where the label is wrong"""
    x = np.asarray(logits, dtype=np.float64)
    B, C = x.shape[:2]
    xs = x.reshape(B, C, -1)
    y = np.asarray(labels).reshape(B, -1).astype(np.int64)
    e = np.exp(xs - xs.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    d = p - (np.arange(C)[None, :, None] == y[:, None])
    ign = np.zeros_like(y, dtype=bool) if ignore is None else y == ignore
    oob = ~ign & ((y < 0) | (y >= C))
    d = np.where(ign[:, None], 0.0, np.where(oob[:, None], np.nan, d))
    return d.reshape(x.shape)


def topk_weight(lmap, kk):
    """float64, lmap's shape: 1 / kk above the threshold, (kk - n_gt) / (n_eq kk) at it, 0 below"""
    thr, n_gt, n_eq, _ = select(lmap, kk)
    m = np.asarray(lmap, dtype=np.float64)
    if np.isnan(thr):
        gt, eq = np.zeros(m.shape, dtype=bool), np.isnan(m)
    else:
        gt, eq = (m > thr) | np.isnan(m), m == thr
    return np.where(gt, 1.0 / kk, np.where(eq, (kk - n_gt) / (n_eq * kk), 0.0))


def topk_loss(logits, labels, k, ignore=None):
    """-> (loss, d loss / d logits) in float64"""
    m = loss_map(logits, labels, ignore)
    kk = kk_of(m.size, k)
    thr, n_gt, n_eq, sum_gt = select(m, kk)
    value = (sum_gt + (kk - n_gt) * float(thr)) / kk
    w = topk_weight(m, kk)
    return value, softmax_minus_onehot(logits, labels, ignore) * np.expand_dims(w, 1)


def boundary_gap(logits, labels, k, ignore=None):
    """the float64 losses on either side of the kk boundary: sorted[kk - 1] - sorted[kk] (inf when kk == n)"""
    m = np.sort(loss_map(logits, labels, ignore).reshape(-1))[::-1]
    kk = kk_of(m.size, k)
    return float("inf") if kk >= m.size else float(m[kk - 1] - m[kk])
