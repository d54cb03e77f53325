"""Evaluation on the device: Dice, Hausdorff distance and HD95 of label volumes (csrc/metrics.hip).

The last stage of the reference's pipeline, `5_compute_metrics.py`, calls `medpy.metric.binary.dc / hd95` per BraTS region on
the host; `3_train.py:82-119` computes a validation Dice the same way.  The functions here carry medpy's names and definitions
(connectivity 1, `numpy.percentile` interpolation) and run on the library's kernels: one pass for region counts and borders, one
batched exact squared distance transform, one gather of the distances at the border voxels.  Tensors stay on the device; numpy
arrays and host tensors are uploaded.  Only a handful of scalars is read back per call.

Volumes with a side beyond 256 (CT cases) take the box route: one launch gives the box of `border(P) | border(G)` of every region,
both border volumes are cropped to it, and the crop is transformed by the brute-force kernel if its sides are at most 256, else by
the linear-time one (csrc/edt_long.hip, sides up to 2048).  The crop is exact: every border voxel of either mask lies inside the
box, so the nearest one does too.  `SEGM_EDT_LONG=1` (read per call) forces the box route and the linear-time kernel at every
size, `SEGM_EDT_LONG=box` the box route with the kernel chosen by the crop's size, i.e. what a large volume gets.

The evaluation report (`asd`, `assd`, `nsd`, `confusion` and the functions and `ALL_METRICS` of the reference's
`light_training/evaluation/metric.py`, `case_report`, `evaluate_report`) needs no distance list: `_Pass.summary` asks
`segm_border_stats` (csrc/surface_stats.hip) for counts, sums, maxima, within-tolerance counts and two exact order statistics per
region, on the same distance-transform planes.  `hd95`, `hd`, `surface_distances`, `case_metrics` and `evaluate` keep the list route.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L
from . import ops_raw

BRATS_REGIONS: Tuple[Tuple[int, ...], ...] = ((1, 3), (1, 2, 3), (3,))      # TC, WT, ET (5_compute_metrics.py:40-46)
_BINARY = ((1,),)
_INT_SENTINEL = 2 ** 31 - 1

_tables = {}


def _long_mode() -> str:
    """SEGM_EDT_LONG, read per call: "" (route by size), "1" (box route, linear-time kernel) or "box" (box route, kernel by crop size)"""
    v = os.environ.get("SEGM_EDT_LONG", "").strip().lower()
    if v in ("", "0"):
        return ""
    if v not in ("1", "box"):
        raise RuntimeError(f"SEGM_EDT_LONG must be unset, 0, 1 or box, got {v!r}")
    return v


def _readback(t: torch.Tensor) -> list:
    """a device-to-host copy of a few scalars (the only kind this module makes: two per case)"""
    return t.tolist()


def _edt_sq(lib, volumes: torch.Tensor, planes, spacing, mode: str) -> torch.Tensor:
    """the brute-force kernel when every side is at most 256 (and the linear-time one is not forced), else the linear-time kernel"""
    if mode != "1" and max(volumes.shape[1:]) <= L.EDT_MAX_LINE:
        return ops_raw.edt_sq(lib, volumes, planes, spacing)
    return ops_raw.edt_sq_long(lib, volumes, planes, spacing)


def _table(regions, device) -> torch.Tensor:
    """the 256-entry label -> region-bits table of `regions` on `device`"""
    regions = tuple(tuple(int(v) for v in r) for r in regions)
    if not 1 <= len(regions) <= L.METRICS_MAX_REGIONS:
        raise RuntimeError(f"between 1 and {L.METRICS_MAX_REGIONS} regions per call, got {len(regions)}")
    key = (regions, str(device))
    if key not in _tables:
        t = np.zeros(256, dtype=np.uint8)
        for r, labels in enumerate(regions):
            for v in labels:
                if not 0 <= v <= 255:
                    raise RuntimeError(f"label {v} of region {r} is outside [0, 255]")
                t[v] |= 1 << r
        _tables[key] = torch.from_numpy(t).to(device)
    return _tables[key]


def _groups(regions):
    """the regions in groups of at most L.METRICS_MAX_REGIONS: the kernels carry 8 region planes per call"""
    regions = list(regions)
    return [regions[i:i + L.METRICS_MAX_REGIONS] for i in range(0, len(regions), L.METRICS_MAX_REGIONS)]


def _to_device(x) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"a tensor or a numpy array is required, got {type(x)}")
    if not L.on_device(t):
        t = t.to("cuda")
    return t


def _labels(x) -> torch.Tensor:
    """a label volume as the kernels take it: uint8, contiguous, on the device (labels must lie in [0, 255])"""
    t = _to_device(x)
    if t.dtype != torch.uint8:
        t = t.to(torch.uint8)
    return t.contiguous()


def _mask(x) -> torch.Tensor:
    """medpy's `astype(bool)`: non-zero = inside"""
    t = _to_device(x)
    return (t != 0).to(torch.uint8).contiguous()


def _volume3(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dim() != 3:
        raise RuntimeError(f"{what}: a (D, H, W) volume is required, got shape {tuple(t.shape)}")
    return t


def _pair(result, reference, conv, what):
    a, b = _volume3(conv(result), what), _volume3(conv(reference), what)
    if a.shape != b.shape:
        raise RuntimeError(f"{what}: shapes {tuple(a.shape)} and {tuple(b.shape)} differ")
    if b.device != a.device:
        b = b.to(a.device)
    return a, b


def _dice(p: int, g: int, both: int) -> float:
    return 2.0 * both / float(p + g) if p + g > 0 else 0.0


def region_masks(labels, regions: Sequence[Sequence[int]] = BRATS_REGIONS) -> torch.Tensor:
    """`convert_labels` of the reference: (n_regions, *labels.shape) fp32 masks, region r = labels in regions[r]"""
    t = _labels(labels)
    if len(regions) > L.METRICS_MAX_REGIONS:                              # any number of regions: eight at a time
        return torch.cat([region_masks(t, g) for g in _groups(regions)])
    bits = _table(regions, t.device)[t.long()]
    return torch.stack([(bits >> r) & 1 for r in range(len(regions))]).float()


def dc(result, reference) -> float:
    """Dice coefficient 2 n(A and B) / (n(A) + n(B)) of two binary volumes; 0.0 when both are empty (medpy.metric.binary.dc)"""
    a, b = _pair(result, reference, _mask, "dc")
    _, counts = ops_raw.seg_regions(L.get_lib(), a, b, _table(_BINARY, a.device))
    c = counts[:, 0].tolist()
    return _dice(c[0], c[1], c[2])


def distance_transform_edt(mask, sampling: Optional[Sequence[float]] = None) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt: the distance of every non-zero voxel to the nearest zero voxel (0 at zero voxels), fp32;
    +inf everywhere when `mask` has no zero voxel.  Each side of the volume is limited to 2048 voxels (RuntimeError beyond): the
    brute-force kernel serves volumes whose sides are all at most 256, the linear-time kernel every larger one."""
    m = _volume3(_to_device(mask), "distance_transform_edt")
    zero = (m == 0).to(torch.uint8).contiguous()
    e = _edt_sq(L.get_lib(), zero[None], [(0, 0)], sampling, _long_mode())[0]
    if e.dtype == torch.int32:
        return torch.where(e == _INT_SENTINEL, torch.full((), math.inf, device=e.device), e.float().sqrt())
    return e.sqrt()


# per region: HD95 and HD of the joined list, the mean distance P -> G and G -> P, the voxel-counted surface Dice (`_Pass.summary`)
SurfaceSummary = namedtuple("SurfaceSummary", "hd95 hd asd_pg asd_gp nsd")


class _Pass:
    """region counts and borders of one (prediction, ground truth) pair, and the border-to-border distance lists made from them"""

    def __init__(self, pred: torch.Tensor, gt: torch.Tensor, regions):
        self.lib = L.get_lib()
        self.n_regions = len(regions)
        self.borders, counts = ops_raw.seg_regions(self.lib, pred, gt, _table(regions, pred.device))
        self.mode = _long_mode()
        self.boxed = self.mode != "" or max(pred.shape) > L.EDT_MAX_LINE
        if not self.boxed:
            self.counts = counts[:, :self.n_regions].tolist()             # first readback: [|P|, |G|, |P and G|, |dP|, |dG|][region]
            return
        # the boxes of border(P) | border(G) of every region, issued before the first readback and read back with the counts
        boxes = ops_raw.planes_bbox(self.lib, self.borders, [(0, r, 1, r) for r in range(self.n_regions)])
        flat = _readback(torch.cat([counts.reshape(-1), boxes[:self.n_regions].reshape(-1).to(torch.int64)]))
        w = L.METRICS_MAX_REGIONS
        self.counts = [flat[q * w:q * w + self.n_regions] for q in range(5)]
        self.boxes = [flat[5 * w + 6 * r:5 * w + 6 * r + 6] for r in range(self.n_regions)]

    def live(self, r: int) -> bool:
        return self.counts[0][r] > 0 and self.counts[1][r] > 0

    def dice(self, r: int) -> float:
        return _dice(self.counts[0][r], self.counts[1][r], self.counts[2][r])

    def distances(self, regions_idx, spacing):
        """-> (flat fp32 vector, [(offset, n(border P), n(border G))] per region of `regions_idx`): for each region the distances from
        the border of P to the border of G, then from the border of G to the border of P"""
        if self.boxed:
            return self._distances_boxed(regions_idx, spacing)
        planes, items, cnt, seg = [], [], [], []
        off = 0
        for i, r in enumerate(regions_idx):
            planes += [(0, r), (1, r)]                                    # edt plane 2 i: to the border of P; 2 i + 1: to the border of G
            items += [(0, r, 2 * i + 1), (1, r, 2 * i)]
            n_p, n_g = self.counts[3][r], self.counts[4][r]
            cnt += [n_p, n_g]
            seg.append((off, n_p, n_g))
            off += n_p + n_g
        edt = ops_raw.edt_sq(self.lib, self.borders, planes, spacing)
        return ops_raw.border_distances(self.lib, self.borders, edt, items, cnt), seg

    def _distances_boxed(self, regions_idx, spacing):
        """the same vector and segments from per-region crops to the box of border(P) | border(G): cropping keeps the memory order of
        the border voxels and every candidate for the nearest one"""
        parts, seg = [], []
        off = 0
        for r in regions_idx:
            z0, z1, y0, y1, x0, x1 = self.boxes[r]
            n_p, n_g = self.counts[3][r], self.counts[4][r]
            if n_p + n_g > 0:
                crop = self.borders[:, z0:z1, y0:y1, x0:x1].contiguous()
                edt = _edt_sq(self.lib, crop, [(0, r), (1, r)], spacing, self.mode)      # plane 0: to the border of P; 1: of G
                parts.append(ops_raw.border_distances(self.lib, crop, edt, [(0, r, 1), (1, r, 0)], [n_p, n_g]))
            seg.append((off, n_p, n_g))
            off += n_p + n_g
        if not parts:
            return torch.empty(0, dtype=torch.float32, device=self.borders.device), seg
        return (parts[0] if len(parts) == 1 else torch.cat(parts)), seg

    def hausdorff(self, regions_idx, spacing):
        """-> [(hd95, hd)] per region of `regions_idx`, with one readback for all of them"""
        if not regions_idx:
            return []
        dist, seg = self.distances(regions_idx, spacing)
        picks, frac = [], []
        for off, n_p, n_g in seg:
            n = n_p + n_g
            s = torch.sort(dist[off:off + n]).values
            rank = 0.95 * (n - 1)                                         # numpy.percentile, linear interpolation
            lo = int(math.floor(rank))
            hi = min(lo + 1, n - 1)
            frac.append(rank - lo)
            # the box route selects with host integers: no index tensor is uploaded, nothing but the two readbacks synchronises
            picks.append(torch.stack((s[lo], s[hi], s[n - 1])) if self.boxed else s[[lo, hi, n - 1]])
        if self.boxed:
            vals = np.asarray(_readback(torch.stack(picks).double()))     # second readback
        else:
            vals = torch.stack(picks).double().cpu().numpy()              # second readback
        return [(float(v[0] + (v[1] - v[0]) * f), float(v[2])) for v, f in zip(vals, frac)]

    def summary(self, regions_idx, spacing, tolerance=None):
        """-> [SurfaceSummary] per region of `regions_idx` (each non-empty on both sides), with one readback for all of them: what
        asd / assd / hd / hd95 and the surface Dice are made of, from segm_border_stats - the distance transform of `distances`, then
        counts, sums, maxima and two order statistics instead of the distance lists and their sorts.  One group per region: the
        P -> G item and the G -> P item; the ranks are `hausdorff`'s, from the border counts of the first readback."""
        if not regions_idx:
            return []
        tol = -1.0 if tolerance is None else float(tolerance)
        ranks, frac = [], []
        for r in regions_idx:
            n = self.counts[3][r] + self.counts[4][r]
            rank = 0.95 * (n - 1)                                         # numpy.percentile, linear interpolation
            lo = int(math.floor(rank))
            ranks.append((lo, min(lo + 1, n - 1)))
            frac.append(rank - lo)
        w = L.METRICS_MAX_PLANES
        if self.boxed:
            outs = []
            for k, r in enumerate(regions_idx):
                z0, z1, y0, y1, x0, x1 = self.boxes[r]
                crop = self.borders[:, z0:z1, y0:y1, x0:x1].contiguous()
                edt = _edt_sq(self.lib, crop, [(0, r), (1, r)], spacing, self.mode)      # plane 0: to the border of P; 1: of G
                outs.append(ops_raw.border_stats(self.lib, crop, edt, [(0, r, 1), (1, r, 0)], [0, 0], 1, [tol, tol], [ranks[k]]))
            vals = _readback(outs[0] if len(outs) == 1 else torch.cat(outs))             # second readback
            rows = [(vals[6 * w * k:6 * w * k + 4], vals[6 * w * k + 4:6 * w * k + 8], vals[6 * w * k + 4 * w:6 * w * k + 4 * w + 2])
                    for k in range(len(regions_idx))]
        else:
            planes, items, groups = [], [], []
            for i, r in enumerate(regions_idx):
                planes += [(0, r), (1, r)]                                # edt plane 2 i: to the border of P; 2 i + 1: to the border of G
                items += [(0, r, 2 * i + 1), (1, r, 2 * i)]
                groups += [i, i]
            edt = ops_raw.edt_sq(self.lib, self.borders, planes, spacing)
            vals = _readback(ops_raw.border_stats(self.lib, self.borders, edt, items, groups, len(regions_idx), [tol] * len(items), ranks))
            rows = [(vals[8 * i:8 * i + 4], vals[8 * i + 4:8 * i + 8], vals[4 * w + 2 * i:4 * w + 2 * i + 2]) for i in range(len(regions_idx))]
        out = []
        for (p, g, v), f in zip(rows, frac):
            n_p, n_g = int(p[0]), int(g[0])
            out.append(SurfaceSummary(hd95=float(v[0] + (v[1] - v[0]) * f), hd=float(max(p[2], g[2])),
                                      asd_pg=p[1] / n_p, asd_gp=g[1] / n_g,
                                      nsd=(p[3] + g[3]) / float(n_p + n_g) if tolerance is not None else math.nan))
        return out


def _binary_pass(result, reference, what) -> _Pass:
    a, b = _pair(result, reference, _mask, what)
    p = _Pass(a, b, _BINARY)
    if p.counts[0][0] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if p.counts[1][0] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return p


def surface_distances(result, reference, voxelspacing: Optional[Sequence[float]] = None) -> torch.Tensor:
    """medpy's `__surface_distances` (connectivity 1): the distance from every border voxel of `result` (in memory order) to the nearest
    border voxel of `reference`, fp32 on the device.  Raises RuntimeError when either volume is empty, as medpy does."""
    p = _binary_pass(result, reference, "surface_distances")
    dist, seg = p.distances([0], voxelspacing)
    return dist[:seg[0][1]]


def hd95(result, reference, voxelspacing: Optional[Sequence[float]] = None) -> float:
    """95th percentile of the joined surface distances result -> reference and reference -> result (medpy.metric.binary.hd95:
    `numpy.percentile(hstack(...), 95)`, linear interpolation)"""
    return _binary_pass(result, reference, "hd95").hausdorff([0], voxelspacing)[0][0]


def hd(result, reference, voxelspacing: Optional[Sequence[float]] = None) -> float:
    """Hausdorff distance: the maximum of the same joined list (medpy.metric.binary.hd)"""
    return _binary_pass(result, reference, "hd").hausdorff([0], voxelspacing)[0][1]


def case_metrics(pred_labels, gt_labels, voxelspacing: Optional[Sequence[float]] = (1, 1, 1),
                 regions: Sequence[Sequence[int]] = BRATS_REGIONS, max_regions: Optional[int] = L.METRICS_MAX_REGIONS) -> np.ndarray:
    """`each_cases_metric` of 5_compute_metrics.py on label volumes: (n_regions, 2) = [dice, hd95] per region, with the reference's rule
    for empty masks (`cal_metric`, :24-30): [0.0, 50] unless both the prediction and the ground truth of the region are non-empty.
    `max_regions` bounds the number of regions a call accepts (8 by default: what one kernel call carries, and what this function
    always refused beyond); `max_regions=None` takes any number, e.g. one region per organ, and runs them in groups of 8 through the
    same kernels (two readbacks per group), concatenated."""
    pred, gt = _pair(pred_labels, gt_labels, _labels, "case_metrics")
    if max_regions is not None and len(regions) > int(max_regions):
        raise RuntimeError(f"case_metrics: at most {int(max_regions)} regions per call (max_regions=None lifts the bound), got {len(regions)}")
    if len(regions) > L.METRICS_MAX_REGIONS:                              # eight at a time, concatenated
        return np.concatenate([case_metrics(pred, gt, voxelspacing, g) for g in _groups(regions)])
    p = _Pass(pred, gt, regions)
    out = np.zeros((len(regions), 2), dtype=np.float64)
    out[:, 1] = 50.0
    live = [r for r in range(len(regions)) if p.live(r)]
    for r, (h95, _) in zip(live, p.hausdorff(live, voxelspacing)):
        out[r] = (p.dice(r), h95)
    return out


def validation_dice(pred_labels, gt_labels, regions: Sequence[Sequence[int]] = BRATS_REGIONS) -> np.ndarray:
    """The validation rule of 3_train.py:82-119 per region: Dice if both are non-empty, 1.0 if both are empty, else 0.0.  Counts only;
    leading batch dimensions are counted as one volume, as the reference does."""
    pred, gt = _labels(pred_labels), _labels(gt_labels)
    if pred.shape != gt.shape or pred.dim() < 3:
        raise RuntimeError(f"validation_dice: two label tensors of one shape (..., D, H, W) are required, got {tuple(pred.shape)} and {tuple(gt.shape)}")
    if gt.device != pred.device:
        gt = gt.to(pred.device)
    if len(regions) > L.METRICS_MAX_REGIONS:
        return np.concatenate([validation_dice(pred, gt, g) for g in _groups(regions)])
    shape = (-1,) + tuple(pred.shape[-2:])
    _, counts = ops_raw.seg_regions(L.get_lib(), pred.reshape(shape), gt.reshape(shape), _table(regions, pred.device))
    c = counts[:, :len(regions)].tolist()
    out = np.zeros(len(regions), dtype=np.float64)
    for r in range(len(regions)):
        n_p, n_g, both = c[0][r], c[1][r], c[2][r]
        out[r] = _dice(n_p, n_g, both) if n_p > 0 and n_g > 0 else (1.0 if n_p == 0 and n_g == 0 else 0.0)
    return out


def evaluate(cases: Iterable, regions: Sequence[Sequence[int]] = BRATS_REGIONS, max_regions: Optional[int] = L.METRICS_MAX_REGIONS):
    """cases: an iterable of (pred_labels, gt_labels) or (pred_labels, gt_labels, voxelspacing).  -> (results (n, n_regions, 2), their
    mean over the cases, their standard deviation): what 5_compute_metrics.py:76-84 saves and prints.  `max_regions`: see
    `case_metrics`."""
    rows = []
    for case in cases:
        spacing = case[2] if len(case) > 2 else (1, 1, 1)
        rows.append(case_metrics(case[0], case[1], spacing, regions, max_regions))
    results = np.stack(rows) if rows else np.zeros((0, len(regions), 2))
    if not rows:
        return results, np.full((len(regions), 2), np.nan), np.full((len(regions), 2), np.nan)
    return results, results.mean(axis=0), results.std(axis=0)


# ---- the evaluation report: medpy's asd / assd, the surface Dice, and the metric table of light_training/evaluation/metric.py ------------
def _binary_summary(result, reference, voxelspacing, tolerance, what) -> SurfaceSummary:
    return _binary_pass(result, reference, what).summary([0], voxelspacing, tolerance)[0]


def asd(result, reference, voxelspacing: Optional[Sequence[float]] = None) -> float:
    """Average surface distance: the mean of `surface_distances(result, reference)`, added in fp64 (medpy.metric.binary.asd,
    connectivity 1).  Not symmetric.  Raises RuntimeError when either volume is empty, as medpy does."""
    return _binary_summary(result, reference, voxelspacing, None, "asd").asd_pg


def assd(result, reference, voxelspacing: Optional[Sequence[float]] = None) -> float:
    """Average symmetric surface distance: the mean of asd(result, reference) and asd(reference, result) (medpy.metric.binary.assd)"""
    s = _binary_summary(result, reference, voxelspacing, None, "assd")
    return (s.asd_pg + s.asd_gp) / 2.0


def nsd(result, reference, tolerance: float, voxelspacing: Optional[Sequence[float]] = None) -> float:
    """Surface Dice at `tolerance`, VOXEL-COUNTED: the number of border voxels of `result` within `tolerance` of the border of
    `reference`, plus the number of border voxels of `reference` within `tolerance` of the border of `result`, over the number of
    border voxels of both.  Every border voxel weighs 1: this is not the surface-area-weighted form, which weighs a voxel by the
    area of its surface patch under the spacing.  Raises RuntimeError when either volume is empty."""
    if not float(tolerance) >= 0.0:
        raise RuntimeError(f"nsd: a tolerance >= 0 is required, got {tolerance}")
    return _binary_summary(result, reference, voxelspacing, tolerance, "nsd").nsd


_Confusion = namedtuple("_Confusion", "tp fp tn fn")


def _confusion(n_p: int, n_g: int, both: int, voxels: int) -> _Confusion:
    return _Confusion(both, n_p - both, voxels - n_p - n_g + both, n_g - both)


def _none(nan: bool) -> float:
    return math.nan if nan else 0.0


# the four existence flags of the reference's ConfusionMatrix, from counts: empty = no voxel set, full = every voxel set
def _test_empty(c): return c.tp + c.fp == 0
def _test_full(c): return c.tn + c.fn == 0
def _ref_empty(c): return c.tp + c.fn == 0
def _ref_full(c): return c.tn + c.fp == 0


def _m_dice(c, nan): return _none(nan) if _test_empty(c) and _ref_empty(c) else float(2.0 * c.tp / (2 * c.tp + c.fp + c.fn))
def _m_jaccard(c, nan): return _none(nan) if _test_empty(c) and _ref_empty(c) else float(c.tp / (c.tp + c.fp + c.fn))
def _m_precision(c, nan): return _none(nan) if _test_empty(c) else float(c.tp / (c.tp + c.fp))
def _m_recall(c, nan): return _none(nan) if _ref_empty(c) else float(c.tp / (c.tp + c.fn))
def _m_specificity(c, nan): return _none(nan) if _ref_full(c) else float(c.tn / (c.tn + c.fp))
def _m_accuracy(c, nan): return float((c.tp + c.tn) / (c.tp + c.fp + c.tn + c.fn))
def _m_for(c, nan): return _none(nan) if _test_full(c) else float(c.fn / (c.fn + c.tn))


def _m_fscore(c, nan, beta=1.0):
    p, r = _m_precision(c, nan), _m_recall(c, nan)
    den = (beta * beta * p) + r
    return math.nan if den == 0.0 else (1 + beta * beta) * p * r / den          # no true positive: NaN where the reference divides by zero


_COUNT_METRICS = {
    "False Positive Rate": lambda c, nan: 1 - _m_specificity(c, nan),
    "Dice": _m_dice,
    "Jaccard": _m_jaccard,
    "Precision": _m_precision,
    "Recall": _m_recall,
    "Accuracy": _m_accuracy,
    "False Omission Rate": _m_for,
    "Negative Predictive Value": lambda c, nan: 1 - _m_for(c, nan),
    "False Negative Rate": lambda c, nan: 1 - _m_recall(c, nan),
    "True Negative Rate": _m_specificity,
    "False Discovery Rate": lambda c, nan: 1 - _m_precision(c, nan),
    "Total Positives Test": lambda c, nan: c.tp + c.fp,
    "Total Negatives Test": lambda c, nan: c.tn + c.fn,
    "Total Positives Reference": lambda c, nan: c.tp + c.fn,
    "total Negatives Reference": lambda c, nan: c.tn + c.fp,
}
_SURFACE_METRICS = {
    "Hausdorff Distance": lambda s: s.hd,
    "Hausdorff Distance 95": lambda s: s.hd95,
    "Avg. Symmetric Surface Distance": lambda s: (s.asd_pg + s.asd_gp) / 2.0,
    "Avg. Surface Distance": lambda s: s.asd_pg,
    "Surface Dice": lambda s: s.nsd,
}


def case_report(pred_labels, gt_labels, voxelspacing: Optional[Sequence[float]] = (1, 1, 1),
                regions: Sequence[Sequence[int]] = BRATS_REGIONS, metrics: Optional[Sequence[str]] = None, tolerance: float = 1.0,
                nan_for_nonexisting: bool = True) -> Dict[str, np.ndarray]:
    """The metric table of light_training/evaluation/metric.py per region of two label volumes: {name: float64 (n_regions,)} for the
    names of `metrics` (default: all of `ALL_METRICS`, i.e. the reference's 19 and "Surface Dice", the voxel-counted `nsd` at
    `tolerance`).  The count entries follow the reference's formulas and `nan_for_nonexisting` rules on tp / fp / tn / fn.  The four
    surface entries and "Surface Dice" are NaN (0 with nan_for_nonexisting=False) for a region whose prediction or ground truth is
    empty or fills the volume; elsewhere "Hausdorff Distance 95" and "Dice" equal `case_metrics` bit for bit.  Any number of regions,
    eight per kernel call; when `metrics` names no surface entry only the region pass runs."""
    names = list(ALL_METRICS) if metrics is None else [str(m) for m in metrics]
    unknown = [m for m in names if m not in ALL_METRICS]
    if unknown:
        raise RuntimeError(f"case_report: unknown metrics {unknown}; the names are {list(ALL_METRICS)}")
    if not float(tolerance) >= 0.0:
        raise RuntimeError(f"case_report: a tolerance >= 0 is required, got {tolerance}")
    pred, gt = _pair(pred_labels, gt_labels, _labels, "case_report")
    if len(regions) > L.METRICS_MAX_REGIONS:                              # eight at a time, concatenated
        parts = [case_report(pred, gt, voxelspacing, g, names, tolerance, nan_for_nonexisting) for g in _groups(regions)]
        return {m: np.concatenate([p[m] for p in parts]) for m in names}
    n = len(regions)
    surface = [m for m in names if m in _SURFACE_METRICS]
    if surface:
        p = _Pass(pred, gt, regions)
        counts = p.counts
    else:
        _, c = ops_raw.seg_regions(L.get_lib(), pred, gt, _table(regions, pred.device))
        counts = c[:, :n].tolist()
    cms = [_confusion(counts[0][r], counts[1][r], counts[2][r], pred.numel()) for r in range(n)]
    out = {m: np.full(n, _none(nan_for_nonexisting), dtype=np.float64) for m in names}
    for m in names:
        if m in _COUNT_METRICS:
            out[m][:] = [_COUNT_METRICS[m](c, nan_for_nonexisting) for c in cms]
    if surface:
        live = [r for r, c in enumerate(cms) if not (_test_empty(c) or _test_full(c) or _ref_empty(c) or _ref_full(c))]
        for r, s in zip(live, p.summary(live, voxelspacing, tolerance)):
            for m in surface:
                out[m][r] = _SURFACE_METRICS[m](s)
    return out


def confusion(pred, gt) -> Tuple[int, int, int, int]:
    """(tp, fp, tn, fn) of two binary volumes (non-zero = inside), from the counts of one region pass"""
    a, b = _pair(pred, gt, _mask, "confusion")
    _, counts = ops_raw.seg_regions(L.get_lib(), a, b, _table(_BINARY, a.device))
    c = counts[:, 0].tolist()
    return tuple(_confusion(c[0], c[1], c[2], a.numel()))


def _binary_metric(name):
    count = name in _COUNT_METRICS

    def fn(test, reference, nan_for_nonexisting: bool = True, voxel_spacing: Optional[Sequence[float]] = None, tolerance: float = 1.0):
        a, b = _pair(test, reference, _mask, name)
        v = case_report(a, b, voxel_spacing, _BINARY, [name], tolerance, nan_for_nonexisting)[name][0]
        return int(v) if name.lower().startswith("total") else float(v)
    fn.__doc__ = (f'"{name}" of two binary volumes as light_training/evaluation/metric.py defines it'
                  + (" (counts only)" if count else " (connectivity 1; NaN, or 0, when either volume is empty or full)"))
    return fn


ALL_METRICS = {name: _binary_metric(name) for name in (
    "False Positive Rate", "Dice", "Jaccard", "Hausdorff Distance", "Hausdorff Distance 95", "Precision", "Recall",
    "Avg. Symmetric Surface Distance", "Avg. Surface Distance", "Accuracy", "False Omission Rate", "Negative Predictive Value",
    "False Negative Rate", "True Negative Rate", "False Discovery Rate", "Total Positives Test", "Total Negatives Test",
    "Total Positives Reference", "total Negatives Reference", "Surface Dice")}

# one function per name of the reference's module
false_positive_rate = ALL_METRICS["False Positive Rate"]
dice = ALL_METRICS["Dice"]
jaccard = ALL_METRICS["Jaccard"]
hausdorff_distance = ALL_METRICS["Hausdorff Distance"]
hausdorff_distance_95 = ALL_METRICS["Hausdorff Distance 95"]
precision = ALL_METRICS["Precision"]
recall = sensitivity = ALL_METRICS["Recall"]
avg_surface_distance_symmetric = ALL_METRICS["Avg. Symmetric Surface Distance"]
avg_surface_distance = ALL_METRICS["Avg. Surface Distance"]
accuracy = ALL_METRICS["Accuracy"]
false_omission_rate = ALL_METRICS["False Omission Rate"]
negative_predictive_value = ALL_METRICS["Negative Predictive Value"]
false_negative_rate = ALL_METRICS["False Negative Rate"]
true_negative_rate = specificity = ALL_METRICS["True Negative Rate"]
false_discovery_rate = ALL_METRICS["False Discovery Rate"]
total_positives_test = ALL_METRICS["Total Positives Test"]
total_negatives_test = ALL_METRICS["Total Negatives Test"]
total_positives_reference = ALL_METRICS["Total Positives Reference"]
total_negatives_reference = ALL_METRICS["total Negatives Reference"]
surface_dice = ALL_METRICS["Surface Dice"]


def fscore(test, reference, nan_for_nonexisting: bool = True, beta: float = 1.0) -> float:
    """(1 + b^2) precision recall / (b^2 precision + recall); NaN where that is 0 / 0 (no true positive)"""
    return _m_fscore(_Confusion(*confusion(test, reference)), nan_for_nonexisting, float(beta))


def evaluate_report(cases: Iterable, regions: Sequence[Sequence[int]] = BRATS_REGIONS, metrics: Optional[Sequence[str]] = None,
                    tolerance: float = 1.0, nan_for_nonexisting: bool = True):
    """cases: an iterable of (pred_labels, gt_labels) or (pred_labels, gt_labels, voxelspacing).  -> ({name: (n_cases, n_regions)},
    {name: (n_regions,)}): `case_report` per case, and per region the mean over the cases that have a value (numpy.nanmean; NaN
    where no case has one)."""
    names = list(ALL_METRICS) if metrics is None else [str(m) for m in metrics]
    rows = []
    for case in cases:
        spacing = case[2] if len(case) > 2 else (1, 1, 1)
        rows.append(case_report(case[0], case[1], spacing, regions, names, tolerance, nan_for_nonexisting))
    per_case = {m: np.stack([r[m] for r in rows]) if rows else np.zeros((0, len(regions))) for m in names}
    mean = {}
    for m, a in per_case.items():
        have = ~np.isnan(a)
        cnt = have.sum(axis=0)
        mean[m] = np.where(cnt > 0, np.where(have, a, 0.0).sum(axis=0) / np.maximum(cnt, 1), np.nan)
    return per_case, mean
