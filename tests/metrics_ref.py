"""The reference of the evaluation tests: medpy's definitions of Dice / surface distances / HD95 restated with numpy only
(TEST INFRASTRUCTURE).  Borders by padded shifts, distances by brute force over coordinate pairs in integer (unit spacing) or
fp64 arithmetic, the percentile by numpy.percentile.  The `scipy_*` functions state the same with scipy.ndimage where it imports.

Also the case builders shared by tests/test_emu_metrics.py and tests/test_gpu_metrics.py."""
import numpy as np

BRATS_REGIONS = ((1, 3), (1, 2, 3), (3,))


def region_mask(labels, region):
    return np.isin(labels, np.asarray(region))


def border(mask):
    """mask ^ binary_erosion(mask, connectivity-1 cross, border_value=0): inside, and one of the six face neighbours (the outside of
    the volume included) is not"""
    m = np.pad(mask.astype(bool), 1, constant_values=False)
    c = m[1:-1, 1:-1, 1:-1]
    inner = (c & m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:])
    return c & ~inner


def fp32_spacing(spacing):
    """the spacing as the kernels see it: rounded to fp32, then exact in fp64"""
    return np.asarray(spacing, dtype=np.float32).astype(np.float64)


def min_sq_dist(points, targets, spacing=None, chunk=512):
    """for every row of `points` (n, 3 integer coordinates) the smallest squared distance to a row of `targets`: int64 for unit spacing,
    fp64 (spacing rounded to fp32) otherwise"""
    points, targets = np.asarray(points, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    unit = spacing is None or all(float(s) == 1.0 for s in spacing)
    out = np.empty(len(points), dtype=np.int64 if unit else np.float64)
    sp = None if unit else fp32_spacing(spacing)
    for i in range(0, len(points), chunk):
        d = points[i:i + chunk, None, :] - targets[None, :, :]
        if unit:
            out[i:i + chunk] = (d * d).sum(-1).min(1)
        else:
            t = d.astype(np.float64) * sp
            out[i:i + chunk] = (t * t).sum(-1).min(1)
    return out


def edt_sq(set_mask, spacing=None):
    """squared distance of EVERY voxel to the nearest set voxel of `set_mask`, brute force (set_mask must not be empty)"""
    targets = np.argwhere(set_mask)
    assert len(targets) > 0
    points = np.argwhere(np.ones(set_mask.shape, dtype=bool))
    return min_sq_dist(points, targets, spacing).reshape(set_mask.shape)


def surface_distances(result, reference, spacing=None):
    """medpy's __surface_distances (connectivity 1) in fp64, in the memory order of the border voxels of `result`"""
    a, b = np.asarray(result).astype(bool), np.asarray(reference).astype(bool)
    if not a.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not b.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return np.sqrt(min_sq_dist(np.argwhere(border(a)), np.argwhere(border(b)), spacing).astype(np.float64))


def dc(result, reference):
    a, b = np.asarray(result).astype(bool), np.asarray(reference).astype(bool)
    n = int(a.sum()) + int(b.sum())
    return 2.0 * int((a & b).sum()) / float(n) if n else 0.0


def joined(result, reference, spacing=None):
    return np.hstack((surface_distances(result, reference, spacing), surface_distances(reference, result, spacing)))


def hd95(result, reference, spacing=None):
    return float(np.percentile(joined(result, reference, spacing), 95))


def hd(result, reference, spacing=None):
    return float(joined(result, reference, spacing).max())


def cal_metric(gt, pred, spacing):
    """5_compute_metrics.py:24-30"""
    if pred.sum() > 0 and gt.sum() > 0:
        return np.array([dc(pred, gt), hd95(pred, gt, spacing)])
    return np.array([0.0, 50])


def case_metrics(pred_labels, gt_labels, spacing=(1, 1, 1), regions=BRATS_REGIONS):
    return np.stack([cal_metric(region_mask(gt_labels, r), region_mask(pred_labels, r), spacing) for r in regions])


def validation_dice(pred_labels, gt_labels, regions=BRATS_REGIONS):
    """3_train.py:82-91"""
    out = []
    for r in regions:
        p, g = region_mask(pred_labels, r), region_mask(gt_labels, r)
        out.append(dc(p, g) if p.any() and g.any() else (1.0 if not p.any() and not g.any() else 0.0))
    return np.array(out)


def counts(pred_labels, gt_labels, regions=BRATS_REGIONS):
    """(5, n_regions): |P|, |G|, |P and G|, |border P|, |border G|"""
    rows = []
    for r in regions:
        p, g = region_mask(pred_labels, r), region_mask(gt_labels, r)
        rows.append([p.sum(), g.sum(), (p & g).sum(), border(p).sum(), border(g).sum()])
    return np.asarray(rows, dtype=np.int64).T


def border_planes(labels, regions=BRATS_REGIONS):
    out = np.zeros(labels.shape, dtype=np.uint8)
    for r, reg in enumerate(regions):
        out |= (border(region_mask(labels, reg)).astype(np.uint8) << r)
    return out


# ---- the same with scipy.ndimage (callers importorskip) -------------------------------------------------------------------------
def scipy_border(mask):
    from scipy.ndimage import binary_erosion, generate_binary_structure
    mask = np.asarray(mask).astype(bool)
    return mask ^ binary_erosion(mask, structure=generate_binary_structure(3, 1), iterations=1)


def scipy_edt_sq_int(set_mask):
    """exact integer squared distances at unit spacing: scipy returns fp64 distances whose squares round to the integers"""
    from scipy.ndimage import distance_transform_edt
    return np.rint(distance_transform_edt(~np.asarray(set_mask).astype(bool)) ** 2).astype(np.int64)


def scipy_surface_distances(result, reference, spacing=None):
    from scipy.ndimage import distance_transform_edt
    dt = distance_transform_edt(~scipy_border(reference), sampling=None if spacing is None else fp32_spacing(spacing))
    return dt[scipy_border(result)]


def scipy_hd95(result, reference, spacing=None):
    return float(np.percentile(np.hstack((scipy_surface_distances(result, reference, spacing),
                                          scipy_surface_distances(reference, result, spacing))), 95))


# ---- cases -------------------------------------------------------------------------------------------------------------------------
def _ellipsoid(shape, centre, radii, ripple=0.0, k=5):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij", sparse=True)
    dz, dy, dx = (z - centre[0]) / radii[0], (y - centre[1]) / radii[1], (x - centre[2]) / radii[2]
    r = np.sqrt(dz * dz + dy * dy + dx * dx)
    if ripple:
        phi = np.arctan2(dy, dx + 1e-9)
        theta = np.arccos(np.clip(dz / np.maximum(r, 1e-9), -1.0, 1.0))
        return r <= 1.0 + ripple * np.sin(k * phi) * np.cos(k * theta)
    return r <= 1.0


def nested_labels(shape, centre, radii, ripple=0.1, scale=1.0, lobe=True, inner=(0.65, 0.42)):
    """BraTS-like labels: label 2 (the outer shell of WT), label 1 inside it, label 3 (ET) innermost, plus a second lobe of labels 2 / 1"""
    lab = np.zeros(shape, dtype=np.uint8)
    r = np.asarray(radii, dtype=np.float64) * scale
    lab[_ellipsoid(shape, centre, r, ripple)] = 2
    lab[_ellipsoid(shape, centre, r * inner[0], ripple)] = 1
    lab[_ellipsoid(shape, centre, r * inner[1], ripple)] = 3
    if lobe:
        c2 = (centre[0] + 0.5 * r[0], centre[1] - 0.9 * r[1], centre[2] + 0.6 * r[2])
        lab[_ellipsoid(shape, c2, r * 0.45) & (lab == 0)] = 2
        lab[_ellipsoid(shape, c2, r * 0.25)] = 1
    return lab


def small_case(shape, shift=(1, -2, 1), island=True):
    """(pred, gt) label volumes of a few 10^4 voxels with odd sides: nested rippled ellipsoids, the prediction shifted and shrunk, two
    disconnected extra pieces, and (island) a 2^3 block of label 3 in the corner opposite to everything else"""
    D, H, W = shape
    c = (0.55 * D, 0.55 * H, 0.5 * W)
    rad = (0.3 * D, 0.3 * H, 0.34 * W)
    gt = nested_labels(shape, c, rad)
    pred = nested_labels(shape, tuple(ci + s for ci, s in zip(c, shift)), rad, scale=0.93)
    gt[-3:, -4:-1, 1:3][gt[-3:, -4:-1, 1:3] == 0] = 1                  # a separate piece that touches the z = D - 1 face
    if island:
        pred[:2, :2, :2] = 3
    return pred, gt


def full_case(shape):
    """a region that touches every face of the volume (the border_value = 0 rule): gt is label 2 everywhere with a core of 1 / 3"""
    gt = np.full(shape, 2, dtype=np.uint8)
    pred = np.full(shape, 2, dtype=np.uint8)
    D, H, W = shape
    gt[D // 3:D // 3 + 3, H // 3:H // 3 + 4, W // 3:W // 3 + 3] = 3
    gt[D // 3 + 3:D // 3 + 5, H // 3:H // 3 + 4, W // 3:W // 3 + 3] = 1
    pred[D // 3 + 1:D // 3 + 4, H // 3 + 1:H // 3 + 4, W // 3:W // 3 + 4] = 3
    pred[0, 0, :] = 0
    pred[-1, -1, -1] = 1
    return pred, gt


def brats_size_case():
    """(pred, gt) at 155 x 240 x 240: three nested rippled ellipsoids and a second lobe; the prediction is the same shifted by (2, -3, 4)
    and scaled 0.95, plus a 4^3 false-positive island of label 3 in the corner"""
    shape = (155, 240, 240)
    c, rad = (75.0, 120.0, 125.0), (38.0, 50.0, 46.0)
    gt = nested_labels(shape, c, rad, ripple=0.12, inner=(0.65, 0.55))
    pred = nested_labels(shape, (c[0] + 2, c[1] - 3, c[2] + 4), rad, ripple=0.12, scale=0.95, inner=(0.65, 0.55))
    pred[:4, :4, :4] = 3
    return pred, gt
