"""The reference of the evaluation-report tests (TEST INFRASTRUCTURE): the metric table of light_training/evaluation/metric.py and
medpy's asd / assd restated in numpy float64 on tests/metrics_ref.py (borders by padded shifts, distances by brute force), the
voxel-counted surface Dice, and the same surface quantities with scipy.ndimage where it imports.  tests/golden/eval_report.npz pins
this restatement to the reference's own module (tests/golden/make_golden_eval_report.py runs it with `medpy.metric` shimmed onto the
functions `hd`, `hd95`, `asd`, `assd` below)."""
import numpy as np

from tests import metrics_ref as R

COUNT_NAMES = ("False Positive Rate", "Dice", "Jaccard", "Precision", "Recall", "Accuracy", "False Omission Rate",
               "Negative Predictive Value", "False Negative Rate", "True Negative Rate", "False Discovery Rate", "Total Positives Test",
               "Total Negatives Test", "Total Positives Reference", "total Negatives Reference")
SURFACE_NAMES = ("Hausdorff Distance", "Hausdorff Distance 95", "Avg. Symmetric Surface Distance", "Avg. Surface Distance")
REFERENCE_NAMES = ("False Positive Rate", "Dice", "Jaccard", "Hausdorff Distance", "Hausdorff Distance 95", "Precision", "Recall",
                   "Avg. Symmetric Surface Distance", "Avg. Surface Distance", "Accuracy", "False Omission Rate",
                   "Negative Predictive Value", "False Negative Rate", "True Negative Rate", "False Discovery Rate",
                   "Total Positives Test", "Total Negatives Test", "Total Positives Reference", "total Negatives Reference")
ALL_NAMES = REFERENCE_NAMES + ("Surface Dice",)


# ---- medpy.metric's four surface functions (connectivity 1 only) ---------------------------------------------------------------------
def hd(result, reference, voxelspacing=None, connectivity=1):
    assert connectivity == 1
    return R.hd(result, reference, voxelspacing)


def hd95(result, reference, voxelspacing=None, connectivity=1):
    assert connectivity == 1
    return R.hd95(result, reference, voxelspacing)


def asd(result, reference, voxelspacing=None, connectivity=1):
    assert connectivity == 1
    return float(R.surface_distances(result, reference, voxelspacing).mean())


def assd(result, reference, voxelspacing=None, connectivity=1):
    return float(np.mean((asd(result, reference, voxelspacing, connectivity), asd(reference, result, voxelspacing, connectivity))))


def nsd(result, reference, tolerance, voxelspacing=None):
    """voxel-counted: border voxels of either mask within `tolerance` of the other border, over all border voxels of both"""
    ab, ba = R.surface_distances(result, reference, voxelspacing), R.surface_distances(reference, result, voxelspacing)
    return float(((ab <= tolerance).sum() + (ba <= tolerance).sum()) / float(len(ab) + len(ba)))


def scipy_asd(result, reference, voxelspacing=None):
    return float(R.scipy_surface_distances(result, reference, voxelspacing).mean())


def scipy_nsd(result, reference, tolerance, voxelspacing=None):
    ab, ba = R.scipy_surface_distances(result, reference, voxelspacing), R.scipy_surface_distances(reference, result, voxelspacing)
    return float(((ab <= tolerance).sum() + (ba <= tolerance).sum()) / float(len(ab) + len(ba)))


# ---- the confusion family ----------------------------------------------------------------------------------------------------------
def confusion(test, reference):
    t, r = np.asarray(test) != 0, np.asarray(reference) != 0
    return int((t & r).sum()), int((t & ~r).sum()), int((~t & ~r).sum()), int((~t & r).sum())


def count_metrics(test, reference, nan_for_nonexisting=True):
    """{name: value} of the 15 entries that need tp / fp / tn / fn only, with the rules for masks that are empty or full"""
    t, r = np.asarray(test) != 0, np.asarray(reference) != 0
    tp, fp, tn, fn = confusion(t, r)
    none = float("nan") if nan_for_nonexisting else 0.0
    t_empty, t_full, r_empty, r_full = not t.any(), bool(t.all()), not r.any(), bool(r.all())
    prec = none if t_empty else tp / (tp + fp)
    rec = none if r_empty else tp / (tp + fn)
    spec = none if r_full else tn / (tn + fp)
    fom = none if t_full else fn / (fn + tn)
    return {
        "Dice": none if t_empty and r_empty else 2.0 * tp / (2 * tp + fp + fn),
        "Jaccard": none if t_empty and r_empty else tp / (tp + fp + fn),
        "Precision": prec, "Recall": rec, "True Negative Rate": spec, "False Omission Rate": fom,
        "False Positive Rate": 1 - spec, "False Negative Rate": 1 - rec, "False Discovery Rate": 1 - prec,
        "Negative Predictive Value": 1 - fom,
        "Accuracy": (tp + tn) / (tp + fp + tn + fn),
        "Total Positives Test": tp + fp, "Total Negatives Test": tn + fn,
        "Total Positives Reference": tp + fn, "total Negatives Reference": tn + fp,
    }


def surface_metrics(test, reference, spacing=None, tolerance=1.0, nan_for_nonexisting=True, scipy=False):
    """{name: value} of the four surface entries and "Surface Dice": NaN (or 0) when either mask is empty or full"""
    t, r = np.asarray(test) != 0, np.asarray(reference) != 0
    names = SURFACE_NAMES + ("Surface Dice",)
    if not t.any() or t.all() or not r.any() or r.all():
        return {m: float("nan") if nan_for_nonexisting else 0.0 for m in names}
    if scipy:
        ab, ba = R.scipy_surface_distances(t, r, spacing), R.scipy_surface_distances(r, t, spacing)
    else:
        ab, ba = R.surface_distances(t, r, spacing), R.surface_distances(r, t, spacing)
    both = np.hstack((ab, ba))
    return {"Hausdorff Distance": float(both.max()), "Hausdorff Distance 95": float(np.percentile(both, 95)),
            "Avg. Surface Distance": float(ab.mean()), "Avg. Symmetric Surface Distance": float(np.mean((ab.mean(), ba.mean()))),
            "Surface Dice": float(((ab <= tolerance).sum() + (ba <= tolerance).sum()) / float(len(both)))}


def case_report(pred_labels, gt_labels, spacing=None, regions=R.BRATS_REGIONS, tolerance=1.0, nan_for_nonexisting=True, scipy=False):
    """{name: float64 (n_regions,)} for all 20 names"""
    out = {m: np.zeros(len(regions), dtype=np.float64) for m in ALL_NAMES}
    for i, reg in enumerate(regions):
        p, g = R.region_mask(pred_labels, reg), R.region_mask(gt_labels, reg)
        row = dict(count_metrics(p, g, nan_for_nonexisting))
        row.update(surface_metrics(p, g, spacing, tolerance, nan_for_nonexisting, scipy))
        for m in ALL_NAMES:
            out[m][i] = row[m]
    return out


# ---- the inputs of tests/golden/eval_report.npz, by generator arguments ------------------------------------------------------------
def golden_cases():
    """[(name, pred, gt, spacing)]: the label cases of tests/metrics_checks.py, an all-empty pair and empty against non-empty"""
    from tests import metrics_checks as K
    cases = []
    for name in ("33x47x21", "40x48x36", "slab", "wide_row", "touches_every_face", "1x1x1"):
        pred, gt = K.LABEL_CASES[name]()
        cases.append((name, pred, gt, None))
    pred, gt = K.LABEL_CASES["33x47x21"]()
    cases.append(("33x47x21_aniso0", pred, gt, K.ANISO[0]))
    pred, gt = K.LABEL_CASES["wide_row"]()
    cases.append(("wide_row_aniso1", pred, gt, K.ANISO[1]))
    pred, gt = R.small_case((21, 30, 25), island=False)
    cases.append(("all_empty", np.zeros_like(pred), np.zeros_like(gt), None))
    cases.append(("empty_pred", np.zeros_like(pred), gt, None))
    cases.append(("empty_gt", pred, np.zeros_like(gt), None))
    return cases
