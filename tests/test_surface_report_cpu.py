"""tests/golden/eval_report.npz - the output of the reference's own light_training/evaluation/metric.py (its ConfusionMatrix and the
19 functions of ALL_METRICS; tests/golden/make_golden_eval_report.py) - against the restatement in tests/surface_ref.py, and the
names of segmamba_amd.metrics.ALL_METRICS against the reference's.  No library is loaded: numpy only."""
import os

import numpy as np
import pytest

from tests import surface_ref as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eval_report.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_names_are_the_references(golden):
    from segmamba_amd import metrics as M
    names = [str(n) for n in golden["names"]]
    assert len(names) == 19 and "total Negatives Reference" in names
    assert names == list(S.REFERENCE_NAMES)
    assert list(M.ALL_METRICS) == names + ["Surface Dice"]
    assert set(S.COUNT_NAMES) | set(S.SURFACE_NAMES) == set(names)
    for fn in ("dice", "jaccard", "precision", "sensitivity", "recall", "specificity", "accuracy", "fscore", "false_positive_rate",
               "false_omission_rate", "false_negative_rate", "true_negative_rate", "false_discovery_rate", "negative_predictive_value",
               "total_positives_test", "total_negatives_test", "total_positives_reference", "total_negatives_reference",
               "hausdorff_distance", "hausdorff_distance_95", "avg_surface_distance", "avg_surface_distance_symmetric",
               "asd", "assd", "nsd", "confusion", "case_report", "evaluate_report"):
        assert callable(getattr(M, fn)), fn


def test_restatement_equals_the_references_output(golden):
    """every case, region, name and both settings of nan_for_nonexisting: NaN where the reference has NaN, else the same double"""
    cases = S.golden_cases()
    assert [c[0] for c in cases] == [str(c) for c in golden["cases"]]
    names = [str(n) for n in golden["names"]]
    assert golden["values"].shape == (2, len(cases), 3, 19)
    for k, nan in enumerate((True, False)):
        for c, (name, pred, gt, spacing) in enumerate(cases):
            got = S.case_report(pred, gt, spacing, nan_for_nonexisting=nan)
            for m, metric in enumerate(names):
                want = golden["values"][k, c, :, m]
                assert np.array_equal(got[metric], want, equal_nan=True), (name, metric, nan, got[metric].tolist(), want.tolist())


def test_golden_holds_the_existence_cases(golden):
    """what the fixture is for: all-empty, empty against non-empty, a full ground truth (touches_every_face WT) and 1 x 1 x 1"""
    names = [str(n) for n in golden["names"]]
    cases = [str(c) for c in golden["cases"]]
    v = golden["values"][0]
    hd95, dice, tnr = names.index("Hausdorff Distance 95"), names.index("Dice"), names.index("True Negative Rate")
    assert np.isnan(v[cases.index("all_empty"), :, dice]).all() and np.isnan(v[cases.index("all_empty"), :, hd95]).all()
    assert (v[cases.index("empty_pred"), :, dice] == 0).all() and np.isnan(v[cases.index("empty_pred"), :, hd95]).all()
    assert np.isnan(v[cases.index("empty_gt"), :, hd95]).all()
    full = v[cases.index("touches_every_face"), 1]
    assert np.isnan(full[hd95]) and np.isnan(full[tnr]) and full[dice] > 0.9
    assert np.isnan(v[cases.index("1x1x1"), :, hd95]).all()
    assert not np.isnan(v[cases.index("wide_row"), :, hd95]).any()
    assert (golden["values"][1][cases.index("all_empty"), :, hd95] == 0).all()
