"""Surface statistics without a distance list (csrc/surface_stats.hip) and the evaluation report on the HIP library: the checks of
tests/test_emu_surface.py on the GPU, plus one case at BraTS size (545 steps of 4 x 4096 voxels: more than the 512 workgroups of an
item, so the grid stride is taken)."""
import numpy as np
import pytest

from tests import metrics_checks as K
from tests import metrics_ref as R
from tests import surface_checks as C
from segmamba_amd import lib as L
from segmamba_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("spacing", C.SPACINGS)
@pytest.mark.parametrize("case", C.ENTRY_CASES)
def test_border_stats_equal_the_list_route(hip, case, spacing):
    C.check_entry_on_case(hip, DEV, case, spacing)


@pytest.mark.parametrize("spacing", [None, C.ANISO[0]])
def test_upper_radix_digits_and_rank_edges(hip, spacing):
    C.check_upper_digits(hip, DEV, spacing)


@pytest.mark.parametrize("shape,spacing", [((3, 5, 7), None), ((5, 7, 150), None), ((4, 8, 130), C.ANISO[0]), ((1, 1, 1), None),
                                           ((2, 3, 300), C.ANISO[1])])
def test_layout(hip, shape, spacing):
    C.check_layout(hip, DEV, shape, spacing)


@pytest.mark.parametrize("mode", ["", "box", "1"])
@pytest.mark.parametrize("case,spacing", [("33x47x21", (1, 1, 1)), ("wide_row", C.ANISO[0]), ("touches_every_face", (1, 1, 1)),
                                          ("1x1x1", (1, 1, 1))])
def test_report_equals_case_metrics_and_hd(hip, monkeypatch, case, spacing, mode):
    monkeypatch.setenv("SEGM_EDT_LONG", mode)
    C.check_report_equals_case_metrics(DEV, case, spacing)


@pytest.mark.parametrize("case,spacing", [("33x47x21", None), ("40x48x36", C.ANISO[1]), ("slab", C.ANISO[0]), ("wide_row", None),
                                          ("33x47x21", C.ANISO[0])])
def test_report_against_the_reference(hip, case, spacing):
    C.check_report_against_reference(DEV, case, spacing)


def test_thin_volume_through_the_box_route(hip):
    C.check_thin_host(DEV, None)
    C.check_thin_host(DEV, C.ANISO[0])


def test_existence_rules(hip):
    C.check_existence_rules(DEV)


def test_ten_regions_in_groups(hip):
    C.check_ten_regions(DEV)


def test_count_entries_launch_the_region_pass_only(hip, monkeypatch):
    C.check_counts_only_launch_nothing_else(DEV, monkeypatch)


def test_evaluate_report(hip):
    C.check_evaluate_report(DEV)


def test_report_tool(hip, tmp_path):
    C.check_report_tool(DEV, tmp_path)


def test_refusals(hip):
    C.check_refusals(hip, DEV)


def test_exports_in_the_hip_library(hip):
    C.check_exports(hip)


# ---- at BraTS size ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brats():
    pred, gt = R.brats_size_case()
    return K.dev_t(pred, DEV), K.dev_t(gt, DEV)


@pytest.mark.parametrize("spacing", [(1, 1, 1), (1.0, 1.2, 0.9)])
def test_brats_size_report(hip, brats, spacing):
    """155 x 240 x 240 (tests/metrics_ref.brats_size_case): the report's Dice, HD95 and HD columns equal case_metrics / hd bit for bit;
    ASD within 2^-23 (unit spacing) or 1e-6 (fp32 transform) of the fp64 mean of `surface_distances`; two calls bit-equal"""
    tp, tg = brats
    sp = None if all(s == 1 for s in spacing) else spacing
    got = M.case_report(tp, tg, spacing)
    cm = M.case_metrics(tp, tg, spacing)
    tol = 2.0 ** -23 if sp is None else 1e-6
    for r, reg in enumerate(R.BRATS_REGIONS):
        a, b = M.region_masks(tp, (reg,))[0].to(tp.dtype), M.region_masks(tg, (reg,))[0].to(tg.dtype)
        want_asd = float(M.surface_distances(a, b, sp).double().mean())
        print("region", reg, "spacing", spacing, {m: v[r] for m, v in got.items()}, "case_metrics", cm[r].tolist(), "asd", want_asd)
        assert C.bits(got["Dice"][r]) == C.bits(cm[r, 0]) and C.bits(got["Hausdorff Distance 95"][r]) == C.bits(cm[r, 1])
        assert C.bits(got["Hausdorff Distance"][r]) == C.bits(M.hd(a, b, sp))
        assert abs(got["Avg. Surface Distance"][r] - want_asd) <= tol * want_asd
        assert 0.0 < got["Surface Dice"][r] < 1.0
    again = M.case_report(tp, tg, spacing)
    assert all(np.array_equal(got[m], again[m]) for m in got)
