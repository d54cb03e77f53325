"""Surface statistics without a distance list (csrc/surface_stats.hip) and the evaluation report of segmamba_amd/metrics.py, with the
kernel sources compiled for the CPU emulator.  `segm_border_stats` is held to the list route exactly (border_distances + torch.sort on
the same distance transform); the host functions to tests/surface_ref.py.  The same checks run on the HIP library in
tests/test_gpu_surface.py."""
import pytest

from tests import emu_util
from tests import surface_checks as C
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.metrics on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("spacing", C.SPACINGS)
@pytest.mark.parametrize("case", C.ENTRY_CASES)
def test_border_stats_equal_the_list_route_emulated(emu, case, spacing):
    """6 items, 3 groups: counts, maxima, within-counts at tau 0 / 1 / 2.5 and both ranks equal the sorted lists; the fp64 sum within
    2 n 2^-53; two calls bit-equal"""
    got = C.check_entry_on_case(emu, "cpu", case, spacing)
    if case == "wide_row" and spacing is None:                            # ET: the two ranks differ in the second radix digit
        assert got[4 * C.W + 4:4 * C.W + 6] == pytest.approx([11.045361, 53.235325], rel=1e-6)


@pytest.mark.parametrize("spacing", [None, C.ANISO[0]])
def test_upper_radix_digits_and_rank_edges_emulated(emu, spacing):
    """squared keys above 2^16 (int32) and fp32 keys that use every digit; the ends of the list, ranks out of range, a group of one
    voxel, tolerance < 0"""
    C.check_upper_digits(emu, "cpu", spacing)


@pytest.mark.parametrize("shape,spacing", [((3, 5, 7), None), ((5, 7, 150), None), ((4, 8, 130), C.ANISO[0]), ((1, 1, 1), None),
                                           ((2, 3, 300), C.ANISO[1])])
def test_layout_emulated(emu, shape, spacing):
    """105, 5250 (beyond the 4096 voxels of a workgroup's packet row, no multiple of 16: the second volume starts at an odd address),
    4160 (a multiple of 16: packets in both volumes), 1 and 1800 voxels; 1 item and 16 items; an item and a group with nothing in them"""
    C.check_layout(emu, "cpu", shape, spacing)


@pytest.mark.parametrize("mode", ["", "box", "1"])
@pytest.mark.parametrize("case,spacing", [("33x47x21", (1, 1, 1)), ("wide_row", C.ANISO[0]), ("touches_every_face", (1, 1, 1)),
                                          ("1x1x1", (1, 1, 1))])
def test_report_equals_case_metrics_and_hd_emulated(product, monkeypatch, case, spacing, mode):
    monkeypatch.setenv("SEGM_EDT_LONG", mode)
    C.check_report_equals_case_metrics("cpu", case, spacing)


@pytest.mark.parametrize("case,spacing", [("33x47x21", None), ("40x48x36", C.ANISO[1]), ("slab", C.ANISO[0]), ("wide_row", None),
                                          ("33x47x21", C.ANISO[0])])
def test_report_against_the_reference_emulated(product, case, spacing):
    """asd / assd and the report's surface columns within 2^-23 (unit spacing) or 1e-6 (fp32 transform) of fp64 brute force; nsd and
    the confusion family exactly"""
    C.check_report_against_reference("cpu", case, spacing)


def test_report_against_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    import numpy as np
    from segmamba_amd import metrics as M
    from tests import metrics_checks as K
    from tests import surface_ref as S
    pred, gt = K.LABEL_CASES["33x47x21"]()
    got = M.case_report(pred, gt, None, tolerance=2.5)
    C.compare_report(got, S.case_report(pred, gt, None, tolerance=2.5, scipy=True), None)
    assert np.isfinite(got["Avg. Surface Distance"]).all()


def test_thin_volume_through_the_box_route_emulated(product):
    C.check_thin_host("cpu", None)
    C.check_thin_host("cpu", C.ANISO[0])


def test_existence_rules_emulated(product):
    C.check_existence_rules("cpu")


def test_ten_regions_in_groups_emulated(product):
    C.check_ten_regions("cpu")


def test_count_entries_launch_the_region_pass_only_emulated(product, monkeypatch):
    C.check_counts_only_launch_nothing_else("cpu", monkeypatch)


def test_evaluate_report_emulated(product):
    C.check_evaluate_report("cpu")


def test_report_tool_emulated(product, tmp_path):
    C.check_report_tool("cpu", tmp_path)


def test_refusals_emulated(product):
    C.check_refusals(product, "cpu")


def test_exports_emulated(emu):
    C.check_exports(emu)
