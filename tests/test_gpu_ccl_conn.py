"""Connected components at connectivity 1, 2 and 3 (csrc/ccl_roots.hip) and what is built on them, on the HIP library: the checks of
tests/test_emu_ccl_conn.py on the GPU, plus one 96 x 160 x 160 ten-class volume at connectivity 3 against the per-class loop."""
import pytest
import torch

from tests import ccl_conn_checks as K
from tests import ccl_conn_ref as CR
from tests import ccl_labels_ref as LR
from tests.test_emu_ccl_conn import HOST_CASES, PER_CLASS_CASES
from segmamba_amd import lib as L
from segmamba_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("case", sorted(CR.MASKS))
def test_mask_roots(hip, case):
    K.check_mask(hip, DEV, case)


@pytest.mark.parametrize("case", sorted(CR.LABELS))
def test_label_roots(hip, case):
    K.check_labels(hip, DEV, case)


def test_legacy_entries_ignore_reserved(hip):
    K.check_legacy_entries_ignore_reserved(hip, DEV)


@pytest.mark.parametrize("case", HOST_CASES)
def test_host_functions_on_masks(hip, case):
    K.check_host_mask_functions(hip, DEV, case)


def test_label_equals_scipy(hip):
    pytest.importorskip("scipy.ndimage")
    K.check_label_equals_scipy(DEV, ["hand", "checker_5x6x66", "random_5x5x65_03", "random_9x10x131_06"])


def test_tie_rule_at_connectivity_2(hip):
    K.check_tie_rule(DEV)


def test_fill_holes_takes_the_background_connectivity(hip):
    K.check_fill_holes(DEV)


@pytest.mark.parametrize("case", PER_CLASS_CASES)
def test_keep_largest_per_class_equals_the_per_class_loop(hip, case):
    K.check_keep_largest_per_class(hip, DEV, case)


def test_diagonal_island_stays_at_connectivity_3(hip):
    K.check_diagonal_island(DEV)


def test_ten_classes_96x160x160_at_connectivity_3_against_the_per_class_loop(hip):
    """2.5 M voxels, 150 tiles along y and z: roots per class against the binary entry at c = 3, the kept label map (and the filled
    one) against the per-class loop, the summary against the loop's counts; two calls bit-equal; no more components than at c = 1"""
    lab = LR.ten_class((96, 160, 160), seed=3)
    t = K.dev_t(lab, DEV)
    roots = PP.label_component_roots(t, connectivity=3)
    assert torch.equal(roots, PP.label_component_roots(t, connectivity=3))
    assert bool((roots[t == 0] == -1).all())
    summary, faces = PP.class_component_summary(t, connectivity=3), PP.class_component_summary(t)
    assert sorted(summary) == list(range(1, 10))
    for c in range(1, 10):
        m = t == c
        assert torch.equal(roots[m], PP.component_roots(m.to(torch.uint8), connectivity=3)[m]), c
        assert summary[c] == PP.component_summary(m.to(torch.uint8), connectivity=3), c
        assert 3 <= summary[c][0] <= faces[c][0] and summary[c][1] >= faces[c][1]
    for fill in (False, True):
        got = PP.keep_largest_per_class(t, fill_holes=fill, connectivity=3)
        assert torch.equal(got, K.loop_route(hip, t, fill, 3)), fill
        assert torch.equal(got, PP.keep_largest_per_class(t, fill_holes=fill, connectivity=3))


def test_connectivity_outside_1_2_3_is_a_value_error(hip):
    K.check_value_errors(hip, DEV)


def test_c_refusals_launch_nothing(hip):
    K.check_c_refusals(hip, DEV)


def test_new_exports_in_the_hip_library(hip):
    K.check_exports(hip)


def test_predictor_passes_connectivity(hip, tmp_path):
    K.check_predictor(DEV, tmp_path)


def test_finish_predictions_connectivity(hip, tmp_path):
    K.check_tool(DEV, tmp_path)
