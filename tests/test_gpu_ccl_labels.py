"""Labelled connected components (csrc/ccl_roots.hip, csrc/ccl_labels.hip) and what is built on them, on the HIP library: the checks of
tests/test_emu_ccl_labels.py on the GPU, plus one 96 x 160 x 160 ten-class volume against the per-class loop of the binary entries."""
import pytest
import torch

from tests import ccl_labels_checks as K
from tests import ccl_labels_ref as LR
from segmamba_amd import lib as L
from segmamba_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("case", sorted(LR.CASES))
def test_label_roots(hip, case):
    K.check_roots(hip, DEV, case)


def test_label_roots_equal_scipy_per_class(hip):
    pytest.importorskip("scipy.ndimage")
    for case in ("stripes_x", "checker_4x6x66", "crossing_17x70x131", "33x47x21", "ten_class_20x30x70", "tie"):
        K.check_roots(hip, DEV, case, with_scipy=True)


def test_stripes_and_checkerboard_winners(hip):
    K.check_known_winners(hip, DEV)


@pytest.mark.parametrize("case", sorted(LR.CASES))
def test_label_selection_and_info(hip, case):
    K.check_selection(hip, DEV, case)


def test_tie_rule_per_label(hip):
    K.check_tie(hip, DEV)


def test_apply_table_passes_labels_through(hip):
    K.check_apply(hip, DEV)


@pytest.mark.parametrize("case", ["ten_class_20x30x70", "33x47x21", "40x48x36", "shell_around_ball", "crossing_17x70x131", "all_zero"])
def test_keep_largest_per_class_equals_the_per_class_loop(hip, case):
    K.check_against_parent_route(hip, DEV, LR.case(case)[0])


def test_ten_classes_96x160x160_against_the_per_class_loop(hip):
    """2.5 M voxels, 150 tiles along y and z: roots per class against the binary entry, the kept label map (and the filled one) against
    the per-class loop, the summary against the loop's counts; two calls bit-equal"""
    lab = LR.ten_class((96, 160, 160), seed=3)
    t = K.dev_t(lab, DEV)
    roots = PP.label_component_roots(t)
    assert torch.equal(roots, PP.label_component_roots(t))
    assert bool((roots[t == 0] == -1).all())
    summary = PP.class_component_summary(t)
    assert sorted(summary) == list(range(1, 10))
    for c in range(1, 10):
        m = t == c
        assert torch.equal(roots[m], PP.component_roots(m.to(torch.uint8))[m]), c
        assert summary[c] == PP.component_summary(m.to(torch.uint8)), c
        assert summary[c][0] >= 3                                         # a condition on the input: the blob and islands or speckle
    for fill in (False, True):
        got = PP.keep_largest_per_class(t, fill_holes=fill)
        assert torch.equal(got, K.parent_route(hip, t, fill)), fill
        assert torch.equal(got, PP.keep_largest_per_class(t, fill_holes=fill))


def test_argmax_10_and_32_classes(hip):
    K.check_argmax_many_classes(hip, DEV)
    K.check_argmax_many_classes(hip, DEV, shape=(6, 9, 128))


def test_argmax_10_classes_resampled_band_rule(hip):
    K.check_argmax_resampled_10(hip, DEV)


def test_argmax_class_bounds(hip):
    K.check_argmax_refusals(hip, DEV)


def test_wrapper_refusals(hip):
    K.check_refusals(hip, DEV)


def test_c_refusals_launch_nothing(hip):
    K.check_c_refusals(hip, DEV)


def test_new_exports_in_the_hip_library(hip):
    K.check_exports(hip)


def test_save_organs_to_nii(hip, tmp_path):
    K.check_save_organs(DEV, tmp_path)


def test_finish_predictions_per_class_and_organs(hip, tmp_path):
    K.check_tools(DEV, tmp_path)


def test_metrics_with_nine_regions(hip, monkeypatch):
    K.check_metrics_groups(DEV, monkeypatch)
