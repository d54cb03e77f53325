"""Labelled connected components (csrc/ccl_roots.hip, csrc/ccl_labels.hip), the per-class selection, the arg-max beyond 8 classes and the host functions on
top, with the kernel sources compiled for the CPU emulator.  References: tests/ccl_labels_ref.py (numpy; scipy.ndimage where it
imports).  The same checks run on the HIP library in tests/test_gpu_ccl_labels.py."""
import pytest

from tests import ccl_labels_checks as K
from tests import ccl_labels_ref as LR
from tests import emu_util
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.postprocess / metrics on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("case", sorted(LR.CASES))
def test_label_roots_emulated(product, case):
    """per class what the binary entry gives, -1 on the background, the numpy union-find per class, two calls bit-equal: stripes one
    voxel wide along each axis, the two-label checkerboard, `1 1 2 2` rows, components across every tile face with their complement as
    a second label, a shell around a ball, blobs with islands, labels up to 255, the degenerate volumes, the sides around the tile's"""
    K.check_roots(product, "cpu", case)


def test_label_roots_equal_scipy_per_class_emulated(product):
    pytest.importorskip("scipy.ndimage")
    for case in ("stripes_x", "checker_4x6x66", "crossing_17x70x131", "33x47x21", "ten_class_20x30x70", "tie"):
        K.check_roots(product, "cpu", case, with_scipy=True)


def test_stripes_and_checkerboard_winners_emulated(product):
    K.check_known_winners(product, "cpu")


@pytest.mark.parametrize("case", sorted(LR.CASES))
def test_label_selection_and_info_emulated(product, case):
    K.check_selection(product, "cpu", case)


def test_tie_rule_per_label_emulated(product):
    K.check_tie(product, "cpu")


def test_apply_table_passes_labels_through_emulated(product):
    K.check_apply(product, "cpu")


@pytest.mark.parametrize("case", ["ten_class_20x30x70", "33x47x21", "40x48x36", "shell_around_ball", "crossing_17x70x131", "all_zero"])
def test_keep_largest_per_class_equals_the_per_class_loop_emulated(product, case):
    K.check_against_parent_route(product, "cpu", LR.case(case)[0])


def test_argmax_10_and_32_classes_emulated(product):
    K.check_argmax_many_classes(product, "cpu")


def test_argmax_10_classes_resampled_band_rule_emulated(product):
    K.check_argmax_resampled_10(product, "cpu")


def test_argmax_class_bounds_emulated(product):
    K.check_argmax_refusals(product, "cpu")


def test_wrapper_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_c_refusals_launch_nothing_emulated(emu):
    K.check_c_refusals(emu, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)


def test_save_organs_to_nii_emulated(product, tmp_path):
    K.check_save_organs("cpu", tmp_path)


def test_finish_predictions_per_class_and_organs_emulated(product, tmp_path):
    K.check_tools("cpu", tmp_path)


def test_metrics_with_nine_regions_emulated(product, monkeypatch):
    K.check_metrics_groups("cpu", monkeypatch)
