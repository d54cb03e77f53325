"""Connected components at connectivity 1, 2 and 3 (csrc/ccl_roots.hip) and the `connectivity` keyword of the host functions, with the
kernel sources compiled for the CPU emulator.  References: tests/ccl_conn_ref.py (numpy; pinned to scipy.ndimage.label here).  The same
checks run on the HIP library in tests/test_gpu_ccl_conn.py."""
import pytest

from tests import ccl_conn_checks as K
from tests import ccl_conn_ref as CR
from tests import emu_util
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")

SCIPY_CASES = ["hand", "checker_5x6x66", "body_centred_5x6x66", "side_points_64", "sides_3x5x65", "1x1x130", "random_5x5x65_03",
               "random_4x3x64_06", "random_9x10x131_03", "random_40x48x136_01"] + [CR.stair_name(s) for s in CR.STAIR_STEPS]
HOST_CASES = ["hand", "checker_5x6x66", "body_centred_5x6x66", "all_zero", "all_one", "1x1x1", "random_5x5x65_03", "random_3x4x63_06",
              "random_9x10x131_01", "random_9x10x131_06"]
PER_CLASS_CASES = ["hand_two_labels", "ten_class_9x13x70", "diagonal_island", "labels_5x5x65_03", "labels_9x10x131_06", "labels_all_zero"]


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.postprocess on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_numpy_reference_equals_scipy_label_at_every_connectivity():
    """the reference of every other test here against scipy.ndimage.label(structure=generate_binary_structure(3, c)), and the
    component counts the cases state (hand case 5 / 4 / 3, checkerboard 990 / 1 / 1, staircases 9 or 1, hollow cube 124 / 124 / 97)"""
    pytest.importorskip("scipy.ndimage")
    K.check_reference_against_scipy(SCIPY_CASES)


@pytest.mark.parametrize("case", sorted(CR.MASKS))
def test_mask_roots_emulated(product, case):
    """roots = the reference at c = 1, 2, 3 with bit = -1, a bit in 1 .. 7 among noise, bit 7 and inverted; c = 1 = segm_ccl_roots; two
    calls bit-equal.  Cases: the hand case, the lattices, the ten staircases, random masks of three densities on the 27 volumes around
    the tile's sides and on 9 x 10 x 131 / 40 x 48 x 136, the degenerate volumes, the sides of the volume"""
    K.check_mask(product, "cpu", case)


@pytest.mark.parametrize("case", sorted(CR.LABELS))
def test_label_roots_emulated(product, case):
    """per class what the binary entry gives at the same c, -1 on the background, different labels never joined, two calls bit-equal"""
    K.check_labels(product, "cpu", case)


def test_legacy_entries_ignore_reserved_emulated(emu):
    K.check_legacy_entries_ignore_reserved(emu, "cpu")


@pytest.mark.parametrize("case", HOST_CASES)
def test_host_functions_on_masks_emulated(product, case):
    K.check_host_mask_functions(product, "cpu", case)


def test_label_equals_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    K.check_label_equals_scipy("cpu", ["hand", "checker_5x6x66", "random_5x5x65_03", "random_9x10x131_06"])


def test_tie_rule_at_connectivity_2_emulated(product):
    K.check_tie_rule("cpu")


def test_fill_holes_takes_the_background_connectivity_emulated(product):
    K.check_fill_holes("cpu")


@pytest.mark.parametrize("case", PER_CLASS_CASES)
def test_keep_largest_per_class_equals_the_per_class_loop_emulated(product, case):
    K.check_keep_largest_per_class(product, "cpu", case)


def test_diagonal_island_stays_at_connectivity_3_emulated(product):
    K.check_diagonal_island("cpu")


def test_connectivity_outside_1_2_3_is_a_value_error_emulated(product):
    K.check_value_errors(product, "cpu")


def test_c_refusals_launch_nothing_emulated(emu):
    K.check_c_refusals(emu, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)


def test_predictor_passes_connectivity_emulated(product, tmp_path):
    K.check_predictor("cpu", tmp_path)


def test_finish_predictions_connectivity_emulated(product, tmp_path):
    K.check_tool("cpu", tmp_path)
