"""The region-based loss (csrc/region_loss.hip) with the kernel sources compiled for the CPU emulator: the sums fed directly over
sizes, region counts, target and logits dtypes, layouts, repeatability, the backward with each coefficient, wrong labels, refusals,
exports, and DC_and_BCE_loss of segmamba_amd.losses on the emulated library.  References: tests/region_loss_ref.py (float64) and the
recorded tests/golden/region_bce.npz.  The same checks run on the HIP library in tests/test_gpu_region_loss.py."""
import pytest

from tests import emu_util
from tests import region_loss_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.losses on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_sums_sizes_regions_dtypes_emulated(emu):
    """V in {1, 7, 63, 64, 65, 240, 255, 257, 4097, 133128, 133184} x R in {1, 3, 8} x four label and three plane dtypes x ignore"""
    K.check_sums(emu, "cpu")


def test_layouts_emulated(emu):
    K.check_layouts(emu, "cpu")


def test_two_calls_bit_equal_emulated(emu):
    K.check_repeat(emu, "cpu")


def test_backward_coefficients_emulated(emu):
    K.check_backward(emu, "cpu")


def test_wrong_and_ignored_labels_emulated(emu):
    K.check_wrong_labels(emu, "cpu")


def test_classes_recorded_reference_emulated(product):
    K.check_classes_recorded("cpu")


def test_label_mode_equals_plane_mode_emulated(product):
    K.check_label_mode_equals_plane_mode("cpu")


def test_never_occurring_region_and_all_ignored_emulated(product):
    K.check_classes_edge_cases("cpu")


def test_strided_logits_through_the_class_emulated(product):
    K.check_strided_logits_through_the_class("cpu")


def test_refusals_emulated(product, monkeypatch):
    K.check_refusals(product, "cpu", monkeypatch)


def test_region_loss_exports_emulated(emu):
    K.check_exports(emu)
