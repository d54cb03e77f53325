"""Softmax Dice + cross entropy (csrc/dice_ce.hip) with the kernel sources compiled for the CPU emulator: the sums fed directly over
sizes, class counts, label and logits dtypes, masks, layouts, repeatability, the backward with each coefficient, wrong labels,
refusals, exports, and the classes of segmamba_amd.losses with device_sums=True on the emulated library.  References:
tests/loss_ref.py (float64) and the recorded tests/golden/dice_ce.npz and topk_ce.npz.  The same checks run on the HIP library in
tests/test_gpu_dice_ce.py."""
import pytest

from tests import emu_util
from tests import dice_ce_checks as K
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


def test_sums_sizes_classes_dtypes_emulated(emu):
    """V in {1, 7, 63, 64, 65, 240, 255, 257, 4097, 133128, 133184} x C in {1, 2, 4, 8, 9, 16} x four label dtypes x ignore x mask"""
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


def test_dc_and_topk_recorded_reference_emulated(product):
    K.check_topk_recorded("cpu")


def test_dice_classes_and_loss_masks_emulated(product):
    K.check_dice_classes_and_masks("cpu")


def test_all_ignored_deep_supervision_and_16_bit_logits_emulated(product):
    K.check_classes_edge_cases("cpu")


def test_strided_logits_through_the_class_emulated(product):
    K.check_strided_logits_through_the_class("cpu")


def test_refusals_emulated(product, monkeypatch):
    K.check_refusals(product, "cpu", monkeypatch)


def test_softmax_dice_exports_emulated(emu):
    K.check_exports(emu)
