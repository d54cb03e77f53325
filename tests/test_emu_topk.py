"""The top-k cross entropy (csrc/topk_ce.hip) with the kernel sources compiled for the CPU emulator: the per-voxel map, the radix
selection fed directly, the backward with each of its factors, ties, wrong labels, refusals, exports, and the classes of
segmamba_amd.losses / train_ops on the emulated library.  References: tests/topk_ref.py (float64) and the recorded
tests/golden/topk_ce.npz.  The same checks run on the HIP library in tests/test_gpu_topk.py."""
import pytest

from tests import emu_util
from tests import topk_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.train_ops / losses on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_map_recorded_cases_emulated(emu):
    """the fixture's cases in fp32 / fp16 / bf16 against the restatement on the same rounded logits; two calls bit-equal"""
    K.check_map(emu, "cpu")


def test_map_wrong_and_ignored_labels_emulated(emu):
    K.check_map_wrong_labels(emu, "cpu")


@pytest.mark.parametrize("name", K.PATTERNS)
def test_select_sizes_and_value_patterns_emulated(emu, name):
    """n in {1, 63, 64, 65, 255, 257, 4097, 70001} x kk in {1, 2, n // 10, n - 1, n} for each of the eight value patterns"""
    K.check_select(emu, "cpu", name)


def test_select_twice_and_unaligned_emulated(emu):
    K.check_select_twice(emu, "cpu")


def test_backward_factors_emulated(emu):
    """coef, scale and the top-k weight alone and combined, three dtypes; two calls bit-equal"""
    K.check_backward(emu, "cpu")


def test_backward_ties_and_wrong_labels_emulated(emu):
    K.check_backward_ties_and_wrong_labels(emu, "cpu")


def test_topk_refusals_emulated(emu):
    K.check_refusals(emu, "cpu")


def test_topk_exports_emulated(emu):
    K.check_exports(emu)


def test_classes_recorded_reference_emulated(product):
    K.check_classes_recorded("cpu")


def test_cross_entropy_reductions_emulated(product):
    K.check_reductions("cpu")


def test_cross_entropy_mean_route_unchanged_emulated(product):
    K.check_mean_route_bits(product, "cpu")


def test_dice_term_refuses_the_library_emulated(product):
    K.check_dice_refuses_device("cpu")
