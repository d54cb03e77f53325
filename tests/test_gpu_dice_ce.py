"""Softmax Dice + cross entropy (csrc/dice_ce.hip) on the HIP library: the checks of tests/test_emu_dice_ce.py on the GPU, plus one
case of (2, 4, 40, 40, 41) - 33 stretches per sample - against the ATen formulation in float64 on the device."""
import pytest
import torch

from tests import dice_ce_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_sums_sizes_classes_dtypes(hip):
    K.check_sums(hip, DEV)


def test_layouts(hip):
    K.check_layouts(hip, DEV)


def test_two_calls_bit_equal(hip):
    K.check_repeat(hip, DEV)


def test_backward_coefficients(hip):
    K.check_backward(hip, DEV)


def test_wrong_and_ignored_labels(hip):
    K.check_wrong_labels(hip, DEV)


def test_classes_recorded_reference(hip):
    K.check_classes_recorded(DEV)


def test_dc_and_topk_recorded_reference(hip):
    K.check_topk_recorded(DEV)


def test_dice_classes_and_loss_masks(hip):
    K.check_dice_classes_and_masks(DEV)


def test_all_ignored_deep_supervision_and_16_bit_logits(hip):
    K.check_classes_edge_cases(DEV)


def test_strided_logits_through_the_class(hip):
    K.check_strided_logits_through_the_class(DEV)


def test_refusals(hip, monkeypatch):
    K.check_refusals(hip, DEV, monkeypatch)


def test_softmax_dice_exports(hip):
    K.check_exports(hip)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_multi_workgroup_against_aten_fp64(hip, dtype):
    K.check_multi_workgroup(DEV, dtype)
