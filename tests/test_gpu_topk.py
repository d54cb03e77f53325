"""The top-k cross entropy (csrc/topk_ce.hip) on the HIP library: the checks of tests/test_emu_topk.py on the GPU, plus one case of
(2, 4, 40, 40, 41) - 33 workgroups per pass over the values, 513 of the per-voxel kernels - against ATen in float64 on the device."""
import pytest
import torch

from tests import topk_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_map_recorded_cases(hip):
    K.check_map(hip, DEV)


def test_map_wrong_and_ignored_labels(hip):
    K.check_map_wrong_labels(hip, DEV)


@pytest.mark.parametrize("name", K.PATTERNS)
def test_select_sizes_and_value_patterns(hip, name):
    """n in {1, 63, 64, 65, 255, 257, 4097, 70001} x kk in {1, 2, n // 10, n - 1, n} for each of the eight value patterns"""
    K.check_select(hip, DEV, name)


def test_select_twice_and_unaligned(hip):
    K.check_select_twice(hip, DEV)


def test_backward_factors(hip):
    K.check_backward(hip, DEV)


def test_backward_ties_and_wrong_labels(hip):
    K.check_backward_ties_and_wrong_labels(hip, DEV)


def test_topk_refusals(hip):
    K.check_refusals(hip, DEV)


def test_topk_exports(hip):
    K.check_exports(hip)


def test_classes_recorded_reference(hip):
    """TopKLoss and DC_and_topk_loss(weight_dice=0) against the recording"""
    K.check_classes_recorded(DEV)


def test_cross_entropy_reductions(hip):
    K.check_reductions(DEV)


def test_cross_entropy_mean_route_unchanged(hip):
    K.check_mean_route_bits(hip, DEV)


def test_dice_term_refuses_device_tensors(hip):
    K.check_dice_refuses_device(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_multi_workgroup_against_aten_fp64(hip, dtype):
    K.check_multi_workgroup(DEV, dtype)
