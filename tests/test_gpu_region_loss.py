"""The region-based loss (csrc/region_loss.hip) on the HIP library: the checks of tests/test_emu_region_loss.py on the GPU, plus one
case of (2, 3, 40, 40, 41) - 33 workgroups per sample - against the ATen formulation in float64 on the device."""
import pytest
import torch

from tests import region_loss_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_sums_sizes_regions_dtypes(hip):
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


def test_label_mode_equals_plane_mode(hip):
    K.check_label_mode_equals_plane_mode(DEV)


def test_never_occurring_region_and_all_ignored(hip):
    K.check_classes_edge_cases(DEV)


def test_strided_logits_through_the_class(hip):
    K.check_strided_logits_through_the_class(DEV)


def test_refusals(hip, monkeypatch):
    K.check_refusals(hip, DEV, monkeypatch)


def test_region_loss_exports(hip):
    K.check_exports(hip)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_multi_workgroup_against_aten_fp64(hip, dtype):
    K.check_multi_workgroup(DEV, dtype)
