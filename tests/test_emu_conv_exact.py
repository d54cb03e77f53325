"""Exact-arithmetic parity of the 3x3x3 convolution kernels with the kernel sources compiled for the CPU emulator: integer operands,
fp64 CPU reference, torch.equal (tests/conv_exact_checks.py).  The same checks run on the HIP library in tests/test_gpu_conv_exact.py."""
import pytest
import torch

from tests import emu_util
from tests import conv_exact_checks as C

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_CASES)
def test_cube_forward_dgrad_accumulate_emulated(emu, shape, nt, splits):
    C.check_cube(emu, "cpu", shape, nt, splits)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_SWEEP)
def test_cube_every_plan_of_one_layer_emulated(emu, shape, nt, splits):
    C.check_cube(emu, "cpu", shape, nt, splits)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_FP16)
def test_cube_fp16_emulated(emu, shape, nt, splits):
    C.check_cube(emu, "cpu", shape, nt, splits, torch.float16)


def test_cube_seven_rounds_in_five_splits_emulated(emu):
    """a forced split count that does not divide the rounds, with more splits than any divisor but R itself"""
    C.check_cube(emu, "cpu", (1, 224, 64, 8, 8, 8), 2, 5)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_ROUNDED)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cube_rounded_once_emulated(emu, shape, nt, splits, dtype):
    C.check_cube_rounded_once(emu, "cpu", shape, nt, splits, dtype)


def test_cube_and_channel_last_refuse_bad_out_and_image_emulated(emu):
    C.check_cube_refusals(emu, "cpu")


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
@pytest.mark.parametrize("shape", C.ROW_CASES_ALL)
def test_row_forward_dgrad_accumulate_emulated(emu, shape, variant):
    C.check_row(emu, "cpu", shape, variant)


@pytest.mark.parametrize("shape", C.ROW_CASES_DEFAULT)
def test_row_cout_16_and_32_emulated(emu, shape):
    C.check_row(emu, "cpu", shape, "default")


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
def test_row_fp16_emulated(emu, variant):
    C.check_row(emu, "cpu", (1, 48, 2, 2, 16), variant, torch.float16)


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
def test_row_narrow_first_layer_and_channel_slice_emulated(emu, variant):
    C.check_row(emu, "cpu", (1, 48, 2, 5, 16), variant, cin=4)
    C.check_row(emu, "cpu", (2, 48, 2, 3, 40), variant, sliced=True)


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_row_rounded_once_emulated(emu, variant, dtype):
    C.check_row_rounded_once(emu, "cpu", variant, dtype)


@pytest.mark.parametrize("shape", C.WGRAD_ROW_CASES)
def test_wgrad_emulated(emu, shape):
    C.check_wgrad_row(emu, "cpu", shape)


def test_wgrad_channel_slices_and_fp16_emulated(emu):
    C.check_wgrad_row_slices(emu, "cpu")
    C.check_wgrad_row(emu, "cpu", (1, 48, 48, 2, 3, 40), torch.float16)


@pytest.mark.parametrize("shape", C.WGRAD_CUBE_CASES)
def test_cube_wgrad_emulated(emu, shape):
    C.check_wgrad_cube(emu, "cpu", shape)


def test_cube_wgrad_fp16_emulated(emu):
    C.check_wgrad_cube(emu, "cpu", (2, 32, 64, 8, 8, 16), torch.float16)


@pytest.mark.parametrize("config,fwd_route,wgrad_route", [("row", v, "mfma") for v in C.ROW_VARIANTS] + [("cube", "cube", "cube"), ("cube", "cube", "mfma")])
def test_dispatcher_on_one_forced_route_emulated(emu, monkeypatch, config, fwd_route, wgrad_route):
    C.check_dispatch(emu, "cpu", monkeypatch, config, fwd_route, wgrad_route)


def test_add_part_after_a_vendor_route_result_that_is_not_dense_emulated(emu, monkeypatch):
    C.check_add_part_after_vendor_route(emu, "cpu", monkeypatch)
