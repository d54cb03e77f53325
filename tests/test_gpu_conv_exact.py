"""Exact-arithmetic parity of the 3x3x3 convolution kernels on the HIP library: the checks of tests/test_emu_conv_exact.py on the GPU,
where LDS races, barrier placement and the real MFMA lane mappings live; integer operands, fp64 CPU reference, torch.equal
(tests/conv_exact_checks.py)."""
import pytest
import torch

from tests import conv_exact_checks as C
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_CASES + C.CUBE_CASES_GPU)
def test_cube_forward_dgrad_accumulate(hip, shape, nt, splits):
    C.check_cube(hip, DEV, shape, nt, splits)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_SWEEP)
def test_cube_every_plan_of_one_layer(hip, shape, nt, splits):
    C.check_cube(hip, DEV, shape, nt, splits)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_FP16)
def test_cube_fp16(hip, shape, nt, splits):
    C.check_cube(hip, DEV, shape, nt, splits, torch.float16)


def test_cube_seven_rounds_in_five_splits(hip):
    C.check_cube(hip, DEV, (1, 224, 64, 8, 8, 8), 2, 5)


@pytest.mark.parametrize("shape,nt,splits", C.CUBE_ROUNDED)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_cube_rounded_once(hip, shape, nt, splits, dtype):
    C.check_cube_rounded_once(hip, DEV, shape, nt, splits, dtype)


def test_cube_and_channel_last_refuse_bad_out_and_image(hip):
    C.check_cube_refusals(hip, DEV)


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
@pytest.mark.parametrize("shape", C.ROW_CASES_ALL + [C.ROW_CASE_GPU])
def test_row_forward_dgrad_accumulate(hip, shape, variant):
    C.check_row(hip, DEV, shape, variant)


@pytest.mark.parametrize("shape", C.ROW_CASES_DEFAULT)
def test_row_cout_16_and_32(hip, shape):
    C.check_row(hip, DEV, shape, "default")


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
def test_row_fp16(hip, variant):
    C.check_row(hip, DEV, (1, 48, 2, 2, 16), variant, torch.float16)


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
def test_row_narrow_first_layer_and_channel_slice(hip, variant):
    C.check_row(hip, DEV, (1, 48, 2, 5, 16), variant, cin=4)
    C.check_row(hip, DEV, (2, 48, 2, 3, 40), variant, sliced=True)


@pytest.mark.parametrize("variant", list(C.ROW_VARIANTS))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_row_rounded_once(hip, variant, dtype):
    C.check_row_rounded_once(hip, DEV, variant, dtype)


@pytest.mark.parametrize("shape", C.WGRAD_ROW_CASES)
def test_wgrad(hip, shape):
    C.check_wgrad_row(hip, DEV, shape)


def test_wgrad_channel_slices_and_fp16(hip):
    C.check_wgrad_row_slices(hip, DEV)
    C.check_wgrad_row(hip, DEV, (1, 48, 48, 2, 3, 40), torch.float16)


@pytest.mark.parametrize("shape", C.WGRAD_CUBE_CASES)
def test_cube_wgrad(hip, shape):
    C.check_wgrad_cube(hip, DEV, shape)


def test_cube_wgrad_fp16(hip):
    C.check_wgrad_cube(hip, DEV, (2, 32, 64, 8, 8, 16), torch.float16)


@pytest.mark.parametrize("config,fwd_route,wgrad_route", [("row", v, "mfma") for v in C.ROW_VARIANTS] + [("cube", "cube", "cube"), ("cube", "cube", "mfma")])
def test_dispatcher_on_one_forced_route(hip, monkeypatch, config, fwd_route, wgrad_route):
    C.check_dispatch(hip, DEV, monkeypatch, config, fwd_route, wgrad_route)


def test_add_part_after_a_vendor_route_result_that_is_not_dense(hip, monkeypatch):
    C.check_add_part_after_vendor_route(hip, DEV, monkeypatch)
