"""The fused add + LayerNorm / RMSNorm (csrc/add_norm.hip) on the HIP library: the checks of tests/test_emu_add_norm.py on the GPU,
plus one case of 524288 x 48 in bf16 with an fp32 residual stream against the float64 restatement evaluated on the device."""
import pytest

from tests import add_norm_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_values_sizes_dtypes_residuals(hip):
    K.check_values(hip, DEV)


def test_exact_values(hip):
    K.check_exact(hip, DEV)


def test_two_calls_bit_equal(hip):
    K.check_repeat(hip, DEV)


def test_row_does_not_depend_on_the_others(hip):
    K.check_row_independence(hip, DEV)


def test_packet_and_element_routes_agree(hip):
    K.check_routes(hip, DEV)


def test_row_strides(hip):
    K.check_layouts(hip, DEV)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_add_norm_exports(hip):
    K.check_exports(hip)


def test_functions_recorded_reference(hip):
    K.check_functions_recorded(DEV)


def test_block_recorded_reference(hip):
    K.check_block_recorded(DEV)


def test_api_rules(hip):
    K.check_api_rules(DEV)


def test_stage0_tokens_bf16_fp32_stream(hip):
    K.check_large(hip, DEV)
