"""The fused add + LayerNorm / RMSNorm (csrc/add_norm.hip) with the kernel sources compiled for the CPU emulator: values over sizes,
dtypes, residual kinds and norms, exact values, repeatability, row independence, the packet against the element route, layouts,
refusals, exports, and layer_norm_fn / rms_norm_fn / RMSNorm / Block of segmamba_amd on the emulated library.  References:
tests/add_norm_ref.py (float64) and the recorded tests/golden/add_norm.npz.  The same checks run on the HIP library in
tests/test_gpu_add_norm.py."""
import pytest

from tests import emu_util
from tests import add_norm_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.add_norm on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_values_sizes_dtypes_residuals_emulated(emu):
    K.check_values(emu, "cpu")


def test_exact_values_emulated(emu):
    K.check_exact(emu, "cpu")


def test_two_calls_bit_equal_emulated(emu):
    K.check_repeat(emu, "cpu")


def test_row_does_not_depend_on_the_others_emulated(emu):
    K.check_row_independence(emu, "cpu")


def test_packet_and_element_routes_agree_emulated(emu):
    K.check_routes(emu, "cpu")


def test_row_strides_emulated(emu):
    K.check_layouts(emu, "cpu")


def test_refusals_emulated(emu):
    K.check_refusals(emu, "cpu")


def test_add_norm_exports_emulated(emu):
    K.check_exports(emu)


def test_functions_recorded_reference_emulated(product):
    K.check_functions_recorded("cpu")


def test_block_recorded_reference_emulated(product):
    K.check_block_recorded("cpu")


def test_api_rules_emulated(product):
    K.check_api_rules("cpu")
