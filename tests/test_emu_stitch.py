"""Stitching a prediction (csrc/stitch.hip, `stitch="hip"` of segmamba_amd/predictor.py) with the kernel sources compiled for the CPU
emulator: bit-equality with the ATen route, the reference's fixture, every entry on its own, refusals and exports.  The same checks
run on the HIP library in tests/test_gpu_stitch.py."""
import pytest

from tests import emu_util
from tests import stitch_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.predictor on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("name", sorted(K.EQUAL_CASES))
def test_bit_equal_to_the_aten_route_emulated(product, name):
    K.check_equal_to_aten(name, "cpu")


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_reference_fixture_emulated(product, name):
    K.check_golden(name, "cpu")


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_gather_emulated(emu, name):
    K.check_gather(emu, name, "cpu")


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_count_emulated(emu, name):
    K.check_count(emu, name, "cpu")


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_blend_emulated(emu, name):
    K.check_blend(emu, name, "cpu")


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_finish_emulated(emu, name):
    K.check_finish(emu, name, "cpu")


def test_c_entries_refuse_emulated(emu):
    K.check_c_refusals(emu, "cpu")


def test_wrappers_refuse_emulated(emu):
    K.check_wrapper_refusals(emu, "cpu")


def test_route_refusals_emulated(product):
    K.check_route_refusals("cpu")


def test_needs_the_device():
    K.check_needs_the_device()


def test_stitch_exports_emulated(emu):
    K.check_exports(emu)
