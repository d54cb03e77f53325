"""Signed-distance and edge targets (csrc/sdm.hip, segmamba_amd/sdm.py) with the kernel sources compiled for the CPU emulator, held
to tests/sdm_ref.py, the numpy float64 restatement of the reference's dataset_sdm_edge.py.  The same checks run on the HIP library in
tests/test_gpu_sdm.py."""
import pytest

from tests import emu_util
from tests import sdm_checks as C
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.sdm on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("name", C.NAMED)
def test_masks_and_targets_emulated(emu, name):
    """bits and counts exactly; sdf and sdm within one fp32 ulp; 0 on the boundary, +-1 at the extremes, dead planes 0; bit-equal"""
    C.check_named(emu, "cpu", name)


@pytest.mark.parametrize("shape", C.SHAPES_X)
def test_widths_around_a_wave_emulated(emu, shape):
    C.check_shape(emu, "cpu", shape)


def test_label_dtypes_emulated(emu):
    C.check_dtypes(emu, "cpu")


def test_offset_pointers_and_output_choice_emulated(emu):
    C.check_offset_pointers(emu, "cpu")


@pytest.mark.parametrize("n", [1, 2, 5])
def test_host_groups_emulated(product, n):
    C.check_host_groups("cpu", n)


def test_ten_regions_emulated(product):
    C.check_many_regions("cpu")


def test_reference_names_emulated(product):
    C.check_reference_names("cpu")


def test_loader_targets_follow_the_augmented_label_emulated(product):
    C.check_loader("cpu", "fused")


def test_tool_and_dataset_emulated(product, tmp_path):
    C.check_tool_and_dataset("cpu", tmp_path)


def test_refusals_emulated(emu):
    C.check_refusals(emu, "cpu")


def test_exports_emulated(emu):
    C.check_exports(emu)
