"""Signed-distance and edge targets (csrc/sdm.hip, segmamba_amd/sdm.py) on the HIP library: the checks of tests/test_emu_sdm.py on
the GPU.  The host functions and the loader run under torch.cuda.set_sync_debug_mode("error"): a copy to the host or a wait raises."""
import pytest

from tests import sdm_checks as C
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("name", C.NAMED)
def test_masks_and_targets(hip, name):
    C.check_named(hip, DEV, name)


@pytest.mark.parametrize("shape", C.SHAPES_X)
def test_widths_around_a_wave(hip, shape):
    C.check_shape(hip, DEV, shape)


def test_label_dtypes(hip):
    C.check_dtypes(hip, DEV)


def test_offset_pointers_and_output_choice(hip):
    C.check_offset_pointers(hip, DEV)


@pytest.mark.parametrize("n", [1, 2, 5])
def test_host_groups_without_a_sync(hip, n):
    C.check_host_groups(DEV, n)


def test_ten_regions(hip):
    C.check_many_regions(DEV)


def test_reference_names(hip):
    C.check_reference_names(DEV)


def test_loader_targets_follow_the_augmented_label(hip):
    C.check_loader(DEV, "fused")


def test_tool_and_dataset(hip, tmp_path):
    C.check_tool_and_dataset(DEV, tmp_path)


def test_refusals(hip):
    C.check_refusals(hip, DEV)


def test_exports_in_the_hip_library(hip):
    C.check_exports(hip)
