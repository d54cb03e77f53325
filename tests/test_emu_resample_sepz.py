"""The separate-z resampling branch (segmamba_amd/resample.py `allow_separate_z=True`, `preprocess_case(force_separate_z=...)` on
segm_zoom_slices / segm_zoom_labels_slices of csrc/resample.hip) with the kernel sources compiled for the CPU emulator.  Reference:
tests/resample_sepz_ref.py (numpy float64; held to the reference's own function in tests/test_resample_sepz_ref_cpu.py).  The same
checks run on the HIP library in tests/test_gpu_resample_sepz.py."""
import pytest

from tests import emu_util
from tests import resample_sepz_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.resample / preprocess on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_data_emulated(product):
    """within 2^-23 |want| + 2^-40 max|x| of the float64 restatement and of the reference's recorded outputs: the axis shrinking,
    growing and unchanged, axes 0, 1 and 2, orders 3 and 1, a row past one x tile, 1 x 1 slices, 2048 slices"""
    K.check_data(product, "cpu")


def test_channels_and_views_emulated(product):
    K.check_channels_and_views(product, "cpu")


def test_clip_is_per_slice_emulated(product):
    K.check_per_slice_clip(product, "cpu")


def test_slice_independence_and_determinism_emulated(product):
    K.check_slice_independence(product, "cpu")


def test_labels_dyadic_factors_emulated(product):
    K.check_labels_dyadic(product, "cpu")


def test_labels_past_one_grid_emulated(product):
    K.check_labels_past_one_grid(product, "cpu")


def test_labels_other_factors_emulated(product):
    K.check_labels_near_ties(product, "cpu")


def test_preprocess_case_separate_z_emulated(product):
    K.check_preprocess_case_separate_z(product, "cpu")


def test_case_preprocessor_and_tool_separate_z_emulated(product, tmp_path, monkeypatch):
    K.check_case_preprocessor_separate_z("cpu", tmp_path, monkeypatch)


def test_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)
