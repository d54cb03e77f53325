"""Device-side resampling (segmamba_amd/resample.py and `preprocess_case(resample=True)` on csrc/resample.hip) with the kernel sources
compiled for the CPU emulator: cubic and linear zoom, the clip, shortcuts and determinism, the label rule at dyadic and at other
factors, `preprocess_case` / `CasePreprocessor` / tools/preprocess_cases.py with resampling, refusals and the exports.  Reference:
tests/resample_ref.py (numpy float64; pinned to scipy in tests/test_resample_ref_cpu.py).  The same checks run on the HIP library in
tests/test_gpu_resample.py."""
import pytest

from tests import emu_util
from tests import resample_checks as K
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


def test_cubic_and_linear_zoom_emulated(product):
    """within 2^-23 |want| + 2^-40 max|x| of the float64 restatement: odd, even and unit sides, a side above 256, factors 2, 0.5,
    1.5, 0.8 / 1.25, 1 to 8 channels, strided channel views"""
    K.check_zoom(product, "cpu")


def test_clip_emulated(product):
    K.check_clip(product, "cpu")


def test_shortcuts_and_determinism_emulated(product):
    K.check_shortcuts_and_determinism(product, "cpu")


def test_labels_dyadic_factors_emulated(product):
    """equal at every voxel, equal counts; -1, a label above 255 and a cell where no label reaches one half"""
    K.check_labels_dyadic(product, "cpu")


def test_labels_other_factors_emulated(product):
    K.check_labels_near_ties(product, "cpu")


def test_preprocess_case_resampled_emulated(product):
    K.check_preprocess_case_resampled(product, "cpu")


def test_case_preprocessor_and_tool_resampled_emulated(product, tmp_path, monkeypatch):
    K.check_case_preprocessor_resampled("cpu", tmp_path, monkeypatch)


def test_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)
