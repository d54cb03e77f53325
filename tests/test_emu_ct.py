"""Device-side CT case preparation (segmamba_amd/preprocess.py on csrc/fingerprint.hip and csrc/preprocess.hip) with the kernel sources
compiled for the CPU emulator: foreground count and sums, exact order statistics, the gather by foreground rank,
`collect_foreground_intensities`, CT normalisation, `preprocess_case(normalization="ct")`, `CTCasePreprocessor` on files, refusals and
the exports.  References: tests/ct_ref.py (numpy restatements) and the recorded tests/golden/ct_fingerprint.npz.  The same checks run
on the HIP library in tests/test_gpu_ct.py."""
import pytest

from tests import ct_checks as K
from tests import emu_util
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.preprocess on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_fingerprint_volumes_and_foregrounds_emulated(product):
    """(19, 37, 53) and (3, 5, 7); blob, one voxel, two, all, none, last partial segment; seg float32 / uint8 / int16; two channels"""
    K.check_volumes(product, "cpu")


def test_fingerprint_strided_views_emulated(product):
    K.check_strided_views(product, "cpu")


def test_fingerprint_value_patterns_emulated(product):
    """ties, mixed signs, a constant, last-digit-only and top-digit-only differences, both zeros: six channels in one call"""
    K.check_values(product, "cpu")


def test_fingerprint_recorded_reference_emulated(product):
    K.check_golden(product, "cpu")


def test_ct_normalize_emulated(product):
    K.check_ct_normalize(product, "cpu")


def test_preprocess_case_ct_emulated(product):
    """also resampled from spacing (0.8, 0.8, 2.0) to (1, 1, 1)"""
    K.check_preprocess_case_ct_resampled(product, "cpu")


def test_default_route_unchanged_emulated(product):
    K.check_default_route_unchanged(product, "cpu")


def test_ct_case_preprocessor_files_emulated(product, tmp_path):
    K.check_ct_case_preprocessor("cpu", tmp_path)


def test_ct_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_ct_exports_emulated(emu):
    K.check_exports(emu)
