"""Device-side resampling (segmamba_amd/resample.py, `preprocess_case(resample=True)`) on the HIP library: the checks of
tests/test_emu_resample.py on the GPU, plus the case at BraTS size (155 x 240 x 240 x 4) resampled from 2 mm to 1 mm along x."""
import pytest

from tests import preprocess_ref as R
from tests import resample_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_cubic_and_linear_zoom(hip):
    K.check_zoom(hip, DEV)


def test_clip(hip):
    K.check_clip(hip, DEV)


def test_shortcuts_and_determinism(hip):
    K.check_shortcuts_and_determinism(hip, DEV)


def test_labels_dyadic_factors(hip):
    K.check_labels_dyadic(hip, DEV)


def test_labels_other_factors(hip):
    K.check_labels_near_ties(hip, DEV)


def test_preprocess_case_resampled(hip):
    K.check_preprocess_case_resampled(hip, DEV)


def test_case_preprocessor_and_tool_resampled(hip, tmp_path, monkeypatch):
    K.check_case_preprocessor_resampled(DEV, tmp_path, monkeypatch)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_new_exports(hip):
    K.check_exports(hip)


def test_preprocess_case_resampled_at_brats_size(hip):
    """the whole of `preprocess_case(resample=True)` at 155 x 240 x 240 x 4, x 2 mm -> 1 mm: data within the bound, seg and class
    locations equal, the properties, and back through `labels_from_logits`"""
    data, seg, _ = R.brats_case()
    assert data.shape == (4, 155, 240, 240)
    want_s, new_shape = K.check_preprocess_resample(hip, DEV, data, seg, (2.0, 1.0, 1.0), (1, 1, 1))
    assert new_shape == [119, 169, 278]
