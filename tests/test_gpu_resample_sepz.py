"""The separate-z resampling branch (segmamba_amd/resample.py `allow_separate_z=True`, `preprocess_case(force_separate_z=...)`) on
the HIP library: the checks of tests/test_emu_resample_sepz.py on the GPU."""
import pytest

from tests import resample_sepz_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_data(hip):
    K.check_data(hip, DEV)


def test_channels_and_views(hip):
    K.check_channels_and_views(hip, DEV)


def test_clip_is_per_slice(hip):
    K.check_per_slice_clip(hip, DEV)


def test_slice_independence_and_determinism(hip):
    K.check_slice_independence(hip, DEV)


def test_labels_dyadic_factors(hip):
    K.check_labels_dyadic(hip, DEV)


def test_labels_past_one_grid(hip):
    K.check_labels_past_one_grid(hip, DEV)


def test_labels_other_factors(hip):
    K.check_labels_near_ties(hip, DEV)


def test_preprocess_case_separate_z(hip):
    K.check_preprocess_case_separate_z(hip, DEV)


def test_case_preprocessor_and_tool_separate_z(hip, tmp_path, monkeypatch):
    K.check_case_preprocessor_separate_z(DEV, tmp_path, monkeypatch)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_new_exports(hip):
    K.check_exports(hip)
