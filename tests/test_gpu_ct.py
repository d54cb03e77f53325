"""Device-side CT case preparation (segmamba_amd/preprocess.py) on the HIP library: the checks of tests/test_emu_ct.py on the GPU, plus
one case of 1 x 96 x 160 x 160 with about a third foreground - many workgroups flushing histograms, offsets over 600 segments -
against np.sort on the host."""
import pytest

from tests import ct_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_fingerprint_volumes_and_foregrounds(hip):
    K.check_volumes(hip, DEV)


def test_fingerprint_strided_views(hip):
    K.check_strided_views(hip, DEV)


def test_fingerprint_value_patterns(hip):
    K.check_values(hip, DEV)


def test_fingerprint_recorded_reference(hip):
    K.check_golden(hip, DEV)


def test_fingerprint_at_size(hip):
    K.check_large(hip, DEV)


def test_ct_normalize(hip):
    K.check_ct_normalize(hip, DEV)


def test_preprocess_case_ct(hip):
    K.check_preprocess_case_ct_resampled(hip, DEV)


def test_default_route_unchanged(hip):
    K.check_default_route_unchanged(hip, DEV)


def test_ct_case_preprocessor_files(hip, tmp_path):
    K.check_ct_case_preprocessor(DEV, tmp_path)


def test_ct_refusals(hip):
    K.check_refusals(hip, DEV)


def test_ct_exports(hip):
    K.check_exports(hip)
