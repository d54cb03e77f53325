"""Stitching a prediction on the HIP library (csrc/stitch.hip, `stitch="hip"` of segmamba_amd/predictor.py): the checks of
tests/stitch_checks.py with both routes on the device, and one mirrored prediction with every synchronising call an error."""
import pytest

from tests import stitch_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("name", sorted(K.EQUAL_CASES))
def test_bit_equal_to_the_aten_route(hip, name):
    K.check_equal_to_aten(name, DEV)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_reference_fixture(hip, name):
    K.check_golden(name, DEV)


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_gather(hip, name):
    K.check_gather(hip, name, DEV)


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_count(hip, name):
    K.check_count(hip, name, DEV)


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_blend(hip, name):
    K.check_blend(hip, name, DEV)


@pytest.mark.parametrize("name", K.ENTRY_CASES)
def test_finish(hip, name):
    K.check_finish(hip, name, DEV)


def test_no_host_round_trip(hip):
    K.check_no_sync(DEV)


def test_c_entries_refuse(hip):
    K.check_c_refusals(hip, DEV)


def test_wrappers_refuse(hip):
    K.check_wrapper_refusals(hip, DEV)


def test_route_refusals(hip):
    K.check_route_refusals(DEV)


def test_stitch_exports(hip):
    K.check_exports(hip)
