"""Intensity augmentation (csrc/intensity.hip, `segmamba_amd.augment.FusedAugmenter`) on the HIP library: the checks of
tests/test_emu_intensity.py on the GPU.  The chain and one whole `FusedAugmenter` call with every coin on run under
`torch.cuda.set_sync_debug_mode("error")`: a device-to-host copy or a wait raises."""
import pytest

from tests import intensity_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_statistics(hip):
    K.check_stats(hip, DEV)


def test_statistics_layouts(hip):
    K.check_stats_layouts(hip, DEV)


def test_noise_scale_copy_bit_equal_to_aten(hip):
    K.check_single_rounding_ops(hip, DEV)


def test_contrast_and_gamma_against_float64(hip):
    K.check_contrast_gamma(hip, DEV)


def test_constant_and_clipped_channels(hip):
    K.check_exact_cases(hip, DEV)


def test_mirror(hip):
    K.check_mirror(hip, DEV)


def test_chain_without_the_host(hip):
    K.check_chain(hip, DEV)


def test_augmenter_single_transforms(hip):
    K.check_augmenter_single_transforms(hip, DEV)


def test_augmenter_everything_on(hip):
    K.check_augmenter_everything(hip, DEV)


def test_augmenter_behaviour(hip):
    K.check_augmenter_behaviour(hip, DEV)


def test_feeders(hip):
    K.check_feeders(DEV)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_intensity_exports(hip):
    K.check_exports(hip)
