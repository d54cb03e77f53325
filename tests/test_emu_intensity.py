"""Intensity augmentation (csrc/intensity.hip, `segmamba_amd.augment.FusedAugmenter`) with the kernel sources compiled for the CPU
emulator: statistics fed directly, the single-rounding ops against ATen's bits, contrast and gamma against the float64 restatement
of tests/intensity_ref.py, the mirror, the chain, the augmenter against `SplineAugmenter`, the feeders, refusals and exports.  The
same checks run on the HIP library in tests/test_gpu_intensity.py."""
import pytest

from tests import emu_util
from tests import intensity_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.augment on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


def test_aten_route_within_its_own_bound():
    """the ratios of the parent's ATen route that k comes from, measured again"""
    K.check_aten_ratios()


def test_statistics_emulated(emu):
    """mean and sd within 1e-12 relative of numpy float64, min and max exact, two calls bit-equal"""
    K.check_stats(emu, "cpu")


def test_statistics_layouts_emulated(emu):
    K.check_stats_layouts(emu, "cpu")


def test_noise_scale_copy_bit_equal_to_aten_emulated(emu):
    K.check_single_rounding_ops(emu, "cpu")


def test_contrast_and_gamma_against_float64_emulated(emu):
    K.check_contrast_gamma(emu, "cpu")


def test_constant_and_clipped_channels_emulated(emu):
    K.check_exact_cases(emu, "cpu")


def test_mirror_emulated(emu):
    K.check_mirror(emu, "cpu")


def test_chain_emulated(product):
    K.check_chain(product, "cpu")


def test_augmenter_single_transforms_emulated(product):
    K.check_augmenter_single_transforms(product, "cpu")


def test_augmenter_everything_on_emulated(product):
    K.check_augmenter_everything(product, "cpu")


def test_augmenter_behaviour_emulated(product):
    K.check_augmenter_behaviour(product, "cpu")


def test_feeders_emulated(product):
    K.check_feeders("cpu")


def test_refusals_emulated(emu):
    K.check_refusals(emu, "cpu")


def test_needs_the_library():
    K.check_needs_the_library()


def test_intensity_exports_emulated(emu):
    K.check_exports(emu)
