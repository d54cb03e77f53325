"""Augmentation at the reference's interpolation orders (segmamba_amd/augment.py `SplineAugmenter` on csrc/augment.hip) with the
kernel sources compiled for the CPU emulator: spline coefficients, the cubic warp, the label rule, order-0 zoom, gaussian blur, the
augmenter replayed from its host draws, the feeders, refusals and the exports.  Reference: tests/augment_ref.py (numpy float64; pinned
to scipy in tests/test_augment_ref_cpu.py).  The same checks run on the HIP library in tests/test_gpu_augment.py."""
import pytest

from tests import augment_checks as K
from tests import emu_util
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


def test_spline_coefficients_emulated(product):
    K.check_coefs(product, "cpu")


def test_cubic_warp_emulated(product):
    """within 2^-23 |want| + 2^-40 max|x| of the float64 restatement at every voxel, none left out, at least 20 % inside"""
    K.check_warp(product, "cpu")


def test_cubic_warp_flags_and_views_emulated(product):
    K.check_warp_flags_and_views(product, "cpu")


def test_labels_emulated(product):
    """equal at every voxel for the three matrices and for the half-voxel shift, int16 and int64"""
    K.check_labels(product, "cpu")


def test_nearest_zoom_emulated(product):
    K.check_zoom_nearest(product, "cpu")


def test_gaussian_blur_emulated(product):
    """within 3 * 2^-23 max|x| of scipy's gaussian_filter on both sides of the radius steps, sides shorter than the radius"""
    K.check_blur(product, "cpu")


def test_augmenter_transforms_replayed_emulated(product):
    K.check_augmenter_transforms(product, "cpu")


def test_augmenter_behaviour_emulated(product):
    K.check_augmenter_behaviour(product, "cpu")


def test_feeders_emulated(product):
    K.check_feeders("cpu")


def test_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_needs_the_library():
    K.check_needs_the_library()


def test_new_exports_emulated(emu):
    K.check_exports(emu)
