"""Device-side case preparation (segmamba_amd/preprocess.py on csrc/preprocess.hip) with the kernel sources compiled for the CPU
emulator: non-zero mask and box, hole filling, crop with the -1 rule, z-score, class locations, `preprocess_case` end to end and back
through `labels_from_logits`, `CasePreprocessor` on files, wrapper refusals and the exports.  References: tests/preprocess_ref.py
(numpy restatements; scipy.ndimage's fill where it imports).  The same checks run on the HIP library in tests/test_gpu_preprocess.py."""
import pytest

from tests import emu_util
from tests import preprocess_checks as K
from tests import preprocess_ref as R
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


@pytest.mark.parametrize("shape", [(37, 46, 53), (21, 26, 30)])
def test_brain_mask_box_crop_emulated(product, shape):
    """the ellipsoid with a cavity, a one-channel pocket and a labelled voxel outside the mask: mask, filled mask, box, crop and seg
    equal the restatement; seg as float32, uint8 and int16"""
    K.check_brain_crop(product, "cpu", shape)


def test_odd_shapes_and_strided_views_emulated(product):
    K.check_shapes_and_strides(product, "cpu")


def test_faces_single_voxel_nan_no_seg_int16_emulated(product):
    K.check_further_cases(product, "cpu")


def test_normalisation_emulated(product):
    """within 4 * 2^-24 * (|x| + |mean|) / std of the float64 restatement, the offset channel (mean 3e4, std 1) included; a constant
    channel gives exact zeros; the masked form leaves the outside bit-equal; two calls are bit-equal"""
    K.check_normalisation(product, "cpu")


def test_class_locations_emulated(product):
    K.check_class_locations("cpu")


def test_preprocess_case_end_to_end_emulated(product):
    data, seg, info = R.brain_case((37, 46, 53))
    K.check_preprocess_case(product, "cpu", data, seg, info)


def test_case_preprocessor_files_emulated(product, tmp_path):
    K.check_case_preprocessor("cpu", tmp_path)


def test_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)
