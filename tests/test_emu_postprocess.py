"""Device-side prediction finishing (segmamba_amd/postprocess.py on csrc/postprocess.hip and csrc/ccl_roots.hip) with the
kernel sources compiled for the CPU emulator: connected components, sizes, selection, hole filling, numbering, the logits -> label
map kernel, wrapper refusals and the exports.  References: tests/postprocess_ref.py (numpy restatements; scipy.ndimage where it imports).  The same checks run on the HIP
library in tests/test_gpu_postprocess.py."""
import numpy as np
import pytest
import torch

from tests import emu_util
from tests import postprocess_checks as K
from tests import postprocess_ref as R
from tests import metrics_ref as MR
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.postprocess on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("case", sorted(K.MASK_CASES))
def test_components_sizes_numbering_emulated(product, case):
    """roots (the smallest linear index of the component), sizes, face flags, the device arg-max and scipy's numbering, for the mask and
    for its complement: blobs with islands, the checkerboard (every voxel its own component), cubes that touch along an edge / at a
    corner only, a component across every tile boundary with sides that are no multiples of the tile, empty, full, 1 x 1 x 1, a slab"""
    K.check_components(product, "cpu", K.MASK_CASES[case]())


@pytest.mark.parametrize("shape", [(12, 22, 70), (5, 9, 131), (9, 6, 3)])
def test_serpentine_terminates_emulated(product, shape):
    """the longest path a volume can hold, one voxel thick: one component, its complement too is long and thin"""
    m = R.serpentine(shape)
    K.check_components(product, "cpu", m, reference=R.roots_union_find)
    from segmamba_amd import postprocess as PP
    assert PP.component_summary(m) == (1, int(m.sum()))


@pytest.mark.parametrize("case", sorted(K.KNOWN_SIZES))
def test_known_component_sizes_emulated(product, case):
    K.check_known_sizes("cpu", case)


def test_label_equals_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    for case in ("33x47x21_pred_wt", "40x48x36_pred_tc", "checkerboard", "crossing_17x70x131", "tie"):
        K.check_components(product, "cpu", K.MASK_CASES[case](), with_scipy=True)


@pytest.mark.parametrize("case", ["33x47x21_pred_wt", "33x47x21_gt_wt", "33x47x21_pred_shell", "40x48x36_pred_tc", "cubes_edge",
                                  "crossing_17x70x131", "full", "1x1x1", "slab", "empty"])
def test_largest_fill_and_min_size_emulated(product, case):
    K.check_selection("cpu", K.MASK_CASES[case]())


def test_shell_fill_adds_959_emulated(product):
    """`pred == 2` of the 33 x 47 x 21 case is one shell of 2672 voxels whose filling adds 959"""
    from segmamba_amd import postprocess as PP
    m = K.MASK_CASES["33x47x21_pred_shell"]()
    assert int(m.sum()) == 2672
    assert int(PP.binary_fill_holes(m).sum().item()) - 2672 == 959


def test_selection_against_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    for case in ("33x47x21_pred_wt", "33x47x21_pred_shell", "40x48x36_pred_tc", "crossing_17x70x131"):
        K.check_selection("cpu", K.MASK_CASES[case](), with_scipy=True)


@pytest.mark.parametrize("case", sorted(R.hole_cases()))
def test_holes_emulated(product, case):
    """a closed shell is filled; with a one-voxel tunnel, or as a cup that opens on a face of the volume, it is not; a shell inside a
    shell: everything inside the outer one; a cavity whose only gap is diagonal is filled (the background is 6-connected too)"""
    K.check_holes("cpu", case)


def test_holes_against_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    for case in sorted(R.hole_cases()):
        K.check_holes("cpu", case, with_scipy=True)


def test_tie_rule_min_size_boundaries_and_empty_emulated(product):
    K.check_tie_and_boundaries("cpu")


@pytest.mark.parametrize("shape", [(33, 47, 21), (40, 48, 36)])
def test_postprocess_labels_emulated(product, shape):
    K.check_postprocess_labels("cpu", MR.small_case(shape)[0])


def test_wrapper_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)


def test_argmax_identity_ties_dtypes_strides_emulated(emu):
    K.check_argmax_identity(emu, "cpu")


def test_paste_and_region_planes_emulated(product):
    K.check_paste_and_regions(product, "cpu")


def test_resampling_band_rule_emulated(emu):
    K.check_resampling(emu, "cpu")


def test_predict_labels_equals_the_three_reference_steps_emulated(product):
    K.check_predict_labels("cpu")
