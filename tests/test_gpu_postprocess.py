"""Device-side prediction finishing (segmamba_amd/postprocess.py) on the HIP library: the checks of tests/test_emu_postprocess.py on
the GPU, plus the case at BraTS size whose reference is the same label propagation written with plain ATen ops on the device."""
import numpy as np
import pytest
import torch

from tests import metrics_checks as MK
from tests import metrics_ref as MR
from tests import postprocess_checks as K
from tests import postprocess_ref as R
from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("case", sorted(K.MASK_CASES))
def test_components_sizes_numbering(hip, case):
    K.check_components(hip, DEV, K.MASK_CASES[case]())


@pytest.mark.parametrize("shape", [(12, 22, 70), (5, 9, 131), (9, 6, 3), (40, 60, 200)])
def test_serpentine_terminates(hip, shape):
    m = R.serpentine(shape)
    K.check_components(hip, DEV, m, reference=R.roots_union_find)
    assert PP.component_summary(K.dev_t(m, DEV)) == (1, int(m.sum()))


@pytest.mark.parametrize("case", sorted(K.KNOWN_SIZES))
def test_known_component_sizes(hip, case):
    K.check_known_sizes(DEV, case)


def test_label_equals_scipy(hip):
    pytest.importorskip("scipy.ndimage")
    for case in ("33x47x21_pred_wt", "40x48x36_pred_tc", "checkerboard", "crossing_17x70x131", "tie"):
        K.check_components(hip, DEV, K.MASK_CASES[case](), with_scipy=True)


@pytest.mark.parametrize("case", ["33x47x21_pred_wt", "33x47x21_gt_wt", "33x47x21_pred_shell", "40x48x36_pred_tc", "cubes_edge",
                                  "crossing_17x70x131", "full", "1x1x1", "slab", "empty"])
def test_largest_fill_and_min_size(hip, case):
    K.check_selection(DEV, K.MASK_CASES[case]())


def test_selection_against_scipy(hip):
    pytest.importorskip("scipy.ndimage")
    for case in ("33x47x21_pred_wt", "33x47x21_pred_shell", "40x48x36_pred_tc", "crossing_17x70x131"):
        K.check_selection(DEV, K.MASK_CASES[case](), with_scipy=True)


@pytest.mark.parametrize("case", sorted(R.hole_cases()))
def test_holes(hip, case):
    K.check_holes(DEV, case)


def test_tie_rule_min_size_boundaries_and_empty(hip):
    K.check_tie_and_boundaries(DEV)


@pytest.mark.parametrize("shape", [(33, 47, 21), (40, 48, 36)])
def test_postprocess_labels(hip, shape):
    K.check_postprocess_labels(DEV, MR.small_case(shape)[0])


def test_wrapper_refusals(hip):
    K.check_refusals(hip, DEV)


def test_new_exports_in_the_hip_library(hip):
    K.check_exports(hip)


def test_argmax_identity_ties_dtypes_strides(hip):
    K.check_argmax_identity(hip, DEV)
    K.check_argmax_identity(hip, DEV, shape=(20, 33, 128))


def test_paste_and_region_planes(hip):
    K.check_paste_and_regions(hip, DEV)


def test_resampling_band_rule(hip):
    K.check_resampling(hip, DEV)


def test_predict_labels_equals_the_three_reference_steps(hip):
    K.check_predict_labels(DEV)


# ---- at BraTS size -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brats():
    return MR.brats_size_case()


# name -> (mask from the prediction, component sizes largest first, voxels that filling adds): computed with scipy when the case was written
BRATS_MASKS = {"TC": ((1, 3), [87173, 4894, 64], 0), "WT": ((1, 2, 3), [340210, 64], 0), "ET": ((3,), [52733, 64], 0),
               "label2": ((2,), [248143], 92067)}


@pytest.mark.parametrize("name", sorted(BRATS_MASKS))
def test_brats_size_components_against_aten_propagation(hip, brats, name):
    """155 x 240 x 240 (tests/metrics_ref.brats_size_case): roots, sizes, largest component and filling against minimum-index propagation
    written with ATen ops on the device (and scipy where it imports).  Conditions on the input first: the component sizes and the
    number of voxels that filling adds."""
    pred, _ = brats
    reg, want_sizes, want_added = BRATS_MASKS[name]
    mask = K.dev_t(MR.region_mask(pred, reg).astype(np.uint8), DEV)
    ref_roots = K.torch_roots(mask)
    cnt = torch.bincount(ref_roots[ref_roots >= 0].long())
    ref_sizes = sorted(cnt[cnt > 0].tolist(), reverse=True)
    ref_fill = K.torch_fill(mask)
    added = int(ref_fill.sum().item()) - int(mask.sum().item())
    print(name, "reference component sizes", ref_sizes, "filling adds", added)
    assert ref_sizes == want_sizes and added == want_added                  # conditions on the input
    roots = ops_raw.ccl_roots(hip, mask)
    assert torch.equal(roots, ref_roots)
    assert torch.equal(roots, ops_raw.ccl_roots(hip, mask))
    sizes, touches = ops_raw.ccl_sizes(hip, roots)
    want = torch.zeros(mask.numel(), dtype=torch.int32, device=DEV)
    want[:len(cnt)] = cnt.to(torch.int32)
    assert torch.equal(sizes.reshape(-1), want)
    assert PP.component_summary(mask) == (len(want_sizes), want_sizes[0])
    assert torch.equal(PP.binary_fill_holes(mask), ref_fill)
    assert torch.equal(PP.largest_connected_domain(mask), K.torch_fill(K.torch_largest(mask)))
    labels, num = PP.label(mask)
    assert num == len(want_sizes)
    try:
        from scipy import ndimage
    except ImportError:
        return
    sl, sn = ndimage.label(mask.cpu().numpy())
    assert sn == num and np.array_equal(labels.cpu().numpy(), sl)
    assert np.array_equal(ref_fill.cpu().numpy(), ndimage.binary_fill_holes(mask.cpu().numpy()).astype(np.uint8))


def test_brats_size_postprocess_labels(hip, brats):
    pred, _ = brats
    t = K.dev_t(pred, DEV)
    got = PP.postprocess_labels(t)
    want = t.clone()
    tab = M._table(MR.BRATS_REGIONS, torch.device(DEV))
    for r in range(3):
        inside = ((tab[want.long()] >> r) & 1).bool()
        kept = K.torch_fill(K.torch_largest(inside.to(torch.uint8)))
        want[inside & (kept == 0)] = 0
    assert torch.equal(got, want)
    assert int((got != t).sum().item()) == 4894 + 64                        # the second lobe (labels 1 / 2 of TC) and the island go


def test_brats_size_metrics_after_largest_connected_domain(hip, brats):
    """The two device stages together: Dice / Hausdorff distance of each region's `largest_connected_domain(prediction mask)` against the
    ground truth.  Reference figures (scipy: largest component, holes filled, medpy's definitions), before -> after:
      HD    TC 158.066 -> 30.249, WT 141.651 -> 8.0623, ET 162.718 -> 7.0
      Dice  TC 0.834821 -> 0.812856, WT 0.887626 -> 0.887703, ET 0.811569 -> 0.812023
    The test recomputes: Dice from the reference masks' counts (exact), the distance by brute force on the device over the reference
    masks' borders (1e-6 relative)."""
    pred, gt = brats
    for reg in MR.BRATS_REGIONS:
        p, g = MR.region_mask(pred, reg).astype(np.uint8), MR.region_mask(gt, reg).astype(np.uint8)
        tp, tg = K.dev_t(p, DEV), K.dev_t(g, DEV)
        ref_mask = K.torch_fill(K.torch_largest(tp))
        got_mask = PP.largest_connected_domain(tp)
        assert torch.equal(got_mask, ref_mask)
        rm = ref_mask.cpu().numpy().astype(bool)
        want_dice = 2.0 * int((rm & g.astype(bool)).sum()) / float(int(rm.sum()) + int(g.sum()))
        pa, pb = np.argwhere(MR.border(rm)), np.argwhere(MR.border(g.astype(bool)))
        ab, ba = MK.torch_min_sq_dist(pa, pb, None, DEV), MK.torch_min_sq_dist(pb, pa, None, DEV)
        want_hd = float(np.sqrt(np.hstack((ab, ba)).astype(np.float64)).max())
        have_dice, have_hd = M.dc(got_mask, tg), M.hd(got_mask, tg)
        print("region", reg, "before: dice", M.dc(tp, tg), "hd", M.hd(tp, tg), "after: dice", have_dice, "hd", have_hd,
              "reference", want_dice, want_hd)
        assert have_dice == want_dice
        assert abs(have_hd - want_hd) <= 1e-6 * want_hd
