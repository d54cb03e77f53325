"""Device-side evaluation (segmamba_amd/metrics.py) on the HIP library: the checks of tests/test_emu_metrics.py on the GPU, plus one
case at BraTS size whose brute-force reference runs on the device with plain ATen ops."""
import numpy as np
import pytest
import torch

from tests import metrics_checks as K
from tests import metrics_ref as R
from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("case", sorted(K.LABEL_CASES))
def test_borders_and_counts(hip, case):
    K.check_borders_and_counts(hip, DEV, *K.LABEL_CASES[case]())


@pytest.mark.parametrize("shape", K.EDT_SHAPES)
def test_edt_unit_spacing_bit_equal(hip, shape):
    K.check_edt(hip, DEV, shape)


@pytest.mark.parametrize("shape,spacing", [((33, 47, 21), K.ANISO[0]), ((40, 48, 36), K.ANISO[1]), ((5, 7, 150), K.ANISO[0]),
                                           ((3, 130, 9), K.ANISO[1]), ((140, 4, 5), K.ANISO[0]), ((1, 1, 1), K.ANISO[1])])
def test_edt_anisotropic_spacing(hip, shape, spacing):
    K.check_edt(hip, DEV, shape, spacing)


def test_edt_and_borders_against_scipy(hip):
    pytest.importorskip("scipy.ndimage")
    K.check_edt_against_scipy(hip, DEV, (33, 47, 21))


@pytest.mark.parametrize("case", ["33x47x21", "40x48x36", "touches_every_face", "slab", "wide_row"])
def test_dice_surface_distances_hd95_hd(hip, case):
    K.check_binary_metrics(DEV, *K.LABEL_CASES[case]())


@pytest.mark.parametrize("case,spacing", [("33x47x21", (1, 1, 1)), ("40x48x36", K.ANISO[1]), ("touches_every_face", (1, 1, 1)),
                                          ("1x1x1", (1, 1, 1)), ("wide_row", K.ANISO[0])])
def test_case_metrics(hip, case, spacing):
    K.check_case(DEV, *K.LABEL_CASES[case](), spacing)


def test_empty_mask_rules_and_evaluate(hip):
    K.check_empty_rules(DEV)


def test_wrapper_refusals(hip):
    K.check_refusals(hip, DEV)


def test_new_exports_in_the_hip_library(hip):
    K.check_exports(hip)


# ---- at BraTS size ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brats():
    pred, gt = R.brats_size_case()
    return pred, gt, R.counts(pred, gt), R.border_planes(pred), R.border_planes(gt)


@pytest.mark.parametrize("spacing", [(1, 1, 1), (1.0, 1.2, 0.9)])
def test_brats_size_case_all_regions(hip, brats, spacing):
    """155 x 240 x 240, analytic rippled ellipsoids (tests/metrics_ref.brats_size_case), all three regions against integer / fp64 brute
    force over the border voxels, computed on the device with ATen.  The case, as generated on the host (reference figures):
      voxels   |P| 92131 / 340274 / 52797, |G| 107356 / 396976 / 61579 (TC / WT / ET)
      borders  |dP| 9853 / 23183 / 6242, |dG| 10886 / 25680 / 6886
      Dice     0.834821 / 0.887626 / 0.811569
      spacing (1, 1, 1):      HD95 5.744563 / 6.480741 / 5.744563, HD 158.0664 / 141.6510 / 162.7175
      spacing (1, 1.2, 0.9):  HD95 5.807753 / 6.502307 / 5.621388, HD 164.4760 / 147.9804 / 169.3262
    Checks: counts and Dice exact, hd95 / hd within 1e-6 relative, two calls bit-equal."""
    pred, gt, want_counts, bpred, bgt = brats
    # conditions on the inputs: every region non-empty on both sides, border counts that keep the brute force affordable
    assert (want_counts[:2] > 0).all()
    assert (want_counts[3:] >= 5e3).all() and (want_counts[3:] <= 1.5e5).all(), want_counts[3:].tolist()
    tp, tg = K.dev_t(pred, DEV), K.dev_t(gt, DEV)
    borders, counts = ops_raw.seg_regions(hip, tp, tg, K.table(DEV))
    got_counts = counts.cpu().numpy()
    print("counts", got_counts[:, :3].tolist())
    assert np.array_equal(got_counts[:, :3], want_counts) and not got_counts[:, 3:].any()
    assert np.array_equal(borders[0].cpu().numpy(), bpred) and np.array_equal(borders[1].cpu().numpy(), bgt)
    got = M.case_metrics(tp, tg, spacing)
    sp = None if all(s == 1 for s in spacing) else spacing
    for r, reg in enumerate(R.BRATS_REGIONS):
        pa, pb = np.argwhere((bpred >> r) & 1), np.argwhere((bgt >> r) & 1)
        assert len(pa) * len(pb) <= 2.25e10
        ab, ba = K.torch_min_sq_dist(pa, pb, sp, DEV), K.torch_min_sq_dist(pb, pa, sp, DEV)
        joined = np.sqrt(np.hstack((ab, ba)).astype(np.float64))
        want_dice = 2.0 * int(want_counts[2, r]) / float(int(want_counts[0, r]) + int(want_counts[1, r]))
        want_hd95, want_hd = float(np.percentile(joined, 95)), float(joined.max())
        a, b = K.dev_t(R.region_mask(pred, reg).astype(np.uint8), DEV), K.dev_t(R.region_mask(gt, reg).astype(np.uint8), DEV)
        have_hd = M.hd(a, b, sp)
        print("region", reg, "spacing", spacing, "dice", got[r, 0], "hd95", got[r, 1], "hd", have_hd, "reference", want_dice, want_hd95, want_hd)
        assert got[r, 0] == want_dice == M.dc(a, b)
        assert abs(got[r, 1] - want_hd95) <= 1e-6 * want_hd95
        assert abs(have_hd - want_hd) <= 1e-6 * want_hd
        assert M.hd95(a, b, sp) == got[r, 1]
        if sp is None:                                                    # the distance lists themselves, in voxel order
            assert np.array_equal(M.surface_distances(a, b).cpu().numpy(), np.sqrt(ab.astype(np.float64)).astype(np.float32))
    # repeatability: bit-equal results of two calls
    assert np.array_equal(M.case_metrics(tp, tg, spacing), got)
    planes = [(v, r) for r in range(3) for v in (0, 1)]
    e1, e2 = ops_raw.edt_sq(hip, borders, planes, sp), ops_raw.edt_sq(hip, borders, planes, sp)
    assert torch.equal(e1, e2)
    items = [(0, r, 2 * r + 1) for r in range(3)]
    cnt = [int(want_counts[3, r]) for r in range(3)]
    assert torch.equal(ops_raw.border_distances(hip, borders, e1, items, cnt), ops_raw.border_distances(hip, borders, e2, items, cnt))


def test_brats_size_int32_edt_equals_scipy(hip, brats):
    """the int32 distance transform of all six border planes at 155 x 240 x 240 equals scipy.ndimage.distance_transform_edt squared"""
    pytest.importorskip("scipy.ndimage")
    pred, gt, _, bpred, bgt = brats
    borders = K.dev_t(np.stack([bpred, bgt]), DEV)
    planes = [(v, r) for r in range(3) for v in (0, 1)]
    e = ops_raw.edt_sq(hip, borders, planes).cpu().numpy()
    for i, (v, r) in enumerate(planes):
        assert np.array_equal(e[i].astype(np.int64), R.scipy_edt_sq_int(((bpred, bgt)[v] >> r) & 1)), (v, r)
