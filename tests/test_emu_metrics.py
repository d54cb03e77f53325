"""Device-side evaluation (segmamba_amd/metrics.py on csrc/metrics.hip) with the kernel sources compiled for the CPU emulator:
borders and counts, the exact squared distance transform, Dice / surface distances / HD95 / HD, the reference's empty-mask rules,
wrapper refusals and the exports.  References: tests/metrics_ref.py (numpy brute force; scipy.ndimage where it imports).  The same
checks run on the HIP library in tests/test_gpu_metrics.py."""
import numpy as np
import pytest
import torch

from tests import emu_util
from tests import metrics_checks as K
from tests import metrics_ref as R
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.metrics on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


@pytest.mark.parametrize("case", sorted(K.LABEL_CASES))
def test_borders_and_counts_emulated(emu, case):
    """bit-equal border planes and equal integer counts: odd sides, a mask on every face of the volume, disconnected pieces, 1 x 1 x 1,
    a 1-thick slab, a row longer than one wave"""
    K.check_borders_and_counts(emu, "cpu", *K.LABEL_CASES[case]())


@pytest.mark.parametrize("shape", K.EDT_SHAPES)
def test_edt_unit_spacing_bit_equal_emulated(emu, shape):
    """int32 squared distances equal brute force at every voxel: a far island, one set voxel, all set, nothing set, lines longer than 64"""
    K.check_edt(emu, "cpu", shape)


@pytest.mark.parametrize("shape,spacing", [((33, 47, 21), K.ANISO[0]), ((40, 48, 36), K.ANISO[1]), ((5, 7, 150), K.ANISO[0]),
                                           ((3, 130, 9), K.ANISO[1]), ((140, 4, 5), K.ANISO[0]), ((1, 1, 1), K.ANISO[1])])
def test_edt_anisotropic_spacing_emulated(emu, shape, spacing):
    """fp32 squared distances within 1e-6 relative of fp64 brute force (three terms of at most two roundings each and two rounded
    additions: 5 * 2^-24 = 3e-7; the reference takes the spacing as rounded to fp32)"""
    K.check_edt(emu, "cpu", shape, spacing)


def test_edt_and_borders_against_scipy_emulated(emu):
    pytest.importorskip("scipy.ndimage")
    K.check_edt_against_scipy(emu, "cpu", (33, 47, 21))


@pytest.mark.parametrize("case", ["33x47x21", "40x48x36", "touches_every_face", "slab", "wide_row"])
def test_dice_surface_distances_hd95_hd_emulated(product, case):
    """Dice exactly, the sorted distance lists at unit spacing exactly (fp32), hd95 / hd within 1e-6 relative, for all three regions and
    three spacings"""
    K.check_binary_metrics("cpu", *K.LABEL_CASES[case]())


def test_hd95_against_scipy_emulated(product):
    pytest.importorskip("scipy.ndimage")
    K.check_binary_metrics("cpu", *K.LABEL_CASES["33x47x21"](), spacings=(None, K.ANISO[0]), with_scipy=True)


@pytest.mark.parametrize("case,spacing", [("33x47x21", (1, 1, 1)), ("40x48x36", K.ANISO[1]), ("touches_every_face", (1, 1, 1)),
                                          ("1x1x1", (1, 1, 1)), ("wide_row", K.ANISO[0])])
def test_case_metrics_emulated(product, case, spacing):
    K.check_case("cpu", *K.LABEL_CASES[case](), spacing)


def test_empty_mask_rules_and_evaluate_emulated(product):
    """prediction lacks ET -> [0.0, 50] for that region only; both lack ET -> [0.0, 50] but validation Dice 1.0; surface distances of an
    empty mask raise; evaluate, region_masks and distance_transform_edt"""
    K.check_empty_rules("cpu")


def test_wrapper_refusals_emulated(product):
    K.check_refusals(product, "cpu")


def test_new_exports_emulated(emu):
    K.check_exports(emu)


def test_compute_metrics_tool_emulated(product, tmp_path):
    """tools/compute_metrics.py: .npy predictions against .npz ground truth of the same name, the saved (cases, regions, 2) array"""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("compute_metrics_tool", os.path.join(emu_util.ROOT, "tools", "compute_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    want = []
    for i in range(2):
        pred, gt = R.small_case((20 + i, 30, 25))
        np.save(tmp_path / "pred" / f"case{i}.npy", pred)
        np.save(tmp_path / "gt" / f"case{i}.npy", gt)
        want.append(R.case_metrics(pred, gt))
    np.save(tmp_path / "pred" / "unmatched.npy", pred)
    out = tmp_path / "result" / "metrics.npy"
    res = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--out", str(out)])
    assert res.shape == (2, 3, 2) and np.array_equal(np.load(out), res)
    assert np.allclose(res, np.stack(want), rtol=1e-6, atol=0.0)
    with pytest.raises(RuntimeError):
        tool.main(["--pred", str(tmp_path / "result"), "--gt", str(tmp_path / "gt")])
