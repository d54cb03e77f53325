"""Evaluation of volumes with sides beyond 256 on the HIP library: the checks of tests/test_emu_edt_long.py on the GPU, the label-level
cases at 24 x 300 x 280 (and with z long), and the count of device-to-host copies of the box route."""
import numpy as np
import pytest
import torch

from tests import edt_long_checks as E
from tests import metrics_checks as K
from segmamba_amd import lib as L
from segmamba_amd import metrics as M

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


@pytest.mark.parametrize("shape", E.THIN_SHAPES)
def test_edt_long_int32_every_voxel(hip, shape):
    E.check_int_exact(hip, DEV, shape)


@pytest.mark.parametrize("shape", K.EDT_SHAPES)
def test_edt_long_int32_equals_brute_force_kernel(hip, shape):
    E.check_int_equals_brute_kernel(hip, DEV, shape)


@pytest.mark.parametrize("spacing", K.ANISO)
@pytest.mark.parametrize("shape", E.THIN_SHAPES)
def test_edt_long_fp32(hip, shape, spacing):
    E.check_fp32(hip, DEV, shape, spacing)


@pytest.mark.parametrize("shape,spacing", [(s, K.ANISO[i % 2]) for i, s in enumerate(K.EDT_SHAPES)])
def test_edt_long_fp32_near_brute_force_kernel(hip, shape, spacing):
    E.check_fp32_near_brute_kernel(hip, DEV, shape, spacing)


def test_edt_long_stack_reuse(hip):
    E.check_stack_reuse(hip, DEV)


def test_planes_bbox(hip):
    E.check_planes_bbox(hip, DEV)


@pytest.mark.parametrize("permuted", [False, True], ids=["y_long", "z_long"])
@pytest.mark.parametrize("spacing", [(1, 1, 1), K.ANISO[1]])
def test_box_route_long_kernel(hip, monkeypatch, spacing, permuted):
    """24 x 300 x 280 with the corner island (and the same with z long): every region's box is 299 long, the crops go to edt_sq_long"""
    E.check_label_route(DEV, monkeypatch, E.LONG_CASE, True, permuted, spacing, expect_long=True)


@pytest.mark.parametrize("permuted", [False, True], ids=["y_long", "z_long"])
@pytest.mark.parametrize("spacing", [(1, 1, 1), K.ANISO[1]])
def test_box_route_brute_force_kernel(hip, monkeypatch, spacing, permuted):
    """without the island the boxes measure at most 255 per side: the crops go to edt_sq"""
    E.check_label_route(DEV, monkeypatch, E.LONG_CASE, False, permuted, spacing, expect_long=False)


@pytest.mark.parametrize("case", ["33x47x21", "touches_every_face", "slab", "1x1x1", "wide_row"])
def test_routes_agree_on_small_volumes(hip, monkeypatch, case):
    E.check_route_equality(DEV, monkeypatch, case)


@pytest.mark.parametrize("mode", ["1", "box"])
def test_empty_mask_rules_under_the_switch(hip, monkeypatch, mode):
    E.check_empty_rules_under_switch(DEV, monkeypatch, mode)


def test_distance_transform_edt_long(hip):
    E.check_distance_transform_edt(DEV)


def test_box_route_makes_two_readbacks(hip, monkeypatch):
    """every synchronising call is an error except the two known scalar copies, and there are exactly two of them"""
    pred, gt = E.long_case(E.LONG_CASE, True, False)
    tp, tg = K.dev_t(pred, DEV), K.dev_t(gt, DEV)
    want = M.case_metrics(tp, tg)                                         # warm-up: the region table is uploaded once
    copies = []
    plain = M._readback

    def counted(t):
        torch.cuda.set_sync_debug_mode("default")
        try:
            copies.append(t.numel())
            return plain(t)
        finally:
            torch.cuda.set_sync_debug_mode("error")
    monkeypatch.setattr(M, "_readback", counted)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = M.case_metrics(tp, tg)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    print("device-to-host copies (elements):", copies)
    assert len(copies) == 2 and copies[0] == 5 * 8 + 3 * 6 and copies[1] == 3 * 3
    assert np.array_equal(got, want)


def test_refusals(hip):
    E.check_refusals(hip, DEV)


def test_new_exports_in_the_hip_library(hip):
    E.check_exports(hip)
