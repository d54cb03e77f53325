"""tests/resample_sepz_ref.py (the numpy restatement the separate-z kernels are held to) against tests/golden/resample_sepz.npz -
the reference's own `resample_data_or_seg(do_separate_z=True, order_z=0)`, recorded by tests/golden/make_golden_resample_sepz.py - and
its slice table against scipy's `map_coordinates(order=0, mode='nearest')`, which is what the reference runs along the axis.

Data are held to resample_ref.data_bound around the restatement (the fixture is rounded to float32, which the bound's first term
covers); labels are equal: both fixture cases have dyadic in-plane factors, where every weight is exact."""
import os

import numpy as np
import pytest

from tests import resample_ref as RR
from tests import resample_sepz_ref as SR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_sepz.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_the_stated_cases(golden):
    assert np.array_equal(golden["data"], SR.data_case()[:1]) and np.array_equal(golden["seg"][0], RR.label_case())
    cases = [tuple(int(v) for v in row) for row in golden["data_cases"]]
    assert [c for c in cases if c[4] == 3] == [(a, *s, 3) for a, s in SR.DATA_TARGETS]
    assert [c for c in cases if c[4] == 1] == [(a, *s, 1) for a, s in (SR.DATA_TARGETS[0], SR.DATA_TARGETS[-1])]
    assert [tuple(int(v) for v in row) for row in golden["seg_cases"]] == [(a, *s) for a, s in SR.SEG_TARGETS]


def test_restatement_meets_the_reference_on_data(golden):
    x = golden["data"][0]
    xmax = float(np.abs(x).max())
    for i, row in enumerate(golden["data_cases"]):
        axis, shape, order = int(row[0]), tuple(int(v) for v in row[1:4]), int(row[4])
        want = SR.sepz_data_ref(x, shape, axis, order)
        got = golden[f"data_out_{i}"][0]
        assert got.dtype == np.float32 and got.shape == want.shape
        err, bound = np.abs(got.astype(np.float64) - want), RR.data_bound(want, xmax)
        print(f"axis {axis} -> {shape} order {order}: worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), (axis, shape, order)


def test_stacked_form_is_the_per_slice_form():
    x = SR.data_case()[1]
    for axis, shape in SR.DATA_TARGETS + [(0, (5, 14, 20))]:
        for order in (3, 1):
            a, b = SR.sepz_data_ref(x, shape, axis, order), SR.sepz_data_ref_stacked(x, shape, axis, order)
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-13 * np.abs(x).max(), (axis, shape, order)


def test_restatement_differs_from_the_3d_zoom(golden):
    """the two routes are different functions: by far more than any bound here"""
    x = golden["data"][0]
    axis, shape = SR.DATA_TARGETS[0]
    assert np.abs(SR.sepz_data_ref(x, shape, axis, 3) - RR.zoom_ref(x, shape, 3)).max() > 100.0


def test_restatement_equals_the_reference_on_labels(golden):
    seg = golden["seg"][0]
    for i, row in enumerate(golden["seg_cases"]):
        axis, shape = int(row[0]), tuple(int(v) for v in row[1:4])
        want, weights = SR.sepz_labels_ref(seg, shape, axis)
        for r in weights.values():
            assert np.array_equal(r * 16.0, np.round(r * 16.0)), "dyadic in-plane weights are multiples of 1/16"
        got = golden[f"seg_out_{i}"][0]
        assert got.dtype == np.int16 and np.array_equal(got.astype(np.int64), want), (axis, shape)
        assert {-1, 300} <= set(np.unique(want))


def test_slice_table_equals_map_coordinates():
    ndimage = pytest.importorskip("scipy.ndimage")
    for n_in in range(1, 41):
        stack = np.arange(n_in, dtype=np.float64)
        for n_out in range(1, 41):
            coords = (float(n_in) / n_out) * (np.arange(n_out) + 0.5) - 0.5
            want = ndimage.map_coordinates(stack, coords[None], order=0, mode="nearest")
            assert np.array_equal(SR.slice_table(n_in, n_out), want.astype(np.int64)), (n_in, n_out)


def test_slice_table_of_the_module_is_the_restatement():
    from segmamba_amd import resample as RS
    for n_in, n_out in [(9, 5), (9, 13), (9, 9), (3, 4), (2048, 1024), (120, 240), (1, 7), (7, 1)]:
        got = RS.slice_table(n_in, n_out)
        assert got.dtype == np.int32 and np.array_equal(got, SR.slice_table(n_in, n_out))
