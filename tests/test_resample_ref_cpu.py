"""tests/resample_ref.py (the numpy restatement the resampling kernels are held to) against scipy.ndimage.zoom, which is what
skimage's `resize` runs for n-D input: orders 3 and 1 within 1e-12 * max|x| (measured: some 1e-14 on unit-variance noise; the margin
covers the order of summation), and the label rule against the per-label loop of batchgenerators' `resize_segmentation`."""
import numpy as np
import pytest

from tests import resample_ref as RR

ndimage = pytest.importorskip("scipy.ndimage")

SHAPES_1D = [(9, 31), (17, 26), (17, 34), (30, 20), (40, 13), (1, 5), (5, 1), (2, 3)]
SHAPES_3D = [((11, 13, 9), (22, 20, 6)), ((7, 1, 12), (9, 1, 24)), ((10, 12, 8), (8, 15, 8)), ((6, 5, 300), (9, 5, 150))]


def _scipy_zoom(x, new_shape, order):
    x = np.asarray(x, dtype=np.float64)
    return ndimage.zoom(x, [o / i for o, i in zip(new_shape, x.shape)], order=order, mode="nearest", grid_mode=True)


@pytest.mark.parametrize("order", [3, 1])
def test_restatement_equals_scipy_zoom(order):
    rng = np.random.RandomState(0)
    worst = 0.0
    for n_in, n_out in SHAPES_1D:
        x = rng.standard_normal(n_in)
        got, want = RR.zoom_ref(x, (n_out,), order, clip=False), _scipy_zoom(x, (n_out,), order)
        assert want.shape == (n_out,)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(x).max()))
    for shape, new_shape in SHAPES_3D:
        x = rng.standard_normal(shape)
        got, want = RR.zoom_ref(x, new_shape, order, clip=False), _scipy_zoom(x, new_shape, order)
        assert want.shape == tuple(new_shape)
        worst = max(worst, float(np.abs(got - want).max() / np.abs(x).max()))
    print(f"order {order}: worst |restatement - scipy| / max|x| = {worst:.3g}")
    assert worst <= 1e-12


def test_clip_is_the_input_range():
    x = RR.step_edge()
    free = RR.zoom_ref(x, (12, 14, 40), 3, clip=False)
    assert free.min() < 0.0 and free.max() > 100.0
    got = RR.zoom_ref(x, (12, 14, 40), 3, clip=True)
    assert got.min() == 0.0 and got.max() == 100.0
    assert np.abs(got - np.clip(_scipy_zoom(x, (12, 14, 40), 3), 0.0, 100.0)).max() <= 1e-12 * 100.0


def _scipy_labels(seg, new_shape):
    out = np.zeros(new_shape, dtype=np.int64)
    weights = {}
    for c in np.unique(seg):
        r = np.clip(_scipy_zoom((seg == c).astype(float), new_shape, 1), 0.0, 1.0)
        out[r >= 0.5] = c
        weights[int(c)] = r
    return out, weights


@pytest.mark.parametrize("new_shape", [(24, 14, 16), (12, 28, 32), (6, 7, 8), (24, 28, 32), (6, 14, 16)])
def test_labels_equal_the_per_label_loop_dyadic(new_shape):
    seg = RR.label_case()
    got, weights = RR.zoom_labels_ref(seg, new_shape)
    want, _ = _scipy_labels(seg, new_shape)
    assert np.array_equal(got, want)
    assert not RR.near_ties(weights).all()


@pytest.mark.parametrize("factor", [(1.5, 1.0, 1.0), (1.5, 1.5, 1.5), (0.8, 1.25, 1.0)])
def test_labels_equal_the_per_label_loop_off_ties(factor):
    seg = RR.ellipsoid_labels()
    new_shape = tuple(int(round(n * f)) for n, f in zip(seg.shape, factor))
    got, weights = RR.zoom_labels_ref(seg, new_shape)
    want, sw = _scipy_labels(seg, new_shape)
    near = RR.near_ties(weights)
    print(f"factor {factor}: near-ties {near.mean():.4f} of the voxels")
    assert near.mean() <= 0.05
    assert np.array_equal(got[~near], want[~near])
    assert RR.reachable(want, weights).all() and RR.reachable(got, weights).all()
    for l in weights:
        assert np.abs(weights[l] - sw[l]).max() <= 1e-12
