"""tests/augment_ref.py (the numpy restatements the augmentation kernels are held to) against scipy itself: `spline_filter`,
`map_coordinates`, `zoom` and `gaussian_filter`, called the way batchgenerators calls them for the reference's transforms."""
import numpy as np
import pytest

from tests import augment_ref as AR

ndimage = pytest.importorskip("scipy.ndimage")

SHAPES = [(12, 14, 16), (7, 33, 9), (5, 2, 300), (6, 1, 9)]
MATRICES = [((0.3, -0.2, 0.45), 0.85), ((-0.52, 0.52, 0.1), 1.35), ((0.0, 0.0, 0.0), 0.7), ((0.05, -0.04, 0.03), 0.7)]


def _volume(shape, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(shape) * 40.0 + 3.0).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES + [(9,), (2,), (1,), (45,)])
def test_coefficients_equal_scipy_spline_filter(shape):
    x = _volume(shape, 1)
    want = ndimage.spline_filter(x, 3, output=np.float64, mode="mirror")
    got = AR.spline_coefs_ref(x)
    assert got.dtype == np.float64 and np.abs(got - want).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("shape", SHAPES)
def test_warp_equals_scipy_map_coordinates(shape):
    """batchgenerators' interpolate_img: map_coordinates(x.astype(float64), coords, order=3, mode='constant', cval=0)"""
    x = _volume(shape, 2)
    inside = 0
    for angles, scale in MATRICES:
        m = AR.affine_matrix(angles, scale, shape)
        got, p = AR.affine_spline3_ref(x, m)
        coords = p.T.reshape((3,) + shape)
        want = ndimage.map_coordinates(x.astype(np.float64), coords, order=3, mode="constant", cval=0.0)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max(), (shape, angles, scale)
        inside += int(AR.inside(p, shape).sum())
    assert inside > 0
    # random points that include both faces and locations just outside them
    rng = np.random.RandomState(5)
    pts = rng.uniform(-1.0, 1.0, (400, 3)) * 0.6 * np.asarray(shape) + (np.asarray(shape) - 1) / 2.0
    pts[:40] = np.round(pts[:40])
    pts[40:60, 0], pts[60:80, 1], pts[80:100, 2] = 0.0, shape[1] - 1.0, shape[2] - 1.0
    pts[100:110, 2] = shape[2] - 1.0 + 1e-7
    got = AR.spline_values(AR.spline_coefs_ref(x), pts, cval=-7.0)
    want = ndimage.map_coordinates(x.astype(np.float64), pts.T, order=3, mode="constant", cval=-7.0)
    assert AR.inside(pts, shape).sum() >= 20 and (~AR.inside(pts, shape)).sum() >= 20
    assert np.abs(got - want).max() <= 1e-12 * np.abs(x).max()


@pytest.mark.parametrize("dtype", [np.int16, np.int64])
def test_labels_equal_the_per_label_loop(dtype):
    """interpolate_img(is_seg=True, order=1, cval=-1) on scipy, label by label"""
    seg = AR.nested_boxes(dtype=dtype)
    cases = [AR.affine_matrix(a, s, seg.shape) for a, s in MATRICES[:3]] + [AR.affine_matrix((0, 0, 0), 1.0, seg.shape, shift=(0, 0, 0.5))]
    for m in cases:
        got, weights, p = AR.affine_labels_ref(seg, m)
        coords = p.T.reshape((3,) + seg.shape)
        want = np.zeros(seg.shape, dtype=np.int64)
        for c in np.unique(seg):
            r = ndimage.map_coordinates((seg == c).astype(float), coords, order=1, mode="constant", cval=-1.0)
            assert np.abs(r.reshape(-1) - weights[int(c)]).max() <= 1e-12
            want[r >= 0.5] = c
        assert np.array_equal(got, want)
        assert set(np.unique(got)) <= set(np.unique(seg).tolist()) | {0}


def test_nearest_zoom_equals_scipy():
    rng = np.random.RandomState(3)
    for n_in, n_out in ((128, 64), (128, 96), (16, 8), (16, 12), (12, 9), (10, 5), (1, 3), (5, 8), (7, 1)):
        x = rng.standard_normal(n_in).astype(np.float32)
        want = ndimage.zoom(x, n_out / n_in, order=0, mode="nearest", grid_mode=True)
        assert np.array_equal(AR.zoom_nearest_ref(x, (n_out,)), want), (n_in, n_out)
    x = rng.standard_normal((16, 12, 10)).astype(np.float32)
    new = (12, 9, 5)
    want = ndimage.zoom(x, [o / i for o, i in zip(new, x.shape)], order=0, mode="nearest", grid_mode=True)
    assert np.array_equal(AR.zoom_nearest_ref(x, new), want)


@pytest.mark.parametrize("sigma", [0.5, 0.62, 0.63, 0.7, 0.87, 0.88, 1.0])
def test_blur_is_bit_equal_to_scipy_gaussian_filter(sigma):
    for shape, seed in (((10, 12, 14), 7), ((3, 5, 40), 8), ((1, 2, 9), 9)):
        x = _volume(shape, seed)
        want = ndimage.gaussian_filter(x, sigma)
        got = AR.gauss_blur_ref(x, sigma)
        assert got.dtype == np.float32 and want.dtype == np.float32
        assert np.array_equal(got, want), (sigma, shape, float(np.abs(got - want).max()))
    assert len(AR.gauss_weights(0.62)) - 1 == 2 and len(AR.gauss_weights(0.63)) - 1 == 3
    assert len(AR.gauss_weights(0.87)) - 1 == 3 and len(AR.gauss_weights(0.88)) - 1 == 4
