"""The reference of the resampling tests (TEST INFRASTRUCTURE): what the reference's `resample_data_or_seg` computes without a
separate z axis, restated with numpy in float64 and without scipy.

Data: skimage's `resize(x, new_shape, order, mode='edge', anti_aliasing=False)`, which for n-D input is
`scipy.ndimage.zoom(x, out / in, order=order, mode='nearest', grid_mode=True)`.  Per axis, for order 3: the line padded by 12 edge
copies, multiplied by the filter gain (6), the causal and anti-causal recursion with the pole sqrt(3) - 2 under mirror boundary
conditions, then the four cubic B-spline weights at u = (i + 0.5) * (n_in / n_out) - 0.5 + 12.  Order 1 has no prefilter and no pad:
the coordinate is clamped to [0, n_in - 1].  The recursions run over whole slabs at once (one numpy statement per step of a line).

Seg: batchgenerators' `resize_segmentation(seg, new_shape, 1)`: per label in ascending order the order-1 zoom of its indicator,
`out[r >= 0.5] = label` on a volume of zeros.

tests/test_resample_ref_cpu.py pins both to scipy.ndimage.zoom where scipy imports."""
import math

import numpy as np

POLE = math.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
NPAD = 12
NEAR_TIE = 1e-9


def prefilter_axis(a, axis):
    """a float64; -> the spline coefficients of the line padded by 12 edge copies on both sides: n + 24 along `axis`"""
    a = np.moveaxis(np.asarray(a, dtype=np.float64), axis, 0)
    n = a.shape[0]
    idx = np.clip(np.arange(-NPAD, n + NPAD), 0, n - 1)
    c = a[idx] * GAIN
    N = n + 2 * NPAD
    z = POLE
    zn1 = z ** (N - 1)
    start = c[0] + zn1 * c[N - 1]
    zi = z
    for i in range(1, min(N - 1, 64)):                                # the pole's 64th power is 5e-35: the later terms add nothing
        start = start + zi * (c[i] + zn1 * c[N - 1 - i])
        zi *= z
    c[0] = start / (1.0 - zn1 * zn1)
    for i in range(1, N):
        c[i] += z * c[i - 1]
    c[N - 1] = (z * c[N - 2] + c[N - 1]) * z / (z * z - 1.0)
    for i in range(N - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def coordinates(n_in, n_out, order):
    """-> (first tap index (into the padded line for order 3), weights (order + 1, n_out))"""
    ratio = float(n_in) / float(n_out)
    u = (np.arange(n_out, dtype=np.float64) + 0.5) * ratio - 0.5
    if order == 3:
        u = u + NPAD
        fl = np.floor(u)
        y = u - fl
        zc = 1.0 - y
        w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
        w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
        w0 = zc * zc * zc / 6.0
        w3 = 1.0 - w0 - w1 - w2
        return fl.astype(np.int64) - 1, np.stack([w0, w1, w2, w3])
    u = np.clip(u, 0.0, float(n_in - 1))
    fl = np.floor(u)
    y = u - fl
    return fl.astype(np.int64), np.stack([1.0 - y, y])


def _gather_axis(c, axis, start, weights, limit):
    c = np.moveaxis(c, axis, 0)
    out = None
    for k in range(weights.shape[0]):
        term = c[np.clip(start + k, 0, limit - 1)] * weights[k].reshape((-1,) + (1,) * (c.ndim - 1))
        out = term if out is None else out + term
    return np.moveaxis(out, 0, axis)


def zoom_ref(x, new_shape, order=3, clip=True):
    """one volume (D, H, W) -> float64 new_shape; equal shapes give the input"""
    x64 = np.asarray(x, dtype=np.float64)
    new_shape = tuple(int(v) for v in new_shape)
    assert order in (1, 3) and x64.ndim == len(new_shape)
    if tuple(x64.shape) == new_shape:
        return x64
    c = x64
    if order == 3:
        for ax in range(c.ndim):
            c = prefilter_axis(c, ax)
    for ax in range(x64.ndim):
        start, w = coordinates(x64.shape[ax], new_shape[ax], order)
        c = _gather_axis(c, ax, start, w, c.shape[ax])
    if clip:
        c = np.clip(c, x64.min(), x64.max())
    return c


def label_weights(seg, new_shape):
    """{label: the order-1 zoom of its indicator, float64}, the labels ascending"""
    seg = np.asarray(seg)
    return {int(l): zoom_ref((seg == l).astype(np.float64), new_shape, order=1, clip=True) for l in np.unique(seg)}


def zoom_labels_ref(seg, new_shape, weights=None):
    """-> (the resized label volume, int64; the weights it decided on)"""
    seg = np.asarray(seg)
    new_shape = tuple(int(v) for v in new_shape)
    if tuple(seg.shape) == new_shape:
        return seg.astype(np.int64), {}
    weights = label_weights(seg, new_shape) if weights is None else weights
    out = np.zeros(new_shape, dtype=np.int64)
    for l in sorted(weights):
        out[weights[l] >= 0.5] = l
    return out, weights


def near_ties(weights):
    """voxels where some label's weight lies within NEAR_TIE of 0.5"""
    m = None
    for r in weights.values():
        t = np.abs(r - 0.5) <= NEAR_TIE
        m = t if m is None else m | t
    return m


def reachable(got, weights):
    """whether `got` is, per voxel, one of the values reached by deciding every near-tied label either way"""
    got = np.asarray(got).astype(np.int64)
    lowest = min(weights) - 1
    strict = np.full(got.shape, lowest, dtype=np.int64)                # the largest label surely at or above 0.5
    for l in sorted(weights):
        strict[weights[l] > 0.5 + NEAR_TIE] = l
    ok = got == np.where(strict == lowest, 0, strict)
    for l, r in weights.items():
        ok |= (np.abs(r - 0.5) <= NEAR_TIE) & (got == l) & (l > strict)
    return ok


def label_counts(seg):
    """the 260 bins of segm_crop_normalize's counts for an integer volume with values >= -1"""
    seg = np.asarray(seg).astype(np.int64)
    c = np.zeros(260, dtype=np.int64)
    c[256] = int((seg < 0).sum())
    c[257] = int((seg > 255).sum())
    inside = seg[(seg >= 0) & (seg <= 255)]
    c[:256] = np.bincount(inside, minlength=256)
    return c


def data_bound(want, xmax):
    """|got - want| <= 2^-23 |want| + 2^-40 max|x|: the rounding to fp32 plus one flipped rounding, and fp64 noise through the
    prefilter (gain at most 27 over three axes, some hundred operations)"""
    return 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * xmax


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def step_edge(shape=(12, 14, 20)):
    """0 in one half and 100 in the other, along x: cubic interpolation overshoots on both sides of the edge"""
    x = np.zeros(shape, dtype=np.float32)
    x[:, :, shape[2] // 2:] = 100.0
    return x


def label_case(shape=(12, 14, 16), dtype=np.int16, high=300):
    """-1 around the rim, nested blocks of labels 1, 2 and `high`, and one cell of 2 x 2 x 2 voxels at even indices that three
    labels share 3 : 3 : 2 - at a factor of 0.5 its output voxel gives no label one half, at a factor of 2 the output voxels near
    its centre do not either"""
    seg = np.zeros(shape, dtype=dtype)
    seg[:2], seg[:, :2], seg[:, :, :2] = -1, -1, -1
    D, H, W = shape
    seg[3:D - 2, 3:H - 2, 3:W - 2] = 1
    seg[5:D - 3, 5:H - 4, 6:W - 4] = 2
    seg[6:8, 6:9, 7:10] = high
    a, b, c = D - 2, H - 2, W - 2
    assert a % 2 == 0 and b % 2 == 0 and c % 2 == 0
    cell = seg[a:a + 2, b:b + 2, c:c + 2]
    cell[0, 0, 0], cell[0, 0, 1], cell[0, 1, 0] = 1, 1, 1
    cell[0, 1, 1], cell[1, 0, 0], cell[1, 0, 1] = 2, 2, 2
    cell[1, 1, 0], cell[1, 1, 1] = high, high
    return seg


def ellipsoid_labels(shape=(24, 28, 30)):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    r2 = ((z - 11.3) / 8.7) ** 2 + ((y - 13.1) / 10.2) ** 2 + ((x - 14.6) / 11.9) ** 2
    seg = np.zeros(shape, dtype=np.int16)
    seg[r2 <= 1.0] = 1
    seg[r2 <= 0.3] = 2
    seg[:, :, :1] = -1
    return seg
