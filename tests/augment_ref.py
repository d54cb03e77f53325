"""The reference of the augmentation tests (TEST INFRASTRUCTURE): what batchgenerators computes through scipy for the reference's
`get_train_transforms` (light_training/augment/train_augment.py:29-50), restated with numpy in float64 and without scipy.

  spline_coefs_ref     `scipy.ndimage.spline_filter(x, 3, output=float64, mode='mirror')`: per axis the gain 6, `_init_causal_mirror`
                       (the whole finite sum), the causal and the anti-causal recursion with the pole sqrt(3) - 2; axes of length 1
                       are left alone
  spline_values        `map_coordinates(..., order=3, mode='constant', cval, prefilter=False)` at a list of points: cval where a
                       component is < 0 or > n - 1, else the 64 taps with scipy's order-3 weights, tap indices mirrored into the line
  affine_spline3_ref   the two together at p = A (z, y, x)^T + t for every output voxel - batchgenerators' `interpolate_img`
  affine_labels_ref    `interpolate_img(is_seg=True, order=1, cval=-1)`: per label in ascending order
                       `result[map_coordinates(seg == c, order=1, mode='constant', cval=-1) >= 0.5] = c` on zeros
  zoom_nearest_ref     `scipy.ndimage.zoom(order=0, mode='nearest', grid_mode=True)`
  gauss_blur_ref       `scipy.ndimage.gaussian_filter(x_fp32, sigma)`: radius int(4 sigma + 0.5), weights exp(-0.5 / sigma^2 t^2)
                       normalised, 'reflect', the axes in order, each pass summed in float64 in the order of scipy's symmetric
                       correlate1d (centre, then the pairs from the outermost inwards) and rounded to float32

tests/test_augment_ref_cpu.py pins all five to scipy itself."""
import math

import numpy as np

POLE = math.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
NEAR_FACE = 1e-9
NEAR_TIE = 1e-9


# ---- matrices -------------------------------------------------------------------------------------------------------------------------
def rotation(ax, ay, az):
    """Rx Ry Rz as batchgenerators' create_matrix_rotation_{x,y,z}_3d compose them"""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
    return Rx @ Ry @ Rz


def affine_matrix(angles, scale, shape, shift=(0.0, 0.0, 0.0)):
    """[A | t] (3, 4): M = scale * (Rx Ry Rz)^T about the centre (n - 1) / 2, plus a shift of the source coordinate"""
    M = float(scale) * rotation(*angles).T
    ctr = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
    return np.concatenate([M, (ctr - M @ ctr + np.asarray(shift, dtype=np.float64))[:, None]], 1)


def output_points(shape):
    """(D * H * W, 3) float64: the indices (z, y, x) of every voxel"""
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), -1).reshape(-1, 3)


def source_points(matrix, pts):
    m = np.asarray(matrix, dtype=np.float64)
    return pts @ m[:, :3].T + m[:, 3]


def inside(p, shape):
    n = np.asarray(shape, dtype=np.float64) - 1.0
    return ((p >= 0.0) & (p <= n)).all(1)


def near_face(p, shape):
    """points with a component within NEAR_FACE of a face: rounding may put them on either side"""
    n = np.asarray(shape, dtype=np.float64) - 1.0
    return ((np.abs(p) <= NEAR_FACE) | (np.abs(p - n) <= NEAR_FACE)).any(1)


# ---- cubic spline ---------------------------------------------------------------------------------------------------------------------
def _prefilter_axis(a, axis):
    c = np.moveaxis(np.array(a, dtype=np.float64), axis, 0)
    n = c.shape[0]
    if n == 1:
        return np.moveaxis(c, 0, axis)
    c *= GAIN
    z = POLE
    zn1 = z ** (n - 1)
    start = c[0] + zn1 * c[n - 1]
    zi = z
    for i in range(1, n - 1):
        start = start + zi * (c[i] + zn1 * c[n - 1 - i])
        zi *= z
    c[0] = start / (1.0 - zn1 * zn1)
    for i in range(1, n):
        c[i] += z * c[i - 1]
    c[n - 1] = (z * c[n - 2] + c[n - 1]) * z / (z * z - 1.0)
    for i in range(n - 2, -1, -1):
        c[i] = z * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def spline_coefs_ref(x):
    """one volume (any rank) -> float64 coefficients"""
    c = np.asarray(x, dtype=np.float64)
    for ax in range(c.ndim):
        c = _prefilter_axis(c, ax)
    return c


def mirror(q, n):
    """... c b a b c ...: indices mirrored at 0 and at n - 1, any number of times"""
    q = np.asarray(q, dtype=np.int64)
    if n == 1:
        return np.zeros_like(q)
    period = 2 * n - 2
    q = np.mod(q, period)
    return np.where(q > n - 1, period - q, q)


def _cubic(u, n):
    fl = np.floor(u)
    y = u - fl
    zc = 1.0 - y
    w1 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (zc * zc * (zc - 2.0) * 3.0 + 4.0) / 6.0
    w0 = zc * zc * zc / 6.0
    w3 = 1.0 - w0 - w1 - w2
    start = fl.astype(np.int64) - 1
    return [mirror(start + k, n) for k in range(4)], [w0, w1, w2, w3]


def spline_values(coefs, p, cval=0.0):
    """coefs (D, H, W) float64, p (M, 3) -> float64 (M,)"""
    D, H, W = coefs.shape
    ok = inside(p, coefs.shape)
    q = p[ok]
    iz, wz = _cubic(q[:, 0], D)
    iy, wy = _cubic(q[:, 1], H)
    ix, wx = _cubic(q[:, 2], W)
    acc = np.zeros(q.shape[0], dtype=np.float64)
    for a in range(4):
        for b in range(4):
            for c in range(4):
                acc += wz[a] * wy[b] * wx[c] * coefs[iz[a], iy[b], ix[c]]
    out = np.full(p.shape[0], float(cval), dtype=np.float64)
    out[ok] = acc
    return out


def affine_spline3_ref(x, matrix, cval=0.0):
    """one volume (D, H, W) -> (float64 (D, H, W), the source points (D * H * W, 3))"""
    p = source_points(matrix, output_points(x.shape))
    return spline_values(spline_coefs_ref(x), p, cval).reshape(x.shape), p


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
def label_weights_at(seg, p):
    """{label: map_coordinates(seg == label, p, order=1, mode='constant', cval=-1), float64 (M,)}, the labels ascending"""
    seg = np.asarray(seg)
    D, H, W = seg.shape
    ok = inside(p, seg.shape)
    q = p[ok]
    idx, wgt = [], []
    for r, n in enumerate((D, H, W)):
        fl = np.floor(q[:, r])
        y = q[:, r] - fl
        i0 = fl.astype(np.int64)
        idx.append((i0, mirror(i0 + 1, n)))
        wgt.append((1.0 - y, y))
    out = {}
    for l in np.unique(seg):
        ind = (seg == l).astype(np.float64)
        acc = np.zeros(q.shape[0], dtype=np.float64)
        for a in range(2):
            for b in range(2):
                for c in range(2):
                    acc += ind[idx[0][a], idx[1][b], idx[2][c]] * wgt[0][a] * wgt[1][b] * wgt[2][c]
        full = np.full(p.shape[0], -1.0, dtype=np.float64)
        full[ok] = acc
        out[int(l)] = full
    return out


def labels_at(seg, p):
    """-> (int64 (M,), the weights it decided on)"""
    weights = label_weights_at(seg, p)
    out = np.zeros(p.shape[0], dtype=np.int64)
    for l in sorted(weights):
        out[weights[l] >= 0.5] = l
    return out, weights


def affine_labels_ref(seg, matrix):
    """one seg (D, H, W) -> (int64 (D, H, W), {label: weights (D * H * W,)}, the source points)"""
    p = source_points(matrix, output_points(seg.shape))
    out, weights = labels_at(seg, p)
    return out.reshape(seg.shape), weights, p


def near_ties(weights):
    m = None
    for r in weights.values():
        t = np.abs(r - 0.5) <= NEAR_TIE
        m = t if m is None else m | t
    return m


# ---- order-0 zoom ---------------------------------------------------------------------------------------------------------------------
def zoom_nearest_ref(x, new_shape):
    x = np.asarray(x)
    out = x
    for ax, (n_in, n_out) in enumerate(zip(x.shape, new_shape)):
        u = (np.arange(n_out, dtype=np.float64) + 0.5) * (float(n_in) / float(n_out)) - 0.5
        out = np.take(out, np.clip(np.floor(u + 0.5).astype(np.int64), 0, n_in - 1), axis=ax)
    return out


# ---- gaussian blur --------------------------------------------------------------------------------------------------------------------
def gauss_weights(sigma):
    """-> float64 (radius + 1,): [0] the centre"""
    radius = int(4.0 * float(sigma) + 0.5)
    t = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * t ** 2)
    phi = phi / phi.sum()
    return phi[radius:]


def reflect(q, n):
    """d c b a | a b c d"""
    q = np.mod(np.asarray(q, dtype=np.int64), 2 * n)
    return np.where(q > n - 1, 2 * n - 1 - q, q)


def gauss_blur_ref(x, sigma):
    """x float32 (any rank) -> float32"""
    out = np.asarray(x, dtype=np.float32)
    w = gauss_weights(sigma)
    radius = len(w) - 1
    for ax in range(out.ndim):
        line = np.moveaxis(out, ax, 0).astype(np.float64)
        n = line.shape[0]
        i = np.arange(n)
        acc = line * w[0]
        for k in range(radius, 0, -1):
            acc = acc + (line[reflect(i - k, n)] + line[reflect(i + k, n)]) * w[k]
        out = np.moveaxis(acc.astype(np.float32), 0, ax)
    return np.ascontiguousarray(out)


def data_bound(want, xmax):
    """|got - want| <= 2^-23 |want| + 2^-40 max|x| (tests/resample_ref.py): one rounding to fp32 and fp64 reordering"""
    return 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * xmax


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def nested_boxes(shape=(12, 14, 16), dtype=np.int16, high=300):
    """nested boxes of the labels 1, 2, 4 and a block of a label above 255"""
    D, H, W = shape
    seg = np.zeros(shape, dtype=dtype)
    seg[1:D - 1, 1:H - 1, 1:W - 1] = 1
    seg[3:D - 2, 3:H - 3, 3:W - 3] = 2
    seg[5:D - 4, 5:H - 5, 5:W - 5] = 4
    seg[2:5, 9:12, 10:14] = high
    return seg
