"""The reference of the labelled connected-components tests (TEST INFRASTRUCTURE): components of a label map restated per class with
the numpy union-find of tests/postprocess_ref.py, the per-class selection rules, and the label-map cases shared by
tests/test_emu_ccl_labels.py and tests/test_gpu_ccl_labels.py.  Every reference is computed once per case and handed out read-only."""
import functools

import numpy as np

from tests import metrics_ref as MR
from tests import postprocess_ref as R


# ---- components per class -----------------------------------------------------------------------------------------------------------
def label_roots(labels):
    """-1 where the label is 0, else the smallest linear index of the voxel's component: a union-find per class"""
    lab = np.asarray(labels)
    out = np.full(lab.shape, -1, dtype=np.int32)
    for c in np.unique(lab[lab != 0]):
        m = lab == c
        out[m] = R.roots_union_find(m)[m]
    return out


def class_sizes(labels, roots):
    """{label: (roots of its components in memory order, their sizes)}"""
    lab, r = np.asarray(labels).reshape(-1), np.asarray(roots).reshape(-1)
    cnt = np.bincount(r[r >= 0], minlength=r.size)
    out = {}
    for c in np.unique(lab[lab != 0]):
        rs = np.flatnonzero((cnt > 0) & (lab == c))
        out[int(c)] = (rs, cnt[rs])
    return out


def info(labels, roots):
    """(256, 3) int64: components, the root of the largest (equal sizes: the LAST in memory; -1: absent), its size"""
    out = np.zeros((256, 3), dtype=np.int64)
    out[:, 1] = -1
    for c, (rs, sz) in class_sizes(labels, roots).items():
        k = np.flatnonzero(sz == sz.max())[-1]
        out[c] = (len(rs), rs[k], sz[k])
    return out


def select(labels, roots, mode, min_size=0, apply=None):
    """mode "largest": a voxel keeps its label iff its root is its label's winner; "min_size": iff its component has at least
    `min_size` voxels; labels with apply[l] == 0 pass through"""
    lab = np.asarray(labels)
    out = np.zeros_like(lab)
    for c, (rs, sz) in class_sizes(lab, roots).items():
        m = lab == c
        if apply is not None and not apply[c]:
            out[m] = c
            continue
        keep = [rs[np.flatnonzero(sz == sz.max())[-1]]] if mode == "largest" else rs[sz >= min_size]
        out[m & np.isin(roots, keep)] = c
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")


def stripes(shape, axis):
    """label 1 + (coordinate % 3) along `axis`, constant along the other two: one-voxel-thick sheets, no background"""
    return (1 + _grid(shape)[axis] % 3).astype(np.uint8)


def checker2(shape):
    z, y, x = _grid(shape)
    return (1 + (z + y + x) % 2).astype(np.uint8)


def rows_1122(shape):
    return (1 + (_grid(shape)[2] // 2) % 2).astype(np.uint8)


def with_complement(mask):
    return np.where(np.asarray(mask) != 0, 1, 2).astype(np.uint8)


def shell_around_ball(shape=(12, 13, 70), lo=(2, 2, 3), hi=(9, 10, 68)):
    out = R.shell(shape, lo, hi)
    out[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = 2
    return out


def high_labels():
    out = np.zeros((6, 9, 70), dtype=np.uint8)
    out[1:3, 1:4, 2:30] = 1
    out[1:3, 4:7, 2:30] = 127                                             # touches label 1 along a face: not joined
    out[3:5, 1:7, 20:68] = 128
    out[0, 0, 60:70] = 255
    out[5, 8, 0:3] = 255
    out[5, 8, 5] = 1
    return out


def tie_labels():
    """two components of 12 voxels of label 1 (the later one is the stated winner) and a smaller one, beside 30 voxels of label 2"""
    out = R.tie_case()
    out[2, 7, 35:65] = 2                                                  # continues the 5-voxel run of label 1 along x: not joined
    return out


def apply_case():
    out = high_labels()
    out[out == 127] = 2
    out[0, 8, 10:14] = 2                                                  # second components of 2 and 255: they must survive
    return out


def ten_class(shape, seed=0):
    """nine blobs (labels 1 .. 9), each with two small islands elsewhere, and speckle of single voxels of random labels"""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.arange(D, dtype=np.float32), np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij",
                          sparse=True)
    out = np.zeros(shape, dtype=np.uint8)
    for c in range(1, 10):
        cz, cy, cx = ((c - 1) // 3 + 0.5) * D / 3, ((c - 1) % 3 + 0.5) * H / 3, (0.3 + 0.05 * c) * W
        out[((z - cz) / (0.14 * D)) ** 2 + ((y - cy) / (0.14 * H)) ** 2 + ((x - cx) / (0.2 * W)) ** 2 < 1.0] = c
    for c in range(1, 10):
        for _ in range(2):
            p = [int(rng.integers(0, n - 3)) for n in shape]
            blk = out[p[0]:p[0] + 3, p[1]:p[1] + 3, p[2]:p[2] + 3]
            blk[blk == 0] = c
    n = max(8, out.size // 4000)
    idx = rng.integers(0, out.size, size=n)
    flat = out.reshape(-1)
    free = flat[idx] == 0
    flat[idx[free]] = rng.integers(1, 10, size=int(free.sum())).astype(np.uint8)
    return out


def random_runs(shape, seed):
    """labels 0 .. 3 at random in runs of two voxels along x: many small components that meet every face of the volume"""
    D, H, W = shape
    rng = np.random.default_rng(seed)
    return np.repeat(rng.integers(0, 4, size=(D, H, (W + 1) // 2)), 2, axis=2)[:, :, :W].astype(np.uint8)


CASES = {
    "stripes_x": lambda: stripes((5, 6, 70), 2),
    "stripes_y": lambda: stripes((5, 14, 70), 1),
    "stripes_z": lambda: stripes((10, 6, 70), 0),
    "checker_4x6x66": lambda: checker2((4, 6, 66)),
    "rows_1122": lambda: rows_1122((5, 6, 70)),
    "crossing_17x70x131": lambda: with_complement(R.crossing((17, 70, 131))),
    "serpentine_5x9x131": lambda: with_complement(R.serpentine((5, 9, 131))),
    "shell_around_ball": shell_around_ball,
    "33x47x21": lambda: MR.small_case((33, 47, 21))[0],
    "40x48x36": lambda: MR.small_case((40, 48, 36), shift=(2, 1, -2))[0],
    "labels_1_127_128_255": high_labels,
    "tie": tie_labels,
    "all_zero": lambda: np.zeros((5, 6, 7), np.uint8),
    "all_one_label": lambda: np.full((5, 9, 70), 7, np.uint8),
    "1x1x1": lambda: np.full((1, 1, 1), 3, np.uint8),
    "line_1x1x200": lambda: (1 + np.arange(200) % 2).astype(np.uint8).reshape(1, 1, 200),
    "ten_class_20x30x70": lambda: ten_class((20, 30, 70)),
}
# the sides 1 below, at and 1 above the tile's (64 x 4 x 4): the shapes tools/ccl_labels_sanitize.cpp runs too
for _w in (63, 64, 65):
    for _h in (3, 4, 5):
        CASES[f"tile_edge_{_h}x{_h}x{_w}"] = functools.partial(lambda h, w: random_runs((h, h, w), h * 100 + w), _h, _w)


@functools.lru_cache(maxsize=None)
def case(name):
    """(labels, reference roots), computed once and read-only"""
    lab = np.ascontiguousarray(CASES[name](), dtype=np.uint8)
    roots = label_roots(lab)
    lab.setflags(write=False)
    roots.setflags(write=False)
    return lab, roots
