"""The reference of the connectivity tests (TEST INFRASTRUCTURE): connected components at connectivity 1, 2 and 3 in numpy, without
scipy, and the cases shared by tests/test_emu_ccl_conn.py and tests/test_gpu_ccl_conn.py.  Every case and every reference is computed
once and handed out read-only.

`roots(mask, c)` lists every pair of neighbouring mask voxels from the explicit offset list (the previous neighbours of a voxel in
memory order, each pair once) and runs a union-find on that edge list in whole-array steps: hook the larger root of every unsettled
edge below the smaller one (`np.minimum.at`), then halve every chain until none is left.  A parent never exceeds its child, so the
root that a component ends with is its smallest linear index.  tests/test_emu_ccl_conn.py pins it to scipy.ndimage.label."""
import functools
import itertools

import numpy as np

from tests import ccl_labels_ref as LR
from tests import postprocess_ref as R

CONNECTIVITIES = (1, 2, 3)


def previous_offsets(c):
    """the (dz, dy, dx) with at most c non-zero coordinates that come BEFORE the voxel in memory order: 3, 9 or 13 of them"""
    out = [d for d in itertools.product((-1, 0, 1), repeat=3) if d < (0, 0, 0) and sum(v != 0 for v in d) <= c]
    assert len(out) == {1: 3, 2: 9, 3: 13}[c]
    return out


def _edges(m, c):
    """(a, b): linear indices of every pair of mask voxels that are neighbours under c, a the later one"""
    D, H, W = m.shape
    idx = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    a, b = [], []
    for dz, dy, dx in previous_offsets(c):
        def cut(n, d, other):                      # the voxel's range along an axis of n for offset d, or the neighbour's
            lo, hi = max(0, -d), n - max(0, d)
            return slice(lo + d, hi + d) if other else slice(lo, hi)
        me = (cut(D, dz, False), cut(H, dy, False), cut(W, dx, False))
        nb = (cut(D, dz, True), cut(H, dy, True), cut(W, dx, True))
        both = m[me] & m[nb]
        a.append(idx[me][both])
        b.append(idx[nb][both])
    return np.concatenate(a), np.concatenate(b)


def roots(mask, c):
    """int32: -1 outside the mask, else the smallest linear index of the voxel's component at connectivity c"""
    m = np.asarray(mask).astype(bool)
    assert m.ndim == 3 and c in CONNECTIVITIES
    a, b = _edges(m, c)
    parent = np.arange(m.size, dtype=np.int64)
    while a.size:
        pa, pb = parent[a], parent[b]
        open_ = pa != pb
        a, b, pa, pb = a[open_], b[open_], pa[open_], pb[open_]
        if not a.size:
            break
        np.minimum.at(parent, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    return np.where(m.reshape(-1), parent, -1).astype(np.int32).reshape(m.shape)


def label_roots(labels, c):
    """-1 where the label is 0, else the component's smallest linear index: `roots` per class"""
    lab = np.asarray(labels)
    out = np.full(lab.shape, -1, dtype=np.int32)
    for k in np.unique(lab[lab != 0]):
        m = lab == k
        out[m] = roots(m, c)[m]
    return out


def components(r):
    r = np.asarray(r).reshape(-1)
    return int((r == np.arange(r.size)).sum())


def scipy_roots(mask, c):
    """the same from scipy.ndimage.label with generate_binary_structure(3, c): the first voxel of every label in raster order"""
    from scipy import ndimage
    m = np.asarray(mask).astype(bool)
    lab, n = ndimage.label(m, structure=ndimage.generate_binary_structure(3, c))
    first = np.full(n + 1, -1, dtype=np.int64)
    flat = lab.reshape(-1)
    pos = np.flatnonzero(flat)[::-1]
    first[flat[pos]] = pos                                                # descending positions: the smallest is written last
    return np.where(flat > 0, first[flat], -1).astype(np.int32).reshape(m.shape), lab.astype(np.int32), int(n)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _points(shape, pts):
    m = np.zeros(shape, dtype=np.uint8)
    for p in pts:
        m[p] = 1
    return m


HAND_POINTS = ((3, 3, 63), (4, 4, 64),       # corner neighbours across the x, y and z faces of the 64 x 4 x 4 tile
               (1, 3, 10), (1, 4, 11),       # edge neighbours across the y face
               (3, 1, 20), (4, 1, 20))       # face neighbours across the z face
HAND_COMPONENTS = {1: 5, 2: 4, 3: 3}


def hand():
    return _points((6, 6, 70), HAND_POINTS)


def checker(shape=(5, 6, 66)):
    z, y, x = LR._grid(shape)
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def body_centred(shape=(5, 6, 66)):
    """all coordinates even, or all odd: every voxel meets its neighbours through corners only"""
    z, y, x = LR._grid(shape)
    return (((z % 2 == 0) & (y % 2 == 0) & (x % 2 == 0)) | ((z % 2 == 1) & (y % 2 == 1) & (x % 2 == 1))).astype(np.uint8)


# the ten diagonal lines through a voxel (the diagonal directions of the previous-neighbour set, up to sign), x falling as well as rising
STAIR_STEPS = [s for s in itertools.product((0, 1), (-1, 0, 1), (-1, 0, 1))
               if sum(v != 0 for v in s) >= 2 and (s[0] == 1 or s[1] == 1)]
assert len(STAIR_STEPS) == 10
STAIR_LEN = 9


def staircase(step):
    """one voxel per step along `step`, nine steps: z and y run over 0 .. 8 (tile faces at 4 and 8), x over 57 .. 65 (the face at 64),
    rising or falling as the step's sign says; an axis the step does not move along has one plane (x: the plane 64)"""
    n = STAIR_LEN
    shape = (n if step[0] else 1, n if step[1] else 1, 66)
    pts = []
    for k in range(n):
        z = k if step[0] else 0
        y = (k if step[1] > 0 else n - 1 - k) if step[1] else 0
        x = (57 + k if step[2] > 0 else 65 - k) if step[2] else 64
        pts.append((z, y, x))
    return _points(shape, pts)


def stair_name(step):
    return "stair_" + "".join("m0p"[v + 1] for v in step)


def sides(shape):
    """the planes x = 0 and x = width - 1: neighbours in the linear index at every row end, never neighbours in the volume"""
    m = np.zeros(shape, dtype=np.uint8)
    m[:, :, 0] = 1
    m[:, :, -1] = 1
    return m


def side_points(width):
    """voxels whose linear indices are 1, W - 1 or W + 1 apart across a row end or a plane end - none of them neighbours:
    (1,4,W-1) | (2,0,0) adjacent at a plane end;  (1,1,W-1) | (1,3,0) W + 1 apart;  (4,2,0) | (4,2,W-1) the ends of one row"""
    W = width
    return _points((5, 5, W), ((1, 4, W - 1), (2, 0, 0), (1, 1, W - 1), (1, 3, 0), (4, 2, 0), (4, 2, W - 1)))


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


DENSITIES = (0.1, 0.3, 0.6)
TILE_EDGE_SHAPES = [(d, h, w) for w in (63, 64, 65) for h in (3, 4, 5) for d in (3, 4, 5)]
RANDOM_SHAPES = TILE_EDGE_SHAPES + [(9, 10, 131), (40, 48, 136)]

MASKS = {
    "hand": hand,
    "checker_5x6x66": checker,
    "body_centred_5x6x66": body_centred,
    "sides_3x5x64": lambda: sides((3, 5, 64)),
    "sides_3x5x65": lambda: sides((3, 5, 65)),
    "sides_2x3x3": lambda: sides((2, 3, 3)),
    "side_points_64": lambda: side_points(64),
    "side_points_70": lambda: side_points(70),
    "1x1x1": lambda: np.ones((1, 1, 1), np.uint8),
    "1x1x130": lambda: random_mask((1, 1, 130), 0.6, 7),
    "5x1x1": lambda: np.array([1, 1, 0, 1, 1], np.uint8).reshape(5, 1, 1),
    "all_zero": lambda: np.zeros((5, 6, 66), np.uint8),
    "all_one": lambda: np.ones((5, 6, 66), np.uint8),
}
for _s in STAIR_STEPS:
    MASKS[stair_name(_s)] = functools.partial(staircase, _s)
for _i, _shape in enumerate(RANDOM_SHAPES):
    for _d in DENSITIES:
        MASKS["random_%dx%dx%d_%02d" % (_shape + (int(_d * 10),))] = functools.partial(random_mask, _shape, _d, 1000 + 10 * _i + int(_d * 10))

# component counts that the cases state (checked against scipy where it imports): name -> {c: components}
KNOWN = {
    "hand": HAND_COMPONENTS,
    "checker_5x6x66": {1: 990, 2: 1, 3: 1},
    "body_centred_5x6x66": {1: 495, 2: 495, 3: 1},
    "sides_3x5x64": {1: 2, 2: 2, 3: 2}, "sides_3x5x65": {1: 2, 2: 2, 3: 2}, "sides_2x3x3": {1: 2, 2: 2, 3: 2},
    "side_points_64": {1: 6, 2: 6, 3: 6}, "side_points_70": {1: 6, 2: 6, 3: 6},
    "1x1x1": {1: 1, 2: 1, 3: 1}, "5x1x1": {1: 2, 2: 2, 3: 2}, "all_zero": {1: 0, 2: 0, 3: 0}, "all_one": {1: 1, 2: 1, 3: 1},
}
for _s in STAIR_STEPS:
    _n = sum(v != 0 for v in _s)
    KNOWN[stair_name(_s)] = {c: (1 if c >= _n else STAIR_LEN) for c in CONNECTIVITIES}


@functools.lru_cache(maxsize=None)
def mask(name):
    m = np.ascontiguousarray(MASKS[name](), dtype=np.uint8)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def mask_roots(name, c, invert=False):
    r = roots(mask(name) == (0 if invert else 1), c)
    r.setflags(write=False)
    return r


# ---- label volumes -------------------------------------------------------------------------------------------------------------------------
def hand_labels(same):
    """the hand case with one label (5, 4, 3 components) or with the two voxels of every pair labelled differently: six components at
    every connectivity - different labels are never joined, diagonally or not"""
    lab = np.zeros((6, 6, 70), dtype=np.uint8)
    for i, p in enumerate(HAND_POINTS):
        lab[p] = 3 if same else 1 + i % 2
    return lab


def random_labels(shape, density, seed):
    rng = np.random.default_rng(seed)
    return ((rng.random(shape) < density) * rng.integers(1, 4, size=shape)).astype(np.uint8)


def diagonal_island():
    """label 1: a block and an island of two voxels that hangs on it by one corner; label 2: a block with a separate speck"""
    lab = np.zeros((8, 9, 70), dtype=np.uint8)
    lab[1:4, 1:4, 58:64] = 1
    lab[4, 4, 64] = lab[4, 4, 65] = 1                                     # corner neighbour of (3, 3, 63), across three tile faces
    lab[5:7, 5:8, 10:20] = 2
    lab[1, 7, 40] = 2
    return lab


LABELS = {
    "hand_one_label": lambda: hand_labels(True),
    "hand_two_labels": lambda: hand_labels(False),
    "checker_two_labels_4x6x66": lambda: LR.checker2((4, 6, 66)),
    "ten_class_20x30x70": lambda: LR.ten_class((20, 30, 70)),
    "diagonal_island": diagonal_island,
    "labels_5x5x65_03": lambda: random_labels((5, 5, 65), 0.3, 5),
    "labels_4x3x64_06": lambda: random_labels((4, 3, 64), 0.6, 6),
    "labels_3x4x63_06": lambda: random_labels((3, 4, 63), 0.6, 7),
    "labels_9x10x131_06": lambda: random_labels((9, 10, 131), 0.6, 8),
    "labels_13x18x136_03": lambda: random_labels((13, 18, 136), 0.3, 9),
    "ten_class_9x13x70": lambda: LR.ten_class((9, 13, 70), seed=4),
    "labels_1x1x130": lambda: random_labels((1, 1, 130), 0.8, 10),
    "labels_all_zero": lambda: np.zeros((5, 6, 7), np.uint8),
    "labels_all_seven": lambda: np.full((5, 9, 70), 7, np.uint8),
}
KNOWN_LABELS = {"hand_one_label": HAND_COMPONENTS, "hand_two_labels": {1: 6, 2: 6, 3: 6},
                "checker_two_labels_4x6x66": {1: 4 * 6 * 66, 2: 2, 3: 2}}


@functools.lru_cache(maxsize=None)
def labels(name):
    lab = np.ascontiguousarray(LABELS[name](), dtype=np.uint8)
    lab.setflags(write=False)
    return lab


@functools.lru_cache(maxsize=None)
def labels_roots(name, c):
    r = label_roots(labels(name), c)
    r.setflags(write=False)
    return r


def fill_holes(mask_, c=1):
    """mask | (zero voxels whose zero-component at background connectivity c touches no face of the volume)"""
    return R.fill_holes(mask_, roots_fn=lambda m: roots(m, c))


def hollow_cube():
    """the 7^3 shell `[1:6]^3` minus `[2:5]^3` with the corner voxel (1, 1, 1) removed: 97 voxels.  The 27 voxels inside reach the
    outside through that corner only: a hole for a background of connectivity 1 and 2 (filled: 124), none at 3 (97)"""
    m = np.zeros((7, 7, 7), dtype=np.uint8)
    m[1:6, 1:6, 1:6] = 1
    m[2:5, 2:5, 2:5] = 0
    m[1, 1, 1] = 0
    return m
