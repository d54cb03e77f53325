"""The reference of the post-processing tests (TEST INFRASTRUCTURE): connected components at connectivity 1, component sizes, the
largest component, hole filling and scipy's numbering restated with numpy only, written from the definitions; the trilinear
resampling rule of F.interpolate(align_corners=False) in fp64; and the case builders shared by tests/test_emu_postprocess.py and
tests/test_gpu_postprocess.py."""
import numpy as np

from tests import metrics_ref as MR

BRATS_REGIONS = MR.BRATS_REGIONS


# ---- components -------------------------------------------------------------------------------------------------------------------
def roots_propagate(mask):
    """-1 outside the mask, else the smallest linear index of the voxel's component: minimum-index propagation over the six shifts
    until nothing changes (exact; needs as many rounds as the longest path)"""
    m = np.asarray(mask).astype(bool)
    big = np.iinfo(np.int64).max
    lab = np.where(m, np.arange(m.size, dtype=np.int64).reshape(m.shape), big)
    while True:
        p = np.pad(lab, 1, constant_values=big)
        n = np.minimum.reduce([p[1:-1, 1:-1, 1:-1], p[:-2, 1:-1, 1:-1], p[2:, 1:-1, 1:-1], p[1:-1, :-2, 1:-1], p[1:-1, 2:, 1:-1],
                               p[1:-1, 1:-1, :-2], p[1:-1, 1:-1, 2:]])
        n = np.where(m, n, big)
        if np.array_equal(n, lab):
            break
        lab = n
    return np.where(m, lab, -1).astype(np.int32)


def roots_union_find(mask):
    """the same by a plain union-find over the voxel list (for long thin paths)"""
    m = np.asarray(mask).astype(bool)
    D, H, W = m.shape
    parent = np.arange(m.size, dtype=np.int64)
    flat = m.reshape(-1)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    for i in np.flatnonzero(flat):
        z, rem = divmod(int(i), H * W)
        y, x = divmod(rem, W)
        for ok, j in ((x > 0, i - 1), (y > 0, i - W), (z > 0, i - H * W)):
            if ok and flat[j]:
                a, b = find(int(i)), find(int(j))
                if a != b:
                    parent[max(a, b)] = min(a, b)
    out = np.full(m.size, -1, dtype=np.int32)
    for i in np.flatnonzero(flat):
        out[i] = find(int(i))
    return out.reshape(m.shape)


def sizes_from_roots(roots):
    """(sizes, touches): the component's voxel count at its root voxel (0 elsewhere); 1 at the roots of components with a voxel on a face"""
    r = np.asarray(roots).reshape(-1)
    inside = r >= 0
    sizes = np.bincount(r[inside], minlength=r.size).astype(np.int32)
    face = np.zeros(roots.shape, dtype=bool)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = True, True, True, True, True, True
    touches = np.zeros(r.size, dtype=np.uint8)
    touches[np.unique(r[inside & face.reshape(-1)])] = 1
    return sizes.reshape(roots.shape), touches.reshape(roots.shape)


def largest(mask, roots=None):
    """the largest component; equal counts: the one whose root comes LAST in memory order (the stated rule); empty stays empty"""
    roots = roots_propagate(mask) if roots is None else roots
    sizes, _ = sizes_from_roots(roots)
    s = sizes.reshape(-1)
    if not s.any():
        return np.zeros(roots.shape, dtype=np.uint8)
    winner = np.flatnonzero(s == s.max())[-1]
    return (roots == winner).astype(np.uint8)


def min_size(mask, n, roots=None):
    roots = roots_propagate(mask) if roots is None else roots
    sizes, _ = sizes_from_roots(roots)
    keep = sizes.reshape(-1)[np.maximum(roots, 0)] >= n
    return ((roots >= 0) & keep).astype(np.uint8)


def fill_holes(mask, roots_fn=roots_propagate):
    """mask | (zero voxels whose zero-component touches no face of the volume)"""
    m = np.asarray(mask).astype(bool)
    r = roots_fn(~m)
    _, touches = sizes_from_roots(r)
    hole = (r >= 0) & (touches.reshape(-1)[np.maximum(r, 0)] == 0)
    return (m | hole).astype(np.uint8)


def largest_connected_domain(mask):
    return fill_holes(largest(mask))


def number(roots):
    """scipy.ndimage.label's numbering: components 1 .. num in memory order of their first voxel"""
    r = np.asarray(roots).reshape(-1)
    is_root = r == np.arange(r.size)
    rank = np.cumsum(is_root).astype(np.int32)
    return np.where(r >= 0, rank[np.maximum(r, 0)], 0).astype(np.int32).reshape(roots.shape), int(is_root.sum())


def postprocess_labels(labels, regions=BRATS_REGIONS, keep="largest", fill=True):
    out = np.asarray(labels).astype(np.uint8).copy()
    for reg in regions:
        m = MR.region_mask(out, reg)
        kept = largest(m) if keep == "largest" else min_size(m, keep)
        if fill:
            kept = fill_holes(kept)
        out[m & (kept == 0)] = 0
    return out


# ---- the same with scipy (callers importorskip) ---------------------------------------------------------------------------------------
def scipy_label(mask):
    from scipy import ndimage
    lab, num = ndimage.label(np.asarray(mask).astype(bool))
    return lab.astype(np.int32), int(num)


def scipy_fill(mask):
    from scipy import ndimage
    return ndimage.binary_fill_holes(np.asarray(mask).astype(bool)).astype(np.uint8)


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def serpentine(shape):
    """a path one voxel thick through every second row of every second plane, each row joined to the next at alternating ends and
    each plane to the next where its path ended: ONE component whose geodesic length is about a quarter of the volume"""
    D, H, W = shape
    m = np.zeros(shape, dtype=np.uint8)
    rows = list(range(0, H, 2))
    x = 0
    for z in range(0, D, 2):
        for k, y in enumerate(rows):
            m[z, y, :] = 1
            x = W - 1 - x                                  # the row is walked to its other end
            if k + 1 < len(rows):
                y2 = rows[k + 1]
                m[z, min(y, y2):max(y, y2) + 1, x] = 1
        if z + 2 < D:
            m[z:z + 3, rows[-1], x] = 1
        rows = rows[::-1]
    return m


def checkerboard(shape):
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def cubes(shape, touch):
    """two 3^3 cubes that meet only along an edge (touch = "edge") or only at a corner ("corner")"""
    m = np.zeros(shape, dtype=np.uint8)
    m[1:4, 1:4, 1:4] = 1
    if touch == "edge":
        m[1:4, 4:7, 4:7] = 1
    else:
        m[4:7, 4:7, 4:7] = 1
    return m


def crossing(shape=(17, 70, 131)):
    """one component that crosses every tile boundary (64 x 4 x 4 tiles) in all three axes: three orthogonal bars through the volume
    plus a diagonal staircase, and a few separate specks"""
    D, H, W = shape
    m = np.zeros(shape, dtype=np.uint8)
    m[D // 2, H // 2, :] = 1
    m[D // 2, :, W // 3] = 1
    m[:, H // 2, (2 * W) // 3] = 1
    for k in range(min(D, H) - 1):                         # a staircase of face-adjacent steps from (0, 0, 5) on
        m[k, k, 5:8] = 1
        m[k + 1, k, 5] = 1
        m[k + 1, k:k + 2, 5] = 1
    m[D - 1, H - 1, W - 1] = 1
    m[0, H - 1, 0] = 1
    m[D - 1, 0, W - 2:] = 1
    return m


def shell(shape, lo, hi):
    """the faces of the box [lo, hi] (inclusive) as a closed one-voxel shell"""
    m = np.zeros(shape, dtype=np.uint8)
    m[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = 1
    m[lo[0] + 1:hi[0], lo[1] + 1:hi[1], lo[2] + 1:hi[2]] = 0
    return m


def hole_cases():
    """name -> (mask, expected number of voxels that filling adds)"""
    shp = (14, 15, 70)
    closed = shell(shp, (2, 2, 3), (9, 10, 68))
    inner = (9 - 2 - 1) * (10 - 2 - 1) * (68 - 3 - 1)
    tunnel = closed.copy()
    tunnel[5, 5, 3] = 0                                   # one voxel of the wall removed
    cup = shell(shp, (0, 2, 3), (9, 10, 68))
    cup[0] = 0                                            # the opening lies on the z = 0 face
    cup_inner = 0
    nested = closed | shell(shp, (4, 4, 10), (7, 8, 40))
    diag = shell(shp, (2, 2, 3), (9, 10, 68))
    diag[2, 2, 3:69] = 0                                  # an edge of the box removed: the cavity meets the outside only diagonally
    return {"closed_shell": (closed, inner), "tunnel": (tunnel, 0), "cup_on_face": (cup, cup_inner),
            "shell_in_shell": (nested, inner - int(shell(shp, (4, 4, 10), (7, 8, 40)).sum())), "diagonal_gap": (diag, inner)}


def tie_case():
    """two components of 12 voxels each and a smaller one: the later of the two large ones is the stated winner"""
    m = np.zeros((6, 9, 70), dtype=np.uint8)
    m[1, 1:3, 2:8] = 1
    m[4, 5:7, 60:66] = 1
    m[2, 7, 30:35] = 1
    return m


# ---- the label map ----------------------------------------------------------------------------------------------------------------------
def source_axis(out_n, in_n):
    """(i0, i1, lambda) per output index of F.interpolate(mode="trilinear", align_corners=False); the coordinate in fp32 as the rule
    states it, the weights then exact in fp64"""
    ratio = np.float32(in_n) / np.float32(out_n)
    src = np.maximum((np.arange(out_n, dtype=np.float32) + np.float32(0.5)) * ratio - np.float32(0.5), np.float32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_n - 1)
    i1 = np.minimum(i0 + 1, in_n - 1)
    return i0, i1, src.astype(np.float64) - i0


def resample_fp64(logits, out_shape):
    """(C, d, h, w) -> (C, D, H, W) in fp64"""
    v = np.asarray(logits, dtype=np.float64)
    for ax, n in enumerate(out_shape):
        i0, i1, lam = source_axis(n, v.shape[ax + 1])
        shp = [1, 1, 1, 1]
        shp[ax + 1] = n
        lam = lam.reshape(shp)
        v = np.take(v, i0, axis=ax + 1) * (1.0 - lam) + np.take(v, i1, axis=ax + 1) * lam
    return v


def paste(labels, out_shape, start):
    full = np.zeros(out_shape, dtype=np.uint8)
    z, y, x = start
    full[z:z + labels.shape[0], y:y + labels.shape[1], x:x + labels.shape[2]] = labels
    return full


def smooth_logits(shape, classes=4, seed=0, amplitude=4.0, noise=0.3):
    """low-resolution noise upsampled (amplitude 4) plus white noise of 0.3, fp32"""
    import torch
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(seed)
    low = torch.randn(1, classes, 5, 6, 5, generator=g) * amplitude
    v = F.interpolate(low, size=tuple(shape), mode="trilinear", align_corners=True)[0]
    return (v + noise * torch.randn(v.shape, generator=g)).contiguous()


def tie_logits(shape, seed=1):
    """integer-valued logits with deliberate ties between classes 0 and 2, 1 and 3, and all four"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-3, 4, size=(4,) + tuple(shape)).astype(np.float32)
    k = rng.integers(0, 4, size=shape)
    v[2][k == 0] = v[0][k == 0]
    v[3][k == 1] = v[1][k == 1]
    for c in (1, 2, 3):
        v[c][k == 2] = v[0][k == 2]
    return v
