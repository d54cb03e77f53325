"""The reference of the case-preparation tests (TEST INFRASTRUCTURE): the steps of the reference's `run_case_npy` - non-zero mask,
hole filling, bounding box, crop with the -1 rule, z-score, class locations, seg dtype, properties - restated with numpy from their
definitions, and the deterministic case builders shared by tests/test_emu_preprocess.py and tests/test_gpu_preprocess.py.
The fill is scipy.ndimage.binary_fill_holes where scipy imports and tests/postprocess_ref.py's own fill otherwise."""
import math

import numpy as np

from tests import postprocess_ref as PR


# ---- the steps ------------------------------------------------------------------------------------------------------------------------
def nonzero_mask(data):
    """OR over the channels of `data[c] != 0` (NaN != 0 is True)"""
    m = np.zeros(data.shape[1:], dtype=bool)
    for c in range(data.shape[0]):
        m |= data[c] != 0
    return m


def fill(mask):
    try:
        from scipy import ndimage
    except ImportError:
        return PR.fill_holes(mask).astype(bool)
    return ndimage.binary_fill_holes(np.asarray(mask).astype(bool))


def bbox_of(mask):
    """[[z0, z1], [y0, y1], [x0, x1]], half-open"""
    out = []
    for ax in range(3):
        other = tuple(a for a in range(3) if a != ax)
        idx = np.flatnonzero(mask.any(axis=other))
        out.append([int(idx[0]), int(idx[-1]) + 1])
    return out


def crop_to_nonzero(data, seg=None, nonzero_label=-1, fill_fn=fill):
    """-> (data crop, seg crop (1, d, h, w), bbox, filled mask)"""
    filled = fill_fn(nonzero_mask(data))
    bb = bbox_of(filled)
    sl = tuple(slice(a, b) for a, b in bb)
    d = data[(slice(None),) + sl]
    m = filled[sl][None]
    if seg is not None:
        s = np.array(seg[(slice(None),) + sl])
        s[(s == 0) & ~m] = nonzero_label
    else:
        s = np.where(m, 0, nonzero_label).astype(np.int8)
    return d, s, bb, filled


def zscore64(x, inside=None):
    """one channel in float64: (x - mean) / max(std, 1e-8) with the population std, over `inside` only when given (the rest is
    returned as it is).  -> (result, mean, std)"""
    x64 = np.asarray(x, dtype=np.float64)
    sel = x64 if inside is None else x64[inside]
    mean, std = float(sel.mean()), float(sel.std())
    out = (x64 - mean) / max(std, 1e-8)
    if inside is not None:
        out = np.where(inside, out, x64)
    return out, mean, std


def zscore32_literal(x, inside=None):
    """the reference's own arithmetic: float32 throughout, numpy's float32 mean() and std()"""
    image = np.array(x, dtype=np.float32)
    if inside is not None:
        mean, std = image[inside].mean(), image[inside].std()
        image[inside] = (image[inside] - mean) / max(std, 1e-8)
        return image
    mean, std = image.mean(), image.std()
    return (image - mean) / max(std, 1e-8)


def zscore_bound(x, mean, std):
    """4 * 2^-24 * (|x| + |mean|) / std per voxel: mean and std carry one fp32 rounding each, the subtraction and the division one each"""
    return 4.0 * 2.0 ** -24 * (np.abs(np.asarray(x, dtype=np.float64)) + abs(mean)) / max(std, 1e-8)


def sample_locations(seg, classes_or_regions, seed=1234):
    rndst = np.random.RandomState(seed)
    out = {}
    for c in classes_or_regions:
        k = tuple(c) if isinstance(c, list) else c
        labels = list(c) if isinstance(c, (tuple, list)) else [c]
        locs = np.argwhere(np.isin(seg, labels))
        if len(locs) == 0:
            out[k] = []
            continue
        n = max(min(10000, len(locs)), int(math.ceil(len(locs) * 0.01)))
        out[k] = locs[rndst.choice(len(locs), n, replace=False)]
    return out


def run_case(data, seg, spacing, out_spacing=(1, 1, 1), all_labels=(1, 2, 3), mask_norm=False, fill_fn=fill):
    """-> (data float64 (C, d, h, w), seg (1, d, h, w) int8 / int16, properties, per-channel (mean, std), filled mask)"""
    d, s, bb, filled = crop_to_nonzero(np.asarray(data, dtype=np.float32), None if seg is None else np.asarray(seg, dtype=np.float32),
                                       fill_fn=fill_fn)
    inside = (s[0] >= 0) if mask_norm else None
    chans, stats = [], []
    for c in range(d.shape[0]):
        o, mean, std = zscore64(d[c], inside)
        chans.append(o)
        stats.append((mean, std))
    locs = sample_locations(s, all_labels)
    s = s.astype(np.int16 if s.max() > 127 else np.int8)
    props = {"original_spacing_trans": [float(v) for v in list(spacing)[::-1]], "target_spacing_trans": list(out_spacing),
             "shape_before_cropping": list(data.shape[1:]), "bbox_used_for_cropping": bb,
             "shape_after_cropping_before_resample": list(d.shape[1:]), "shape_after_resample": list(d.shape[1:]),
             "class_locations": locs}
    return np.stack(chans), s, props, stats, filled


# ---- cases ------------------------------------------------------------------------------------------------------------------------------
def _grid(shape):
    return np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")


def brain_case(shape=(37, 46, 53), centre=None, radii=None, seed=0):
    """An ellipsoid "brain" in four fp32 channels (non-zero everywhere inside, zero outside) with
      * a cavity that is zero in all channels (filling closes it),
      * a pocket that is zero in channel 2 only (the OR over the channels does not see it),
      * a seg of nested labels 1 - 3 inside the brain, 0 elsewhere,
      * one voxel of label 2 outside the ellipsoid but inside its bounding box.
    -> (data (4, D, H, W) float32, seg (1, D, H, W) float32, info)"""
    shape = tuple(shape)
    centre = tuple(round(n * f) for n, f in zip(shape, (0.52, 0.53, 0.49))) if centre is None else tuple(centre)
    radii = tuple(min(c, n - 1 - c) - 2.5 for c, n in zip(centre, shape)) if radii is None else tuple(radii)
    z, y, x = _grid(shape)
    r2 = ((z - centre[0]) / radii[0]) ** 2 + ((y - centre[1]) / radii[1]) ** 2 + ((x - centre[2]) / radii[2]) ** 2
    brain = r2 <= 1.0
    rng = np.random.RandomState(seed)
    data = np.zeros((4,) + shape, dtype=np.float32)
    for c in range(4):
        base = (80.0 + 40.0 * c) * (1.2 - 0.6 * r2) + 25.0 * np.sin(0.3 * z + c) * np.cos(0.2 * y) + 10.0 * rng.standard_normal(shape)
        data[c] = np.where(brain, np.maximum(base, 1.0), 0.0).astype(np.float32)
    q = [max(2, int(r // 4)) for r in radii]
    cav = tuple(slice(c - h, c + h) for c, h in zip(centre, q))
    cavity = np.zeros(shape, dtype=bool)
    cavity[cav] = True
    data[:, cavity] = 0.0
    pocket = np.zeros(shape, dtype=bool)
    pocket[centre[0] - 1:centre[0] + 2, centre[1] + q[1] + 1:centre[1] + q[1] + 4, centre[2] - 1:centre[2] + 2] = True
    data[2][pocket] = 0.0
    seg = np.zeros(shape, dtype=np.float32)
    off = r2 + 0.35 * (x - centre[2]) / radii[2]                      # nested lobes shifted along x: next to the cavity, not in it
    seg[brain & (off < 0.45)] = 2
    seg[brain & (off < 0.25)] = 1
    seg[brain & (off < 0.10)] = 3
    seg[cavity] = 0
    bb = bbox_of(brain)
    stray = (bb[0][0] + 1, bb[1][0] + 1, bb[2][0] + 1)                # a corner of the box: far outside the ellipsoid
    assert not brain[stray]
    seg[stray] = 2
    return data, seg[None], {"brain": brain, "cavity": cavity, "pocket": pocket, "stray": stray, "bbox": bb}


BRATS_SHAPE = (155, 240, 240)
BRATS_CENTRE, BRATS_RADII = (80, 125, 118), (59.5, 84.5, 69.5)        # the box [[21, 140], [41, 210], [49, 188]]


def brats_case():
    return brain_case(BRATS_SHAPE, BRATS_CENTRE, BRATS_RADII, seed=3)


def faces_case(shape=(9, 14, 21)):
    """a cross of three bars through the volume: the mask touches all six faces"""
    data = np.zeros((2,) + tuple(shape), dtype=np.float32)
    D, H, W = shape
    data[0, :, H // 2, W // 2] = 3.0
    data[1, D // 2, :, W // 2] = -2.0
    data[0, D // 2, H // 2, :] = 0.5
    return data


def single_voxel_case(shape=(6, 7, 11), at=(4, 2, 9)):
    data = np.zeros((3,) + tuple(shape), dtype=np.float32)
    data[(1,) + tuple(at)] = -7.0
    return data


def big_class_seg(shape=(1, 104, 110, 112)):
    """a seg for the class locations: label 1 in more than 10^6 voxels (the 1 % rule decides n), label 2 in a small block (the voxel
    count decides), label 3 in 20 000 voxels (the 10 000 cap decides), label 4 nowhere"""
    seg = np.zeros(shape, dtype=np.int16)
    seg[:, 2:100, 3:108, 4:110] = 1
    seg[:, 5:9, 6:11, 7:12] = 2
    seg[:, 50:60, 40:80, 30:80] = 3
    seg[:, 0, 0, :7] = -1
    return seg


# ---- the patch loader's stand-in dataset (tests/test_dataloading_cpu.py, tests/golden/make_golden_patch_boxes.py) -----------------
PATCH_SIZE = (16, 16, 16)
PATCH_BATCH = 6
PATCH_BATCHES = 12
# name -> (probabilistic oversampling, np.random.seed)
PATCH_SCENARIOS = {"last_third_seed1": (False, 1), "last_third_seed2": (False, 2), "probabilistic_seed3": (True, 3),
                   "probabilistic_seed4": (True, 4)}
PATCH_CLAMP_CASE, PATCH_ODD_CASE, PATCH_EVEN_CASE, PATCH_EMPTY_CASE = 1, 2, 3, 4


def patch_standin_dataset():
    """five small "preprocessed cases" as the loaders' dataset (a list of the reference's dicts, numpy arrays):
      0  larger than the patch, labels 1 - 3 in its middle;
      1  larger than the patch, its only foreground (label 2) in the planes z <= 3: a patch centred there is moved by the lower clamp;
      2  13 voxels along z (need_to_pad 3, odd);   3  12 voxels along y (need_to_pad 4, even);
      4  no foreground at all (every class list empty)."""
    shapes = [(30, 34, 32), (28, 40, 36), (13, 34, 32), (33, 12, 30), (20, 22, 24)]
    items = []
    for i, shp in enumerate(shapes):
        n = int(np.prod(shp))
        data = (np.arange(2 * n, dtype=np.float32).reshape((2,) + shp) % 977.0) * 0.25 + i + 1.0
        seg = np.zeros((1,) + shp, dtype=np.int8)
        seg[:, :, :2] = -1
        if i == 0:
            seg[:, 10:20, 12:22, 8:24], seg[:, 12:16, 14:18, 10:14], seg[:, 22:26, 5:9, 20:29] = 1, 3, 2
        elif i == 1:
            seg[:, 0:4, 10:30, 5:30] = 2
        elif i == 2:
            seg[:, 3:9, 20:30, 2:12] = 1
        elif i == 3:
            seg[:, 5:25, 3:9, 4:20], seg[:, 26:31, 2:6, 22:28] = 1, 3
        items.append({"data": data, "seg": seg, "properties": {"name": f"case_{i}", "class_locations": sample_locations(seg, (1, 2, 3))}})
    return items
