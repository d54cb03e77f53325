"""The reference of the separate-z resampling tests (TEST INFRASTRUCTURE): what the reference's `resample_data_or_seg(...,
do_separate_z=True, order_z=0)` computes (default_resampling.py:154-207), restated with numpy in float64 on tests/resample_ref.py.

Every 2-D slice across the axis is resized on its own - data by `zoom_ref` (skimage's resize = scipy's zoom, clipped to the SLICE's
range), a seg by `zoom_labels_ref` (batchgenerators' resize_segmentation) - and the slices are stacked back along the axis.  Then,
where the axis changes its length, `map_coordinates(stack, coordinates, order=0, mode='nearest')` with the in-plane coordinates at
the integers: output slice k is slice `slice_table(n_in, n_out)[k]` of the stack.  With equal lengths the table is the identity.

tests/test_resample_sepz_ref_cpu.py holds this to tests/golden/resample_sepz.npz (the reference's own function) and the table to
scipy's map_coordinates."""
import numpy as np

from tests import resample_ref as RR


# (axis, new shape) of the data cases: the axis shrinking, growing and unchanged at axis 0, then axes 1 and 2
DATA_TARGETS = [(0, (5, 21, 17)), (0, (13, 21, 17)), (0, (9, 21, 17)), (1, (12, 9, 25)), (2, (7, 10, 33))]
# (axis, new shape) of the fixture's seg cases on resample_ref.label_case(): in-plane factor 2 with 12 -> 7, factor 0.5 with 12 -> 20
SEG_TARGETS = [(0, (7, 28, 32)), (0, (20, 7, 8))]


def data_case(channels=2, shape=(9, 14, 20), seed=5):
    """unit noise, slice k of axis 0 scaled by 10^(k % 4): a clip to the channel's range instead of the slice's shows at once"""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** (np.arange(shape[0]) % 4)
    return (rng.standard_normal((channels,) + tuple(shape)) * scale[None, :, None, None]).astype(np.float32)


def slice_table(n_in, n_out):
    """the slice map_coordinates(order=0, mode='nearest') reads at (n_in / n_out) * (k + 0.5) - 0.5: the coordinate plus one half,
    floored, clipped to the axis; float64, every operation rounded on its own"""
    k = np.arange(n_out, dtype=np.float64)
    scale = float(n_in) / n_out
    return np.clip(np.floor(scale * (k + 0.5) - 0.5 + 0.5), 0, n_in - 1).astype(np.int64)


def _shape_2d(new_shape, axis):
    return tuple(int(n) for i, n in enumerate(new_shape) if i != axis)


def sepz_data_ref(x, new_shape, axis, order=3, clip=True):
    """one channel (n0, n1, n2) -> float64 new_shape: `zoom_ref` per 2-D slice, stacked, then the table"""
    x = np.asarray(x)
    new_shape = tuple(int(v) for v in new_shape)
    if tuple(x.shape) == new_shape:
        return x.astype(np.float64)
    s2 = _shape_2d(new_shape, axis)
    stack = np.stack([RR.zoom_ref(x.take(k, axis), s2, order, clip) for k in range(x.shape[axis])], axis)
    return stack.take(slice_table(x.shape[axis], new_shape[axis]), axis)


def sepz_data_ref_stacked(x, new_shape, axis, order=3, clip=True):
    """`sepz_data_ref` with `zoom_ref`'s steps run on all slices at once - the same elementwise arithmetic per slice, for inputs
    of a thousand slices (tests/test_resample_sepz_ref_cpu.py holds the two to each other)"""
    x64 = np.moveaxis(np.asarray(x, dtype=np.float64), axis, 0)
    new_shape = tuple(int(v) for v in new_shape)
    s2 = _shape_2d(new_shape, axis)
    c = x64
    if tuple(x64.shape[1:]) != s2:
        if order == 3:
            for ax in (1, 2):
                c = RR.prefilter_axis(c, ax)
        for ax in (1, 2):
            start, w = RR.coordinates(x64.shape[ax], s2[ax - 1], order)
            c = RR._gather_axis(c, ax, start, w, c.shape[ax])
        if clip:
            c = np.clip(c, x64.min(axis=(1, 2), keepdims=True), x64.max(axis=(1, 2), keepdims=True))
    return np.moveaxis(c[slice_table(x64.shape[0], new_shape[axis])], 0, axis)


def sepz_labels_ref(seg, new_shape, axis):
    """one seg (n0, n1, n2) -> (int64 new_shape, {label: weights of new_shape}, 0 where the label is absent from the source slice)"""
    seg = np.asarray(seg)
    new_shape = tuple(int(v) for v in new_shape)
    if tuple(seg.shape) == new_shape:
        return seg.astype(np.int64), {}
    s2 = _shape_2d(new_shape, axis)
    table = slice_table(seg.shape[axis], new_shape[axis])
    labels = [int(l) for l in np.unique(seg)]
    outs, weights = [], {l: [] for l in labels}
    for k in range(seg.shape[axis]):
        o, w = RR.zoom_labels_ref(seg.take(k, axis), s2)
        outs.append(o)
        for l in labels:
            weights[l].append(w.get(l, np.zeros(s2)) if w else (seg.take(k, axis) == l).astype(np.float64))
    out = np.stack(outs, axis).take(table, axis)
    return out, {l: np.stack(weights[l], axis).take(table, axis) for l in labels}

