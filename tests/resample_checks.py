"""Checks shared by tests/test_emu_resample.py (kernel sources on the CPU emulator) and tests/test_gpu_resample.py (the HIP library):
every function takes the loaded library and the device its tensors live on.  Reference: tests/resample_ref.py, the numpy float64
restatement that tests/test_resample_ref_cpu.py pins to scipy.ndimage.zoom.

Data are held to |got - want| <= 2^-23 |want| + 2^-40 max|x_c| (resample_ref.data_bound).  Labels are equal at every voxel where the
factors are dyadic (all weights are multiples of 1/64, the arithmetic is exact); elsewhere a voxel where some label's weight lies
within 1e-9 of 0.5 may take any value reached by deciding the near-tied labels either way, every other voxel is equal.  Every check
first asserts the conditions on its own input that keep it from passing vacuously."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import nifti
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP
from segmamba_amd import preprocess as P
from segmamba_amd import resample as RS
from tests import preprocess_ref as R
from tests import resample_ref as RR
from tests.preprocess_checks import _builtin_or_numpy, dev_t

NEW_EXPORTS = ("segm_zoom", "segm_zoom_workspace_bytes", "segm_zoom_labels")
NEAR_TIE_SHARE = 0.05


def _np(t):
    return t.cpu().numpy()


def data_within(got, x, new_shape, order, clip, name):
    """one channel against the restatement; -> the worst error over the bound"""
    want = RR.zoom_ref(x, new_shape, order, clip)
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.shape, want.shape)
    bound = RR.data_bound(want, float(np.abs(x).max()))
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"zoom {name}: order {order} {x.shape} -> {tuple(new_shape)} worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (name, worst)
    return worst


# ---- 1. cubic and linear zoom ---------------------------------------------------------------------------------------------------------
ZOOM_CASES = [  # channels, shape, new shape: odd and even sides, a side of 1, a side above 256, factors 2, 0.5, 1.5, 0.8 / 1.25
    (1, (11, 13, 9), (22, 20, 6)),
    (2, (7, 1, 12), (9, 1, 24)),
    (3, (5, 6, 300), (4, 9, 150)),
    (8, (10, 12, 8), (8, 15, 8)),
    (4, (9, 10, 17), (9, 10, 34)),
    (5, (12, 9, 16), (6, 9, 8)),
    (6, (8, 6, 10), (12, 9, 15)),
    (7, (1, 1, 1), (3, 2, 4)),
]


def check_zoom(lib, dev):
    rng = np.random.RandomState(21)
    worst = 0.0
    for C, shape, new_shape in ZOOM_CASES:
        x = (rng.standard_normal((C,) + shape) * (1.0 + 50.0 * rng.random_sample((C, 1, 1, 1))) + 3.0).astype(np.float32)
        t = dev_t(x, dev)
        for order in (3, 1):
            got = _np(ops_raw.zoom(lib, t, new_shape, order, False))
            for c in range(C):
                worst = max(worst, data_within(got[c], x[c], new_shape, order, False, f"{C} channels, channel {c}"))
    # strided channel views: the strides go to the kernel
    big = rng.standard_normal((6, 11, 19, 48)).astype(np.float32)
    for view in (lambda a: a[::2, :, 1:-1, 3:40], lambda a: a[1:5, 2:9], lambda a: a[:, :, :, 4:44], lambda a: a[5:6, :, ::2]):
        host, t = np.ascontiguousarray(view(big)), view(dev_t(big, dev))
        assert not t.is_contiguous() and t.stride(-1) == 1
        new_shape = (host.shape[1] * 2, int(round(host.shape[2] * 0.8)), int(round(host.shape[3] * 1.25)))
        for order in (3, 1):
            got = _np(ops_raw.zoom(lib, t, new_shape, order, True))
            for c in range(host.shape[0]):
                worst = max(worst, data_within(got[c], host[c], new_shape, order, True, f"view, channel {c}"))
    print(f"zoom: worst error / bound over all cases {worst:.3f}")
    return worst


# ---- 2. clip --------------------------------------------------------------------------------------------------------------------------
def check_clip(lib, dev):
    step = RR.step_edge()
    new_shape = (12, 14, 40)
    free = RR.zoom_ref(step, new_shape, 3, clip=False)
    assert free.min() < -1.0 and free.max() > 101.0, "the unclipped spline must leave the input's range"
    x = np.stack([step, np.full(step.shape, 7.25, np.float32), np.full(step.shape, -3.0e4, np.float32), step - 50.0])
    got = _np(ops_raw.zoom(lib, dev_t(x, dev), new_shape, 3, True))
    unclipped = _np(ops_raw.zoom(lib, dev_t(x, dev), new_shape, 3, False))
    assert unclipped[0].min() < -1.0 and unclipped[0].max() > 101.0, "without the clip the device overshoots too"
    for c in (0, 3):
        lo, hi = float(x[c].min()), float(x[c].max())
        assert got[c].min() == lo and got[c].max() == hi and ((got[c] >= lo) & (got[c] <= hi)).all()
        data_within(got[c], x[c], new_shape, 3, True, f"step edge, channel {c}")
    assert np.array_equal(got[1], np.full(new_shape, 7.25, np.float32)) and np.array_equal(got[2], np.full(new_shape, -3.0e4, np.float32))
    lin = _np(ops_raw.zoom(lib, dev_t(x, dev), new_shape, 1, True))
    assert lin[0].min() == 0.0 and lin[0].max() == 100.0 and np.array_equal(lin[1], np.full(new_shape, 7.25, np.float32))
    # through the public name: clipped, as the reference's resize is
    pub = _np(RS.resample_data_or_seg_to_shape(dev_t(x, dev), new_shape, (1, 1, 1), (1, 1, 0.5)))
    assert np.array_equal(pub, got)


# ---- 3. shortcuts and determinism -------------------------------------------------------------------------------------------------------
def check_shortcuts_and_determinism(lib, dev):
    rng = np.random.RandomState(4)
    x = rng.standard_normal((3, 9, 11, 14)).astype(np.float32)
    seg = RR.label_case()
    t, s = dev_t(x, dev), dev_t(seg[None], dev)
    same = RS.resample_data_or_seg_to_shape(t, (9, 11, 14), (1, 1, 1), (1, 1, 1))
    assert same is t or (same.dtype == t.dtype and torch.equal(same, t))
    same_seg = RS.resample_data_or_seg_to_shape(s, seg.shape, (1, 1, 1), (1, 1, 1), is_seg=True, order=1)
    assert same_seg.dtype == s.dtype and torch.equal(same_seg, s)
    assert RS.compute_new_shape((10, 20, 30), (1.0, 2.0, 0.5), (2.0, 1.0, 1.0)) == [5, 40, 15] == P.compute_new_shape((10, 20, 30), (1.0, 2.0, 0.5), (2.0, 1.0, 1.0))
    for order in (3, 1):
        for clip in (True, False):
            a, b = ops_raw.zoom(lib, t, (14, 9, 21), order, clip), ops_raw.zoom(lib, t, (14, 9, 21), order, clip)
            assert torch.equal(a, b), "two calls must be bit-equal"
    a, ca = ops_raw.zoom_labels(lib, s[0], (18, 21, 24))
    b, cb = ops_raw.zoom_labels(lib, s[0], (18, 21, 24))
    assert torch.equal(a, b) and torch.equal(ca, cb)
    a = RS.resample_data_or_seg(t, (14, 9, 21))
    assert torch.equal(a, RS.resample_data_or_seg(t, (14, 9, 21))) and a.dtype == torch.float32 and tuple(a.shape) == (3, 14, 9, 21)
    # more than eight channels go through in groups
    many = dev_t(np.concatenate([x, x, x, x]), dev)
    assert torch.equal(RS.resample_data_or_seg(many, (14, 9, 21))[9:12], a)


# ---- 4. labels, dyadic factors ------------------------------------------------------------------------------------------------------
DYADIC = [(2, 1, 1), (1, 1, 2), (2, 2, 1), (1, 2, 2), (2, 2, 2), (0.5, 1, 1), (1, 0.5, 1), (0.5, 0.5, 1), (1, 0.5, 0.5), (0.5, 0.5, 0.5),
          (2, 0.5, 1), (0.5, 2, 2)]


def check_labels_dyadic(lib, dev):
    for high in (300, 200):
        seg = RR.label_case(high=high)
        assert seg.dtype == np.int16 and set(np.unique(seg)) == {-1, 0, 1, 2, high}
        for factor in DYADIC:
            new_shape = tuple(int(n * f) for n, f in zip(seg.shape, factor))
            want, weights = RR.zoom_labels_ref(seg, new_shape)
            top = np.max(np.stack(list(weights.values())), axis=0)
            nobody = top < 0.5
            assert (want[nobody] == 0).all()
            if all(f != 1 for f in factor) and len(set(factor)) == 1:
                # only with all three axes at 2 or at 0.5 can three labels share a cell so that none reaches one half
                assert nobody.any(), ("a cell where no label reaches 0.5 is required", factor)
            for r in weights.values():
                assert np.array_equal(r * 64.0, np.round(r * 64.0)), "dyadic weights are multiples of 1/64"
            assert {-1, high} <= set(np.unique(want))
            got, counts = ops_raw.zoom_labels(lib, dev_t(seg, dev), new_shape)
            assert got.dtype == torch.int16 and np.array_equal(_np(got).astype(np.int64), want), (high, factor)
            assert counts.dtype == torch.int64 and np.array_equal(_np(counts), RR.label_counts(want)), (high, factor)
            pub = RS.resample_data_or_seg_to_shape(dev_t(seg[None], dev), new_shape, (1, 1, 1), (1, 1, 1), is_seg=True, order=1)
            assert tuple(pub.shape) == (1,) + new_shape and np.array_equal(_np(pub[0]).astype(np.int64), want)
    # float and int8 segs take the same path
    seg = RR.label_case(high=100)
    want = RR.zoom_labels_ref(seg, (24, 28, 32))[0]
    for dt in (np.float32, np.int8, np.int64):
        got = RS.resample_data_or_seg(dev_t(seg[None].astype(dt), dev), (24, 28, 32), is_seg=True, order=1)
        assert got.dtype == torch.int16 and np.array_equal(_np(got[0]).astype(np.int64), want)


# ---- 5. labels, other factors -------------------------------------------------------------------------------------------------------
def check_labels_near_ties(lib, dev):
    seg = RR.ellipsoid_labels()
    assert set(np.unique(seg)) == {-1, 0, 1, 2}
    for factor in [(1.5, 1.0, 1.0), (1.5, 1.5, 1.5), (0.8, 1.25, 1.0)]:
        new_shape = tuple(int(round(n * f)) for n, f in zip(seg.shape, factor))
        want, weights = RR.zoom_labels_ref(seg, new_shape)
        near = RR.near_ties(weights)
        share = float(near.mean())
        print(f"labels {factor}: near-ties {share:.4f} of the voxels")
        assert share <= NEAR_TIE_SHARE and not near.all()
        got, counts = ops_raw.zoom_labels(lib, dev_t(seg, dev), new_shape)
        g = _np(got).astype(np.int64)
        assert np.array_equal(g[~near], want[~near]), factor
        assert RR.reachable(g, weights).all(), factor
        assert np.array_equal(_np(counts), RR.label_counts(g))


# ---- 6. preprocess_case(resample=True) --------------------------------------------------------------------------------------------------
def resampled_oracle(data, seg, dev, new_spacing_case, all_labels=(1, 2, 3)):
    """the oracle's input is the device's own normalised crop and relabelled seg at unit spacing (covered by
    tests/preprocess_checks.py, bit-equal between calls); -> (crop data, crop seg, properties at unit spacing)"""
    props = {"spacing": (1.0, 1.0, 1.0)}
    d0, s0 = P.preprocess_case(dev_t(data, dev), None if seg is None else dev_t(seg, dev), props, all_labels=all_labels)
    return _np(d0), _np(s0), props


def check_preprocess_resample(lib, dev, data, seg, spacing, out_spacing, raw_shape_back=True):
    """`preprocess_case(resample=True)` against the restatement applied to the device's own crop"""
    d0, s0, p0 = resampled_oracle(data, seg, dev, None)
    crop_shape = list(d0.shape[1:])
    spacing_trans = [float(v) for v in spacing[::-1]]
    new_shape = RS.compute_new_shape(crop_shape, spacing_trans, list(out_spacing))
    assert new_shape != crop_shape
    for n_in, n_out in zip(crop_shape, new_shape):
        assert n_out in (n_in, 2 * n_in, n_in // 2) and (n_out != n_in // 2 or n_in % 2 == 0), "dyadic factors only"
    props = {"spacing": tuple(spacing), "raw_size": data.shape[1:], "name": "case"}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, out_spacing=out_spacing, resample=True)
    assert d.dtype == torch.float32 and tuple(d.shape) == (data.shape[0],) + tuple(new_shape)
    want_s, weights = RR.zoom_labels_ref(s0[0], new_shape)
    assert s.dtype == torch.int8 and tuple(s.shape) == (1,) + tuple(new_shape)
    assert set(np.unique(want_s)) >= {-1, 0, 1, 2, 3} and np.array_equal(_np(s)[0].astype(np.int64), want_s)
    g = _np(d)
    for c in range(data.shape[0]):
        data_within(g[c], d0[c], new_shape, 3, True, f"preprocess_case channel {c}")
    assert props["shape_after_cropping_before_resample"] == crop_shape == p0["shape_after_cropping_before_resample"]
    assert props["shape_after_resample"] == new_shape and props["bbox_used_for_cropping"] == p0["bbox_used_for_cropping"]
    assert props["shape_before_cropping"] == list(data.shape[1:])
    assert props["original_spacing_trans"] == spacing_trans and list(props["target_spacing_trans"]) == list(out_spacing)
    want_locs = R.sample_locations(want_s[None].astype(np.int8), (1, 2, 3))
    assert list(props["class_locations"].keys()) == [1, 2, 3]
    for k in (1, 2, 3):
        assert len(want_locs[k]) > 0 and np.array_equal(props["class_locations"][k], want_locs[k]), k
    raw_pickle = pickle.dumps(props)
    assert b"torch" not in raw_pickle and _builtin_or_numpy(props)
    d2, s2 = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": tuple(spacing)}, out_spacing=out_spacing, resample=True)
    assert torch.equal(d, d2) and torch.equal(s, s2), "two calls must be bit-equal"
    # back: one-hot logits of the resampled seg -> the raw shape
    onehot = torch.nn.functional.one_hot(s[0].long().clamp(min=0), 4).permute(3, 0, 1, 2).float().contiguous()
    back = PP.labels_from_logits(onehot, pickle.loads(raw_pickle))
    assert tuple(back.shape) == tuple(data.shape[1:]) and back.dtype == torch.uint8
    return want_s, new_shape


def check_preprocess_case_resampled(lib, dev, shape=(37, 46, 53)):
    data, seg, _ = R.brain_case(shape)
    check_preprocess_resample(lib, dev, data, seg, (2.0, 1.0, 1.0), (1, 1, 1))          # x 2 mm -> 1 mm
    zdata, zseg, zinfo = R.brain_case(shape)
    z0, z1 = zinfo["bbox"][0]
    if (z1 - z0) % 2:                                  # the factor 0.5 wants an even side: drop the brain's first plane
        zdata[:, z0], zseg[:, z0] = 0.0, 0.0
    box = R.crop_to_nonzero(zdata, zseg)[2]
    assert (box[0][1] - box[0][0]) % 2 == 0
    check_preprocess_resample(lib, dev, zdata, zseg, (1.0, 1.0, 1.0), (2, 1, 1))        # z 1 mm -> 2 mm
    # a seg with a label above 127 comes back as int16, its locations from the resampled seg
    seg200 = seg.copy()
    seg200[seg200 == 3] = 200
    props = {"spacing": (2.0, 1.0, 1.0)}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg200, dev), props, all_labels=(1, 2, 200), resample=True)
    assert s.dtype == torch.int16 and int(s.max()) == 200 and len(props["class_locations"][200]) > 0
    # an invalid seg value is still refused
    bad = seg.copy()
    bad[0, 10, 13, 15] = 1.5
    with pytest.raises(RuntimeError, match="no integer"):
        P.preprocess_case(dev_t(data, dev), dev_t(bad, dev), {"spacing": (2.0, 1.0, 1.0)}, resample=True)
    # resample=True at the target spacing is the plain path
    a = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)}, resample=True)
    b = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)})
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _write_cases(root, cases, names, spacing):
    for case, (data, seg, _) in cases.items():
        os.makedirs(os.path.join(root, "images", case))
        for c, name in enumerate(names):
            nifti.write_nifti(os.path.join(root, "images", case, name), data[c], spacing)
        nifti.write_nifti(os.path.join(root, "images", case, "seg.nii.gz"), seg[0].astype(np.uint8), spacing)


def _check_written(out, cases, dev):
    for case, (data, seg, _) in cases.items():
        d0, s0, p0 = resampled_oracle(data, seg, dev, None)
        crop = list(d0.shape[1:])
        new_shape = [crop[0], crop[1], 2 * crop[2]]
        z = np.load(os.path.join(out, case + ".npz"))
        with open(os.path.join(out, case + ".pkl"), "rb") as f:
            raw_pickle = f.read()
        props = pickle.loads(raw_pickle)
        assert b"torch" not in raw_pickle and _builtin_or_numpy(props)
        assert z["data"].dtype == np.float32 and z["data"].shape == (4,) + tuple(new_shape) and z["seg"].dtype == np.int8
        want_s = RR.zoom_labels_ref(s0[0], new_shape)[0]
        assert np.array_equal(z["seg"][0].astype(np.int64), want_s)
        for c in range(4):
            data_within(z["data"][c], d0[c], new_shape, 3, True, f"{case} channel {c}")
        assert props["shape_after_cropping_before_resample"] == crop and props["shape_after_resample"] == new_shape
        assert tuple(props["spacing"]) == (2.0, 1.0, 1.0) and props["name"] == case
        want_locs = R.sample_locations(want_s[None].astype(np.int8), (1, 2, 3))
        assert all(np.array_equal(props["class_locations"][k], want_locs[k]) for k in (1, 2, 3))
        onehot = torch.nn.functional.one_hot(dev_t(z["seg"][0], dev).long().clamp(min=0), 4).permute(3, 0, 1, 2).float().contiguous()
        assert tuple(PP.labels_from_logits(onehot, props).shape) == data.shape[1:]


def check_case_preprocessor_resampled(dev, tmp_path, monkeypatch):
    """`CasePreprocessor(resample=True)` and tools/preprocess_cases.py --resample on NIfTI files with 2 mm voxels along x"""
    raw, out, out2 = (os.path.join(str(tmp_path), n) for n in ("raw", "out", "out_tool"))
    names = ["t1.nii.gz", "t1ce.nii.gz", "t2.nii.gz", "flair.nii.gz"]
    cases = {"case_b": R.brain_case((21, 26, 30), seed=1), "case_a": R.brain_case((19, 28, 27), seed=2)}
    _write_cases(raw, cases, names, (2.0, 1.0, 1.0))
    with pytest.raises(NotImplementedError, match="resample=True"):
        P.CasePreprocessor(raw, "images", names, "seg.nii.gz").run((1, 1, 1), out, (1, 2, 3))
    written = P.CasePreprocessor(raw, "images", names, "seg.nii.gz", resample=True).run((1, 1, 1), out, (1, 2, 3))
    assert [os.path.basename(w) for w in written] == ["case_a.npz", "case_b.npz"]
    _check_written(out, cases, dev)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tools import preprocess_cases
    monkeypatch.setattr(sys, "argv", ["preprocess_cases.py", "--raw", os.path.join(raw, "images"), "--out", out2, "--data-files", *names,
                                      "--seg-file", "seg.nii.gz", "--resample"])
    preprocess_cases.main()
    _check_written(out2, cases, dev)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    rng = np.random.RandomState(9)
    x = dev_t(rng.standard_normal((2, 6, 7, 8)).astype(np.float32), dev)
    seg = dev_t(RR.label_case(), dev)
    for call in (lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (3.0, 1.0, 1.0), (1, 1, 1), force_separate_z=True),
                 lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (5.0, 1.0, 1.0), (1, 1, 1), force_separate_z=None),
                 lambda: RS.resample_data_or_seg(x, (6, 7, 16), do_separate_z=True, axis=[0]),
                 lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (1, 1, 1), (1, 1, 0.5), order=2),
                 lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (1, 1, 1), (1, 1, 0.5), order=0),
                 lambda: RS.resample_data_or_seg_to_shape(seg[None], (6, 7, 16), (1, 1, 1), (1, 1, 0.5), is_seg=True, order=3),
                 lambda: RS.resample_data_or_seg_to_shape(seg[None], (6, 7, 16), (1, 1, 1), (1, 1, 0.5), is_seg=True, order=0)):
        with pytest.raises(NotImplementedError):
            call()
    # isotropic spacings decide against the separate axis by themselves, as two equal low-resolution axes do
    assert tuple(RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (1, 1, 1), (1, 1, 0.5), force_separate_z=None).shape) == (2, 6, 7, 16)
    assert tuple(RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (5.0, 5.0, 1.0), (1, 1, 1), force_separate_z=None).shape) == (2, 6, 7, 16)
    for call in (lambda: ops_raw.zoom(lib, x, (2049, 2, 2)),                                      # a side above the limit
                 lambda: ops_raw.zoom(lib, x, (0, 2, 2)),
                 lambda: ops_raw.zoom(lib, x, (4, 4)),
                 lambda: ops_raw.zoom(lib, x, (6, 7, 16), order=2),                               # unsupported order
                 lambda: ops_raw.zoom(lib, x, (6, 7, 16), order=0),
                 lambda: ops_raw.zoom(lib, x[0], (6, 7, 16)),                                     # wrong rank
                 lambda: ops_raw.zoom(lib, x.double(), (6, 7, 16)),                               # wrong dtype
                 lambda: ops_raw.zoom(lib, x[:, :, :, ::2], (6, 7, 16)),                          # non-unit x stride
                 lambda: ops_raw.zoom(lib, x.repeat(5, 1, 1, 1)[:9], (6, 7, 16)),                 # more than 8 channels
                 lambda: ops_raw.zoom_labels(lib, seg, (2049, 2, 2)),
                 lambda: ops_raw.zoom_labels(lib, seg[None], (6, 7, 16)),
                 lambda: ops_raw.zoom_labels(lib, seg.float(), (6, 7, 16)),
                 lambda: ops_raw.zoom_labels(lib, seg.to(torch.int8), (6, 7, 16)),
                 lambda: ops_raw.zoom_labels(lib, seg[:, :, ::2], (6, 7, 16)),
                 lambda: RS.resample_data_or_seg(x[0], (6, 7, 16)),
                 lambda: RS.resample_data_or_seg(seg[None].float() + 0.5, (6, 7, 16), is_seg=True, order=1)):
        with pytest.raises(RuntimeError):
            call()
    # the C entries refuse what the wrappers would have refused, without touching the device
    a = L.ZoomArgs()
    assert lib.dll.segm_zoom(a) == -1 and lib.dll.segm_zoom(None) == -1
    out = torch.empty(2, 6, 7, 16, dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.dll.segm_zoom_workspace_bytes(2, 6, 7, 8, 3) // 8, dtype=torch.float64, device=x.device)

    def args(**kw):
        a = L.ZoomArgs()
        a.channels, a.depth, a.height, a.width, a.out_depth, a.out_height, a.out_width = 2, 6, 7, 8, 6, 7, 16
        a.order, a.clip = 3, 1
        a.stride_c, a.stride_z, a.stride_y = x.stride()[:3]
        a.data, a.out, a.workspace, a.workspace_bytes = x.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel() * 8
        a.stream = L.stream_handle(x)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.dll.segm_zoom(args()) == 0
    for kw in ({"out_width": 2049}, {"width": 2049}, {"out_depth": 0}, {"channels": 9}, {"order": 2}, {"order": 0}, {"clip": 2}, {"stride_y": 7}):
        assert lib.dll.segm_zoom(args(**kw)) == -2, kw
    assert lib.dll.segm_zoom(args(workspace_bytes=ws.numel() * 8 - 8)) == -6 and lib.dll.segm_zoom(args(workspace=None)) == -6
    assert lib.dll.segm_zoom(args(depth=2048, height=2048, width=1024, workspace_bytes=1 << 62)) == -2     # 2^32 voxels
    assert lib.dll.segm_zoom_workspace_bytes(2, 6, 7, 8, 3) == 256 + 2 * 10 * 11 * 12 * 8 and lib.dll.segm_zoom_workspace_bytes(2, 6, 7, 8, 1) == 256
    for bad in ((9, 6, 7, 8, 3), (2, 6, 7, 2049, 3), (2, 6, 7, 8, 2), (2, 0, 7, 8, 3)):
        assert lib.dll.segm_zoom_workspace_bytes(*bad) == 0, bad
    b = L.ZoomLabelsArgs()
    assert lib.dll.segm_zoom_labels(b) == -1
    b.seg, b.out = seg.data_ptr(), out.data_ptr()
    b.depth, b.height, b.width, b.out_depth, b.out_height, b.out_width = 12, 14, 16, 2, 2, 2049
    assert lib.dll.segm_zoom_labels(b) == -2


# ---- 8. exports -------------------------------------------------------------------------------------------------------------------------
def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
