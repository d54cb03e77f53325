"""Checks of the separate-z resampling branch, shared by tests/test_emu_resample_sepz.py (kernel sources on the CPU emulator) and
tests/test_gpu_resample_sepz.py (the HIP library): every function takes the loaded library and the device its tensors live on.
Reference: tests/resample_sepz_ref.py, the numpy float64 restatement that tests/test_resample_sepz_ref_cpu.py holds to the
reference's own function (tests/golden/resample_sepz.npz).

Data are held to |got - want| <= 2^-23 |want| + 2^-40 max|x_c| (resample_ref.data_bound, the project's bound for the 3-D zoom: the
rounding to fp32 plus fp64 noise through the prefilter; the branch has one prefilter pass fewer).  Labels are equal at every voxel
where the in-plane factors are dyadic (the weights are multiples of 1/16, the arithmetic is exact); elsewhere a voxel where some
label's weight lies within resample_ref.NEAR_TIE of 0.5 may take any value reached by deciding the near-tied labels either way, every
other voxel is equal, and such voxels are at most 5 % of a case."""
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd import preprocess as P
from segmamba_amd import resample as RS
from tests import preprocess_ref as R
from tests import resample_checks as K
from tests import resample_ref as RR
from tests import resample_sepz_ref as SR
from tests.preprocess_checks import _builtin_or_numpy, dev_t

NEW_EXPORTS = ("segm_zoom_slices", "segm_zoom_slices_workspace_bytes", "segm_zoom_labels_slices")
NEAR_TIE_SHARE = 0.05
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resample_sepz.npz")


def _np(t):
    return t.cpu().numpy()


def _sepz(t, new_shape, axis, order=3, is_seg=False):
    return RS.resample_data_or_seg(t, new_shape, is_seg, [axis], order, True, order_z=0, allow_separate_z=True)


def within(got, want, xmax, name):
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
    bound = RR.data_bound(want, xmax)
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"sepz {name}: worst error / bound {worst:.3f}")
    assert (err <= bound).all(), (name, worst)
    return worst


def data_within(got, x, new_shape, axis, order, name, ref=SR.sepz_data_ref):
    """(c, ...) against the restatement, channel by channel"""
    assert got.shape == (x.shape[0],) + tuple(new_shape), (name, got.shape)
    for c in range(x.shape[0]):
        within(got[c], ref(x[c], new_shape, axis, order), float(np.abs(x[c]).max()), f"{name} axis {axis} order {order} channel {c}")


# ---- 1. data ----------------------------------------------------------------------------------------------------------------------------
def check_data(lib, dev):
    x = SR.data_case()
    assert x.shape == (2, 9, 14, 20) and np.abs(x[:, 3]).max() > 100.0 * np.abs(x[:, 0]).max()
    t = dev_t(x, dev)
    golden = np.load(GOLDEN)
    fixture = {tuple(int(v) for v in row): golden[f"data_out_{i}"][0] for i, row in enumerate(golden["data_cases"])}
    assert np.array_equal(golden["data"][0], x[0])
    seen = 0
    for axis, shape in SR.DATA_TARGETS:
        for order in (3, 1):
            got = _np(_sepz(t, shape, axis, order))
            data_within(got, x, shape, axis, order, f"{x.shape[1:]} -> {shape}")
            fix = fixture.get((axis, *shape, order))
            if fix is not None:
                within(got[0], fix.astype(np.float64), float(np.abs(x[0]).max()), f"fixture axis {axis} -> {shape} order {order}")
                seen += 1
    assert seen == len(fixture) == 7
    rng = np.random.RandomState(31)
    for shape, new_shape, ref in (((1, 3, 5, 300), (4, 7, 450), SR.sepz_data_ref),            # a row past one x tile
                                  ((1, 3, 1, 1), (5, 2, 2), SR.sepz_data_ref),
                                  ((1, 2048, 2, 2), (1024, 3, 3), SR.sepz_data_ref_stacked)):  # the key array at its limit
        y = (rng.standard_normal(shape) * 30.0 + 5.0).astype(np.float32)
        for order in (3, 1):
            data_within(_np(_sepz(dev_t(y, dev), new_shape, 0, order)), y, new_shape, 0, order, f"{shape[1:]} -> {new_shape}", ref)


def check_channels_and_views(lib, dev):
    """8 channels in one launch, 9 split by the host, strided channel views: the strides go to the kernel"""
    x9 = SR.data_case(channels=9, seed=6)
    shape = (5, 21, 17)
    got9 = _np(_sepz(dev_t(x9, dev), shape, 0))
    data_within(got9, x9, shape, 0, 3, "9 channels")
    got8 = _np(ops_raw.zoom_slices(lib, dev_t(x9[:8], dev), shape, RS.slice_table(9, 5)))
    assert np.array_equal(got8, got9[:8])
    big = SR.data_case(channels=5, shape=(9, 16, 28), seed=7)
    for view in (lambda a: a[::2, :, 1:-1, 3:23], lambda a: a[1:4, 2:8], lambda a: a[4:5, :, ::2]):
        host, t = np.ascontiguousarray(view(big)), view(dev_t(big, dev))
        assert not t.is_contiguous() and t.stride(-1) == 1
        for axis in (0, 1):
            new_shape = [int(round(n * f)) for n, f in zip(host.shape[1:], (1.5, 0.75, 1.25))]
            new_shape[axis] = host.shape[1 + axis] + 3
            data_within(_np(_sepz(t, new_shape, axis)), host, new_shape, axis, 3, "view")


# ---- 2. the clip is per slice -----------------------------------------------------------------------------------------------------------
def check_per_slice_clip(lib, dev):
    S, H, W = 5, 12, 20
    x = np.zeros((1, S, H, W), dtype=np.float32)
    for k in range(S):                                # a step edge along x from 10^k to 2 * 10^k: ranges decades apart
        x[0, k, :, :W // 2], x[0, k, :, W // 2:] = 10.0 ** k, 2.0 * 10.0 ** k
    new_shape = (8, 12, 40)
    table = SR.slice_table(S, new_shape[0])
    assert set(table) == set(range(S))
    free = SR.sepz_data_ref(x[0], new_shape, 0, 3, clip=False)
    got = _np(_sepz(dev_t(x, dev), new_shape, 0))
    unclipped = _np(ops_raw.zoom_slices(lib, dev_t(x, dev), new_shape, RS.slice_table(S, new_shape[0]), 3, False))
    for k, s in enumerate(table):
        lo, hi = float(x[0, s].min()), float(x[0, s].max())
        assert free[k].min() < lo - 0.01 * lo and free[k].max() > hi + 0.01 * lo, "the unclipped spline must leave the slice's range"
        assert unclipped[0, k].min() < lo - 0.01 * lo and unclipped[0, k].max() > hi + 0.01 * lo, "without the clip the device overshoots too"
        assert got[0, k].min() == lo and got[0, k].max() == hi, (k, s)      # a channel-wide clip would let the overshoot through
    data_within(got, x, new_shape, 0, 3, "step edges")
    lin = _np(_sepz(dev_t(x, dev), new_shape, 0, 1))
    data_within(lin, x, new_shape, 0, 1, "step edges")


# ---- 3. slices do not see each other; determinism ----------------------------------------------------------------------------------------
def check_slice_independence(lib, dev):
    x = SR.data_case()
    t = dev_t(x, dev)
    for order in (3, 1):
        for shape in ((13, 21, 17), (5, 21, 17)):
            got = _sepz(t, shape, 0, order)
            assert torch.equal(got, _sepz(t, shape, 0, order)), "two calls must be bit-equal"
            for k, s in enumerate(SR.slice_table(9, shape[0])):
                alone = _sepz(t[:, s:s + 1], (1,) + shape[1:], 0, order)
                assert torch.equal(alone[:, 0], got[:, k]), (order, shape, k)
    # an unchanged in-plane shape copies the slices; equal shapes return the input
    got = _sepz(t, (13, 14, 20), 0)
    assert torch.equal(got, t[:, torch.from_numpy(SR.slice_table(9, 13)).to(t.device)])
    same = _sepz(t, (9, 14, 20), 0)
    assert same is t or (same.dtype == t.dtype and torch.equal(same, t))
    # axes 1 and 2 are axis 0 of the transposed volume, bit for bit
    a1 = _sepz(t, (12, 13, 25), 1)
    assert a1.is_contiguous() and torch.equal(a1, _sepz(t.permute(0, 2, 1, 3).contiguous(), (13, 12, 25), 0).permute(0, 2, 1, 3))
    a2 = _sepz(t, (7, 10, 33), 2)
    assert a2.is_contiguous() and torch.equal(a2, _sepz(t.permute(0, 3, 1, 2).contiguous(), (33, 7, 10), 0).permute(0, 2, 3, 1))
    # a table with entries outside the volume is clamped, not followed
    wild = ops_raw.zoom_slices(lib, t, (4, 21, 17), [-7, 0, 8, 1 << 30])
    tame = ops_raw.zoom_slices(lib, t, (4, 21, 17), [0, 0, 8, 8])
    assert torch.equal(wild, tame)


# ---- 4. labels --------------------------------------------------------------------------------------------------------------------------
def _label_cases():
    ell = RR.ellipsoid_labels()[6:18]
    assert set(np.unique(ell)) == {-1, 0, 1, 2} and ell.shape[0] == 12
    seg = RR.label_case()
    seg[10, 12:14, 14:16] = [[1, 2], [300, 0]]        # four labels share one 2 x 2 cell of a slice: at a factor of 0.5 none reaches 0.5
    return {"label_case": seg, "ellipsoid": np.ascontiguousarray(ell)}


def check_labels_dyadic(lib, dev):
    for name, seg in _label_cases().items():
        assert seg.dtype == np.int16 and seg.shape[0] == 12
        for factor in (2.0, 0.5):
            for n_out in (7, 20):
                new_shape = (n_out, int(seg.shape[1] * factor), int(seg.shape[2] * factor))
                want, weights = SR.sepz_labels_ref(seg, new_shape, 0)
                for r in weights.values():
                    assert np.array_equal(r * 16.0, np.round(r * 16.0)), "dyadic weights are multiples of 1/16"
                if name == "label_case":
                    assert {-1, 300} <= set(np.unique(want))
                    top = np.max(np.stack(list(weights.values())), axis=0)
                    assert (want[top < 0.5] == 0).all()
                    assert factor != 0.5 or n_out != 20 or (top < 0.5).any(), "a cell where no label reaches 0.5 is required"
                got, counts = ops_raw.zoom_labels_slices(lib, dev_t(seg, dev), new_shape, RS.slice_table(12, n_out))
                assert got.dtype == torch.int16 and np.array_equal(_np(got).astype(np.int64), want), (name, new_shape)
                assert counts.dtype == torch.int64 and np.array_equal(_np(counts), RR.label_counts(want)), (name, new_shape)
                again, none = ops_raw.zoom_labels_slices(lib, dev_t(seg, dev), new_shape, RS.slice_table(12, n_out), want_counts=False)
                assert none is None and torch.equal(again, got)
    # the public name, the other two axes, float and int8 segs; the fixture
    seg = RR.label_case(high=100)
    for axis, new_shape in ((1, (24, 9, 32)), (2, (6, 7, 20)), (0, (7, 28, 32))):
        want = SR.sepz_labels_ref(seg, new_shape, axis)[0]
        for dt in (np.int16, np.float32, np.int8):
            got = _sepz(dev_t(seg[None].astype(dt), dev), new_shape, axis, 1, is_seg=True)
            assert got.dtype == torch.int16 and got.is_contiguous() and np.array_equal(_np(got[0]).astype(np.int64), want), (axis, dt)
    golden = np.load(GOLDEN)
    for i, row in enumerate(golden["seg_cases"]):
        got = _sepz(dev_t(golden["seg"], dev), tuple(int(v) for v in row[1:4]), int(row[0]), 1, is_seg=True)
        assert np.array_equal(_np(got), golden[f"seg_out_{i}"])


def check_labels_past_one_grid(lib, dev):
    """more output voxels than 2048 workgroups of 256 hold: the label kernel's workgroups walk the output a second time"""
    seg = RR.label_case()[4:7, :, :]
    new_shape = (150, 56, 64)                         # in-plane factor 4: every weight is exact
    assert new_shape[0] * new_shape[1] * new_shape[2] > 2048 * 256 and set(np.unique(seg)) >= {-1, 0, 1, 2, 300}
    table = [(7 * k) % 3 for k in range(new_shape[0])]
    per_slice = np.stack([RR.zoom_labels_ref(s, new_shape[1:])[0] for s in seg])
    want = per_slice[table]
    got, counts = ops_raw.zoom_labels_slices(lib, dev_t(np.ascontiguousarray(seg), dev), new_shape, table)
    assert np.array_equal(_np(got).astype(np.int64), want) and np.array_equal(_np(counts), RR.label_counts(want))


def check_labels_near_ties(lib, dev):
    for name, seg in _label_cases().items():
        for plane in ((21, 24), (17, 13), (35, 45)):
            new_shape = (7,) + plane
            want, weights = SR.sepz_labels_ref(seg, new_shape, 0)
            near = RR.near_ties(weights)
            share = float(near.mean())
            print(f"labels {name} {seg.shape[1:]} -> {plane}: near-ties {share:.4f} of the voxels")
            assert share <= NEAR_TIE_SHARE and not near.all()
            got, counts = ops_raw.zoom_labels_slices(lib, dev_t(seg, dev), new_shape, RS.slice_table(12, 7))
            g = _np(got).astype(np.int64)
            assert np.array_equal(g[~near], want[~near]), (name, plane)
            assert RR.reachable(g, weights).all(), (name, plane)
            assert np.array_equal(_np(counts), RR.label_counts(g))


# ---- 5. preprocess_case -----------------------------------------------------------------------------------------------------------------
SPACING = (1.0, 1.0, 5.0)                 # SimpleITK's (x, y, z): 5 mm slices
OUT_SPACING = (2.5, 1.5, 1.5)


def _thick_case(shape=(18, 32, 36), seed=0):
    data, seg, _ = R.brain_case(shape, seed=seed)
    return data, seg


def check_preprocess_case_separate_z(lib, dev):
    data, seg = _thick_case()
    d0, s0, p0 = K.resampled_oracle(data, seg, dev, None)
    crop = list(d0.shape[1:])
    assert 10 <= crop[0] <= 12 and 22 <= crop[1] <= 27 and 27 <= crop[2] <= 31, crop
    new_shape = RS.compute_new_shape(crop, [5.0, 1.0, 1.0], list(OUT_SPACING))
    assert new_shape[0] == 2 * crop[0] and new_shape[1] < crop[1] and new_shape[2] < crop[2]
    props = {"spacing": SPACING, "raw_size": data.shape[1:], "name": "case"}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, out_spacing=OUT_SPACING, resample=True, force_separate_z=None)
    assert d.dtype == torch.float32 and tuple(d.shape) == (4,) + tuple(new_shape)
    assert s.dtype == torch.int8 and tuple(s.shape) == (1,) + tuple(new_shape)
    data_within(_np(d), d0, new_shape, 0, 3, "preprocess_case")
    want_s, weights = SR.sepz_labels_ref(s0[0], new_shape, 0)
    near = RR.near_ties(weights)
    g = _np(s)[0].astype(np.int64)
    assert set(np.unique(want_s)) >= {-1, 0, 1, 2, 3} and near.mean() <= NEAR_TIE_SHARE
    assert np.array_equal(g[~near], want_s[~near]) and RR.reachable(g, weights).all()
    assert props["shape_after_cropping_before_resample"] == crop == p0["shape_after_cropping_before_resample"]
    assert props["shape_after_resample"] == new_shape and props["bbox_used_for_cropping"] == p0["bbox_used_for_cropping"]
    assert props["shape_before_cropping"] == list(data.shape[1:])
    assert props["original_spacing_trans"] == [5.0, 1.0, 1.0] and list(props["target_spacing_trans"]) == list(OUT_SPACING)
    want_locs = R.sample_locations(g[None].astype(np.int8), (1, 2, 3))
    assert list(props["class_locations"].keys()) == [1, 2, 3]
    for k in (1, 2, 3):
        assert len(want_locs[k]) > 0 and np.array_equal(props["class_locations"][k], want_locs[k]), k
    raw_pickle = pickle.dumps(props)
    assert b"torch" not in raw_pickle and _builtin_or_numpy(props)
    d2, s2 = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": SPACING}, out_spacing=OUT_SPACING, resample=True,
                               force_separate_z=True)
    assert torch.equal(d, d2) and torch.equal(s, s2), "forced and decided take the same route; two calls are bit-equal"
    # force_separate_z=False is today's route, bit for bit - and another function of the case
    today = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": SPACING}, out_spacing=OUT_SPACING, resample=True)
    off = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": SPACING}, out_spacing=OUT_SPACING, resample=True,
                            force_separate_z=False)
    assert torch.equal(today[0], off[0]) and torch.equal(today[1], off[1])
    assert tuple(today[0].shape) == tuple(d.shape) and float((today[0] - d).abs().max()) > 0.05
    # auto on an isotropic case decides against: the 3-D zoom
    iso = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (2.0, 2.0, 2.0)}, out_spacing=(1, 2, 2), resample=True)
    auto = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (2.0, 2.0, 2.0)}, out_spacing=(1, 2, 2), resample=True,
                             force_separate_z=None)
    assert torch.equal(iso[0], auto[0]) and torch.equal(iso[1], auto[1])


def check_case_preprocessor_separate_z(dev, tmp_path, monkeypatch):
    """`CasePreprocessor(resample=True, force_separate_z=None)` and tools/preprocess_cases.py --resample --separate-z auto on two NIfTI
    cases with 5 mm slices: what `preprocess_case`, checked above, gives for the same arrays"""
    raw, out, out2, out3 = (os.path.join(str(tmp_path), n) for n in ("raw", "out", "out_tool", "out_never"))
    names = ["t1.nii.gz", "t1ce.nii.gz", "t2.nii.gz", "flair.nii.gz"]
    cases = {"case_b": R.brain_case((18, 32, 36), seed=1), "case_a": R.brain_case((17, 30, 33), seed=2)}
    K._write_cases(raw, cases, names, SPACING)
    written = P.CasePreprocessor(raw, "images", names, "seg.nii.gz", resample=True, force_separate_z=None).run(OUT_SPACING, out, (1, 2, 3))
    assert [os.path.basename(w) for w in written] == ["case_a.npz", "case_b.npz"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from tools import preprocess_cases
    common = ["preprocess_cases.py", "--raw", os.path.join(raw, "images"), "--data-files", *names, "--seg-file", "seg.nii.gz", "--resample",
              "--spacing", *[str(v) for v in OUT_SPACING]]
    monkeypatch.setattr(sys, "argv", common + ["--out", out2, "--separate-z", "auto"])
    preprocess_cases.main()
    monkeypatch.setattr(sys, "argv", common + ["--out", out3])
    preprocess_cases.main()
    for case, (data, seg, _) in cases.items():
        props = {"spacing": SPACING}
        d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, out_spacing=OUT_SPACING, resample=True, force_separate_z=None)
        plain = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": SPACING}, out_spacing=OUT_SPACING, resample=True)
        assert float((plain[0] - d).abs().max()) > 0.05
        for folder, want in ((out, (d, s)), (out2, (d, s)), (out3, plain)):
            z = np.load(os.path.join(folder, case + ".npz"))
            assert np.array_equal(z["data"], _np(want[0])) and np.array_equal(z["seg"], _np(want[1])), (folder, case)
            with open(os.path.join(folder, case + ".pkl"), "rb") as f:
                got_props = pickle.load(f)
            assert got_props["shape_after_resample"] == props["shape_after_resample"] and got_props["name"] == case
        with open(os.path.join(out, case + ".pkl"), "rb") as f:
            got_props = pickle.load(f)
        assert all(np.array_equal(got_props["class_locations"][k], props["class_locations"][k]) for k in (1, 2, 3))


# ---- 6. refusals and exports ------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    rng = np.random.RandomState(9)
    x = dev_t(rng.standard_normal((2, 6, 7, 8)).astype(np.float32), dev)
    seg = dev_t(RR.label_case(), dev)
    # without the keyword the branch is refused as before, and the message names the keyword
    for call in (lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (3.0, 1.0, 1.0), (1, 1, 1), force_separate_z=True),
                 lambda: RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (5.0, 1.0, 1.0), (1, 1, 1), force_separate_z=None),
                 lambda: RS.resample_data_or_seg(x, (6, 7, 16), do_separate_z=True, axis=[0]),
                 lambda: RS.resample_data_or_seg_to_spacing(x, (5.0, 1.0, 1.0), (5.0, 1.0, 0.5), force_separate_z=None)):
        with pytest.raises(NotImplementedError, match="allow_separate_z"):
            call()
    for call in (lambda: RS.resample_data_or_seg(x, (6, 7, 16), axis=[0], do_separate_z=True, order_z=1, allow_separate_z=True),
                 lambda: RS.resample_data_or_seg(x, (6, 7, 16), axis=[0], order=2, do_separate_z=True, allow_separate_z=True),
                 lambda: RS.resample_data_or_seg(seg[None], (6, 7, 16), True, [0], 3, True, allow_separate_z=True)):
        with pytest.raises(NotImplementedError):
            call()
    for call in (lambda: RS.resample_data_or_seg(x, (6, 7, 16), axis=[0, 1], do_separate_z=True, allow_separate_z=True),
                 lambda: RS.resample_data_or_seg(x, (6, 7, 16), axis=None, do_separate_z=True, allow_separate_z=True),
                 lambda: ops_raw.zoom_slices(lib, x, (2049, 2, 2), [0] * 2049),
                 lambda: ops_raw.zoom_slices(lib, x, (0, 2, 2), []),
                 lambda: ops_raw.zoom_slices(lib, x, (3, 7, 16), [0, 1]),                         # a table of the wrong length
                 lambda: ops_raw.zoom_slices(lib, x, (2, 7, 16), [0.0, 1.0]),                     # no integers
                 lambda: ops_raw.zoom_slices(lib, x, (2, 7, 16), [0, 1], order=2),
                 lambda: ops_raw.zoom_slices(lib, x[0], (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_slices(lib, x.double(), (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_slices(lib, x[:, :, :, ::2], (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_slices(lib, x.repeat(5, 1, 1, 1)[:9], (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_labels_slices(lib, seg, (2, 2049, 2), [0, 1]),
                 lambda: ops_raw.zoom_labels_slices(lib, seg[None], (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_labels_slices(lib, seg.float(), (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_labels_slices(lib, seg[:, :, ::2], (2, 7, 16), [0, 1]),
                 lambda: ops_raw.zoom_labels_slices(lib, seg, (2, 7, 16), [0])):
        with pytest.raises(RuntimeError):
            call()
    # the decision rule with the keyword: forced, by the current spacing, by the target's; two coarse axes decide against
    assert tuple(RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (5.0, 1.0, 1.0), (1, 1, 1), force_separate_z=None,
                                                  allow_separate_z=True).shape) == (2, 6, 7, 16)
    by_target = RS.resample_data_or_seg_to_shape(x, (3, 7, 16), (1.0, 1.0, 1.0), (4.0, 1.0, 1.0), force_separate_z=None, allow_separate_z=True)
    assert torch.equal(by_target, RS.resample_data_or_seg(x, (3, 7, 16), axis=[0], do_separate_z=True, allow_separate_z=True))
    two = RS.resample_data_or_seg_to_shape(x, (6, 7, 16), (5.0, 5.0, 1.0), (1, 1, 1), force_separate_z=None, allow_separate_z=True)
    assert torch.equal(two, RS.resample_data_or_seg(x, (6, 7, 16)))
    to_spacing = RS.resample_data_or_seg_to_spacing(x, (5.0, 1.0, 1.0), (2.5, 1.0, 0.5), force_separate_z=None, allow_separate_z=True)
    assert tuple(to_spacing.shape) == (2, 12, 7, 16)
    assert torch.equal(to_spacing, RS.resample_data_or_seg(x, (12, 7, 16), axis=[0], do_separate_z=True, allow_separate_z=True))
    # the C entries refuse what the wrappers would have refused, without touching the device
    assert lib.dll.segm_zoom_slices(L.ZoomSlicesArgs()) == -1 and lib.dll.segm_zoom_slices(None) == -1
    out = torch.empty(2, 5, 7, 16, dtype=torch.float32, device=x.device)
    src = torch.zeros(5, dtype=torch.int32, device=x.device)
    nbytes = lib.dll.segm_zoom_slices_workspace_bytes(2, 6, 7, 8, 7, 16, 3)
    assert nbytes == 256 + 2 * 6 * 11 * 12 * 8
    assert lib.dll.segm_zoom_slices_workspace_bytes(2, 6, 7, 8, 7, 16, 1) == 256 == lib.dll.segm_zoom_slices_workspace_bytes(2, 6, 7, 8, 7, 8, 3)
    assert lib.dll.segm_zoom_slices_workspace_bytes(8, 2048, 2, 2, 3, 3, 1) == 2 * 8 * 2048 * 4
    for bad in ((9, 6, 7, 8, 7, 16, 3), (2, 6, 7, 2049, 7, 16, 3), (2, 6, 7, 8, 7, 16, 2), (2, 0, 7, 8, 7, 16, 3), (2, 6, 7, 8, 0, 16, 3),
                (2, 6, 7, 8, 7, 2049, 3)):
        assert lib.dll.segm_zoom_slices_workspace_bytes(*bad) == 0, bad
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)

    def args(**kw):
        a = L.ZoomSlicesArgs()
        a.channels, a.slices, a.height, a.width, a.out_slices, a.out_height, a.out_width = 2, 6, 7, 8, 5, 7, 16
        a.order, a.clip = 3, 1
        a.stride_c, a.stride_s, a.stride_y = x.stride()[:3]
        a.data, a.source, a.out, a.workspace, a.workspace_bytes = x.data_ptr(), src.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes
        a.stream = L.stream_handle(x)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert lib.dll.segm_zoom_slices(args()) == 0
    for kw in ({"out_width": 2049}, {"width": 2049}, {"out_slices": 0}, {"slices": 0}, {"height": 0}, {"channels": 9}, {"order": 2},
               {"order": 0}, {"clip": 2}, {"stride_y": 7}):
        assert lib.dll.segm_zoom_slices(args(**kw)) == -2, kw
    for kw in ({"data": None}, {"out": None}, {"source": None}):
        assert lib.dll.segm_zoom_slices(args(**kw)) == -1, kw
    assert lib.dll.segm_zoom_slices(args(workspace_bytes=nbytes - 8)) == -6 and lib.dll.segm_zoom_slices(args(workspace=None)) == -6
    assert lib.dll.segm_zoom_slices(args(slices=2048, height=2048, width=1024, workspace_bytes=1 << 62)) == -2     # 2^32 voxels
    b = L.ZoomLabelsSlicesArgs()
    assert lib.dll.segm_zoom_labels_slices(b) == -1 and lib.dll.segm_zoom_labels_slices(None) == -1
    b.seg, b.out = seg.data_ptr(), out.data_ptr()
    assert lib.dll.segm_zoom_labels_slices(b) == -1                                                # no table
    b.source = src.data_ptr()
    for shape in ((12, 14, 16, 2, 2, 2049), (12, 14, 16, 0, 2, 2), (12, 0, 16, 2, 2, 2), (2049, 14, 16, 2, 2, 2)):
        b.slices, b.height, b.width, b.out_slices, b.out_height, b.out_width = shape
        assert lib.dll.segm_zoom_labels_slices(b) == -2, shape


def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert "segm_zoom_slices_args" in hdr and "segm_zoom_labels_slices_args" in hdr
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
