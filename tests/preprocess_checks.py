"""Checks shared by tests/test_emu_preprocess.py (kernel sources on the CPU emulator) and tests/test_gpu_preprocess.py (the HIP
library): every function takes the loaded library and the device its tensors live on.  References: tests/preprocess_ref.py.
Mask, box, crop, seg and class locations are exact (array_equal); the normalisation is held to 4 * 2^-24 * (|x| + |mean|) / std
against the float64 restatement.  Every check first asserts the conditions on its own input that keep it from passing vacuously."""
import os
import pickle

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import nifti
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP
from segmamba_amd import preprocess as P
from tests import preprocess_ref as R

NEW_EXPORTS = ("segm_nonzero_mask_bbox", "segm_crop_stats", "segm_crop_stats_workspace_bytes", "segm_crop_normalize")


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


def _box_list(bbox6):
    z0, y0, x0, z1, y1, x1 = (int(v) for v in bbox6.tolist())
    return [[z0, z1], [y0, y1], [x0, x1]]


# ---- 1. mask, box, crop ---------------------------------------------------------------------------------------------------------------
def check_brain_case_conditions(data, seg, info, filled):
    """the conditions the issue states on the synthetic case; -> the number of voxels that filling adds"""
    raw = R.nonzero_mask(data)
    added = int(filled.sum()) - int(raw.sum())
    assert added >= 1 and np.array_equal(filled & ~raw, info["cavity"]), "filling must add the cavity and nothing else"
    assert raw[info["pocket"]].all() and (data[2][info["pocket"]] == 0).all(), "the one-channel pocket must add nothing"
    bb = R.bbox_of(filled)
    assert all(b[0] > 0 and b[1] < n for b, n in zip(bb, data.shape[1:])), "the box must be strictly inside the volume"
    assert bb == R.bbox_of(raw), "the box of the mask is the box of the filled mask"
    sl = tuple(slice(a, b) for a, b in bb)
    assert int(((seg[0][sl] == 0) & ~filled[sl]).sum()) >= 1, "at least one voxel must get -1"
    stray = info["stray"]
    assert seg[0][stray] == 2 and not filled[stray] and all(b[0] <= s < b[1] for b, s in zip(bb, stray))
    assert set(np.unique(seg[0][info["brain"]])) >= {1.0, 2.0, 3.0}
    return added


def check_mask_box_crop(lib, dev, data, seg=None, fill_fn=R.fill):
    """raw kernels and `crop_to_nonzero` against the restatement, exactly"""
    want_raw = R.nonzero_mask(data)
    want_d, want_s, want_bb, want_filled = R.crop_to_nonzero(data, seg, fill_fn=fill_fn)
    t = data if isinstance(data, torch.Tensor) else dev_t(data, dev)
    mask, bbox = ops_raw.nonzero_mask_bbox(lib, t)
    assert mask.dtype == torch.uint8 and np.array_equal(_np(mask), want_raw.astype(np.uint8))
    assert bbox.dtype == torch.int32 and _box_list(bbox) == want_bb
    m2, b2 = ops_raw.nonzero_mask_bbox(lib, t)
    assert torch.equal(mask, m2) and torch.equal(bbox, b2)
    filled = P.create_nonzero_mask(t)
    assert filled.dtype == torch.uint8 and np.array_equal(_np(filled), want_filled.astype(np.uint8))
    got_d, got_s, got_bb = P.crop_to_nonzero(t, None if seg is None else dev_t(seg, dev))
    assert got_bb == want_bb
    assert got_d.dtype == torch.float32 and got_d.is_contiguous()
    assert np.array_equal(_np(got_d).view(np.uint32), np.ascontiguousarray(want_d).view(np.uint32)), "the crop must be bit-equal"
    assert tuple(got_s.shape) == want_s.shape and got_s.dtype == (torch.int8 if seg is None else torch.int16)
    assert np.array_equal(_np(got_s).astype(np.int64), want_s.astype(np.int64))
    return want_d, want_s, want_bb, want_filled


def check_brain_crop(lib, dev, shape=(37, 46, 53)):
    data, seg, info = R.brain_case(shape)
    filled = R.fill(R.nonzero_mask(data))
    added = check_brain_case_conditions(data, seg, info, filled)
    print("brain case", shape, "filling adds", added, "box", R.bbox_of(filled))
    _, want_s, bb, _ = check_mask_box_crop(lib, dev, data, seg)
    stray = tuple(s - b[0] for s, b in zip(info["stray"], bb))
    assert want_s[0][stray] == 2 and (want_s == -1).sum() >= 1
    # seg as uint8 and as int16 give the same
    for dt in (np.uint8, np.int16):
        got = P.crop_to_nonzero(dev_t(data, dev), dev_t(seg.astype(dt), dev))[1]
        assert np.array_equal(_np(got).astype(np.int64), want_s.astype(np.int64))


def check_shapes_and_strides(lib, dev):
    """sides that are no multiples of 4, 16 or 64; the 16-byte path (aligned, W % 4 == 0) and the scalar one; strided channel views"""
    rng = np.random.RandomState(5)
    for shape in [(13, 22, 37), (9, 17, 70), (10, 12, 40), (5, 6, 11), (3, 5, 129)]:
        data = rng.standard_normal((3,) + shape).astype(np.float32)
        data[rng.random_sample(data.shape) < 0.6] = 0.0
        data[:, :2], data[:, :, -3:], data[:, :, :, :5] = 0.0, 0.0, 0.0
        data[:, :, :, -2:] = 0.0
        seg = ((rng.random_sample((1,) + shape) < 0.3) * rng.randint(1, 4, size=(1,) + shape)).astype(np.float32)
        assert R.nonzero_mask(data).any()
        bb = check_mask_box_crop(lib, dev, data, seg)[2]
        assert bb[0][0] == 2 and bb[2][0] >= 5 and bb[2][1] <= shape[2] - 2
    big = rng.standard_normal((6, 11, 19, 48)).astype(np.float32)
    big[rng.random_sample(big.shape) < 0.7] = 0.0
    big[:, :3], big[:, :, :, :9] = 0.0, 0.0
    for view in (lambda a: a[::2, :, 1:-1, 3:40], lambda a: a[1:5, 2:9], lambda a: a[:, :, :, 4:44], lambda a: a[5:6, :, ::2]):
        host = view(big)
        t = view(dev_t(big, dev))
        assert not t.is_contiguous() and t.stride(-1) == 1 and R.nonzero_mask(host).any()
        check_mask_box_crop(lib, dev, host, None)                             # the numpy view: uploaded contiguous
        want = R.crop_to_nonzero(np.ascontiguousarray(host), None)
        mask, bbox = ops_raw.nonzero_mask_bbox(lib, t)                       # the device view itself: strides go to the kernel
        assert np.array_equal(_np(mask), R.nonzero_mask(host).astype(np.uint8)) and _box_list(bbox) == want[2]
        got = P.crop_to_nonzero(t)
        assert np.array_equal(_np(got[0]), want[0]) and np.array_equal(_np(got[1]), want[1]) and got[2] == want[2]
        z = P.zscore_normalize(t)
        for c in range(host.shape[0]):
            ref, mean, std = R.zscore64(host[c])
            assert (np.abs(_np(z[c]).astype(np.float64) - ref) <= R.zscore_bound(host[c], mean, std)).all()


def check_further_cases(lib, dev):
    # a mask that touches each face
    data = R.faces_case()
    bb = check_mask_box_crop(lib, dev, data)[2]
    assert bb == [[0, data.shape[1]], [0, data.shape[2]], [0, data.shape[3]]]
    # a single non-zero voxel
    data = R.single_voxel_case()
    want = check_mask_box_crop(lib, dev, data)
    assert want[2] == [[4, 5], [2, 3], [9, 10]] and want[0].shape == (3, 1, 1, 1)
    # a NaN voxel counts as non-zero (as `!=` has it), -0.0 does not
    data = np.zeros((2, 6, 9, 13), dtype=np.float32)
    data[1, 2, 3, 4] = np.nan
    data[0, 4, 7, 11] = -0.0
    data[0, 3, 5, 6] = 1.0
    want = check_mask_box_crop(lib, dev, data)
    assert want[2] == [[2, 4], [3, 6], [4, 7]]
    # seg absent: the -1 / 0 int8 map and empty class lists
    data, _, info = R.brain_case((21, 26, 30))
    props = {"spacing": (1.0, 1.0, 1.0)}
    d, s = P.preprocess_case(dev_t(data, dev), None, props)
    _, want_s, bb, filled = R.crop_to_nonzero(data, None)
    assert s.dtype == torch.int8 and np.array_equal(_np(s), want_s) and set(np.unique(want_s)) == {-1, 0}
    assert props["class_locations"] == {1: [], 2: [], 3: []} and props["bbox_used_for_cropping"] == bb
    # a seg containing 200: int16
    data, seg, _ = R.brain_case((21, 26, 30))
    seg[seg == 3] = 200
    props = {"spacing": (1.0, 1.0, 1.0)}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, all_labels=(1, 2, 200))
    want = R.run_case(data, seg, (1.0, 1.0, 1.0), all_labels=(1, 2, 200))
    assert (seg == 200).any() and s.dtype == torch.int16 and want[1].dtype == np.int16 and np.array_equal(_np(s), want[1])
    assert all(np.array_equal(props["class_locations"][k], want[2]["class_locations"][k]) for k in (1, 2, 200))
    # without it: int8
    seg[seg == 200] = 127
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)}, all_labels=(1, 2, 127))
    assert s.dtype == torch.int8 and int(s.max()) == 127


# ---- 2. normalisation -----------------------------------------------------------------------------------------------------------------
def _norm_within(got, x, inside=None, name=""):
    """got (fp32) against the float64 restatement, per voxel, and against the reference's literal float32 arithmetic"""
    ref, mean, std = R.zscore64(x, inside)
    bound = R.zscore_bound(x, mean, std)
    err = np.abs(got.astype(np.float64) - ref)
    sel = slice(None) if inside is None else inside
    worst = float((err[sel] / bound[sel]).max())
    lit = R.zscore32_literal(x, inside).astype(np.float64)
    lit_own = np.abs(lit - ref)
    print(f"normalisation {name}: mean {mean:.6g} std {std:.6g} worst error / bound {worst:.3f}; "
          f"numpy float32 against float64 / bound {float((lit_own[sel] / bound[sel]).max()):.3f}")
    assert (err[sel] <= bound[sel]).all(), (name, worst)
    assert (np.abs(got.astype(np.float64) - lit)[sel] <= (lit_own + bound)[sel]).all(), name
    if inside is not None:
        assert np.array_equal(got[~inside].view(np.uint32), np.asarray(x, dtype=np.float32)[~inside].view(np.uint32)), \
            "voxels outside the mask must be bit-equal to the input"


def check_normalisation(lib, dev, shape=(23, 30, 41)):
    data, seg, info = R.brain_case(shape)
    rng = np.random.RandomState(11)
    offset = (3.0e4 + rng.standard_normal(shape)).astype(np.float32)          # mean 3e4, std about 1
    const = np.full(shape, 7.25, dtype=np.float32)                            # std 0
    x = np.concatenate([data, offset[None], const[None]])
    assert abs(float(offset.astype(np.float64).mean()) - 3.0e4) < 1.0 and 0.9 < float(offset.astype(np.float64).std()) < 1.1
    t = dev_t(x, dev)
    got = P.zscore_normalize(t)
    assert got.dtype == torch.float32 and tuple(got.shape) == x.shape
    g = _np(got)
    for c in range(5):
        _norm_within(g[c], x[c], name=f"channel {c}" if c < 4 else "offset channel")
    assert np.array_equal(g[5], np.zeros(shape, dtype=np.float32)), "a constant channel gives exact zeros through the 1e-8 clamp"
    assert torch.equal(got, P.zscore_normalize(t)), "two calls must be bit-equal"
    s64a, s32a = ops_raw.crop_stats(lib, t)
    s64b, s32b = ops_raw.crop_stats(lib, t)
    assert torch.equal(s64a, s64b) and torch.equal(s32a, s32b)
    for c in range(6):
        mean, std = float(x[c].astype(np.float64).mean()), float(x[c].astype(np.float64).std())
        assert abs(float(s64a[c]) - mean) <= 1e-12 * max(abs(mean), 1.0) and abs(float(s64a[8 + c]) - std) <= 1e-9 * max(std, 1e-3), c
        assert float(s32a[c]) == float(np.float32(float(s64a[c]))) and float(s32a[8 + c]) == float(np.float32(float(s64a[8 + c])))
    assert float(s64a[16]) == float(np.prod(shape))
    # the masked form: statistics and normalisation over seg >= 0, the rest untouched
    _, crop_seg, bb, _ = R.crop_to_nonzero(data, seg)
    sl = (slice(None),) + tuple(slice(a, b) for a, b in bb)
    xc = np.ascontiguousarray(x[sl])
    inside = crop_seg[0] >= 0
    assert inside.any() and (~inside).any()
    xc[0][~inside] = 5.5                                                      # something to leave untouched
    gm = _np(P.zscore_normalize(dev_t(xc, dev), dev_t(crop_seg, dev), use_mask_for_norm=True))
    for c in range(5):
        _norm_within(gm[c], xc[c], inside, name=f"masked channel {c}")
    assert np.array_equal(gm[5][inside], np.zeros(int(inside.sum()), dtype=np.float32)) and (gm[5][~inside] == 7.25).all()
    # `preprocess_case` with the mask: the same through the fused path (statistics over seg >= 0 of the crop, the rest copied)
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)}, use_mask_for_norm=True)
    assert np.array_equal(_np(s), R.run_case(data, seg, (1.0, 1.0, 1.0), mask_norm=True)[1])
    raw_crop = np.ascontiguousarray(data[sl])
    for c in range(4):
        _norm_within(_np(d)[c], raw_crop[c], inside, name=f"preprocess_case masked channel {c}")


# ---- 3. class locations ---------------------------------------------------------------------------------------------------------------
def check_class_locations(dev):
    seg = R.big_class_seg()
    n1, n2, n3 = int((seg == 1).sum()), int((seg == 2).sum()), int((seg == 3).sum())
    assert n1 > 10 ** 6 and 0 < n2 < 10000 and n3 > 10000 and n3 * 0.01 < 10000 and not (seg == 4).any()
    classes = [1, 2, 3, 4, (2, 3), [1, 3]]
    want = R.sample_locations(seg, classes)
    got = P.sample_foreground_locations(dev_t(seg, dev), classes)
    assert list(got.keys()) == [1, 2, 3, 4, (2, 3), (1, 3)] == list(want.keys())
    assert len(want[1]) == int(np.ceil(n1 * 0.01)) > 10000 and len(want[2]) == n2 and len(want[3]) == 10000
    assert got[4] == [] and want[4] == []
    for k in (1, 2, 3, (2, 3), (1, 3)):
        assert isinstance(got[k], np.ndarray) and got[k].dtype == np.int64 and got[k].shape[1] == 4
        assert np.array_equal(got[k], want[k]), k
    # another seed gives other rows; a (d, h, w) seg gets the leading column of zeros
    other = P.sample_foreground_locations(dev_t(seg, dev), [3], seed=7)
    assert not np.array_equal(other[3], want[3])
    alone = P.sample_foreground_locations(dev_t(seg[0], dev), [2])[2]
    assert np.array_equal(alone, R.sample_locations(seg, [2])[2]) and (alone[:, 0] == 0).all()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------------------
def check_preprocess_case(lib, dev, data, seg, info, fill_fn=R.fill, expect_box=None, expect_added=None):
    """the whole of `preprocess_case` against the restatement, then back through `labels_from_logits`"""
    want_d, want_s, want_p, stats, filled = R.run_case(data, seg, (1.0, 1.0, 1.0), fill_fn=fill_fn)
    added = check_brain_case_conditions(data, seg, info, filled)
    print("preprocess_case", data.shape, "box", want_p["bbox_used_for_cropping"], "filling adds", added)
    if expect_box is not None:
        assert want_p["bbox_used_for_cropping"] == expect_box and added == expect_added
    props = {"spacing": (1.0, 1.0, 1.0), "raw_size": data.shape[1:], "name": "case"}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props)
    assert d.dtype == torch.float32 and s.dtype == torch.int8 and np.array_equal(_np(s), want_s)
    for key in ("original_spacing_trans", "target_spacing_trans", "shape_before_cropping", "bbox_used_for_cropping",
                "shape_after_cropping_before_resample", "shape_after_resample"):
        assert list(props[key]) == list(want_p[key]), key
    assert list(props["class_locations"].keys()) == [1, 2, 3]
    for k in (1, 2, 3):
        assert len(want_p["class_locations"][k]) > 0 and np.array_equal(props["class_locations"][k], want_p["class_locations"][k])
    g = _np(d)
    sl = tuple(slice(a, b) for a, b in want_p["bbox_used_for_cropping"])
    for c in range(data.shape[0]):
        x = data[c][sl]
        bound = R.zscore_bound(x, *stats[c])
        err = np.abs(g[c].astype(np.float64) - want_d[c])
        print(f"  channel {c}: mean {stats[c][0]:.6g} std {stats[c][1]:.6g} worst error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all(), c
    d2, s2 = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)})
    assert torch.equal(d, d2) and torch.equal(s, s2), "two calls must be bit-equal"
    # back: one-hot logits of clamp(seg, 0) -> labels_from_logits with the properties -> the original seg inside the filled mask
    onehot = torch.nn.functional.one_hot(s[0].long().clamp(min=0), 4).permute(3, 0, 1, 2).float().contiguous()
    back = _np(PP.labels_from_logits(onehot, props))
    orig = seg[0].astype(np.uint8)
    assert back.shape == orig.shape and np.array_equal(back[filled], orig[filled])
    differ = np.argwhere(back != orig)
    assert all(tuple(v) == tuple(info["stray"]) for v in differ), differ[:5]
    assert not (orig != 0)[~_in_box(orig.shape, want_p["bbox_used_for_cropping"])].any(), "no label lies outside the box"


def _in_box(shape, bb):
    m = np.zeros(shape, dtype=bool)
    m[tuple(slice(a, b) for a, b in bb)] = True
    return m


def _builtin_or_numpy(o) -> bool:
    if isinstance(o, dict):
        return all(_builtin_or_numpy(k) and _builtin_or_numpy(v) for k, v in o.items())
    if isinstance(o, (list, tuple)):
        return all(_builtin_or_numpy(v) for v in o)
    return type(o) in (int, float, str, bool, type(None), np.ndarray) or isinstance(o, np.generic)


def check_case_preprocessor(dev, tmp_path):
    """`CasePreprocessor.run` on files written with nifti.write_nifti: .npz / .pkl load back, the pickle holds builtin and numpy types"""
    raw, out = os.path.join(str(tmp_path), "raw"), os.path.join(str(tmp_path), "out")
    names = ["t1.nii.gz", "t1ce.nii.gz", "t2.nii.gz", "flair.nii.gz"]
    cases = {"case_b": R.brain_case((21, 26, 30), seed=1), "case_a": R.brain_case((19, 28, 27), seed=2)}
    for case, (data, seg, _) in cases.items():
        os.makedirs(os.path.join(raw, "images", case))
        for c, name in enumerate(names):
            nifti.write_nifti(os.path.join(raw, "images", case, name), data[c], (1.0, 1.0, 1.0))
        nifti.write_nifti(os.path.join(raw, "images", case, "seg.nii.gz"), seg[0].astype(np.uint8), (1.0, 1.0, 1.0))
    pre = P.CasePreprocessor(raw, "images", names, "seg.nii.gz")
    assert pre.get_iterable_list() == ["case_a", "case_b"]
    written = pre.run((1, 1, 1), out, (1, 2, 3))
    assert [os.path.basename(w) for w in written] == ["case_a.npz", "case_b.npz"]
    for case, (data, seg, _) in cases.items():
        want_d, want_s, want_p, stats, _ = R.run_case(data, seg, (1.0, 1.0, 1.0))
        z = np.load(os.path.join(out, case + ".npz"))
        with open(os.path.join(out, case + ".pkl"), "rb") as f:
            raw_pickle = f.read()
        props = pickle.loads(raw_pickle)
        assert b"torch" not in raw_pickle and _builtin_or_numpy(props)
        assert z["data"].dtype == np.float32 and z["seg"].dtype == np.int8 and np.array_equal(z["seg"], want_s)
        sl = tuple(slice(a, b) for a, b in want_p["bbox_used_for_cropping"])
        for c in range(4):
            assert (np.abs(z["data"][c].astype(np.float64) - want_d[c]) <= R.zscore_bound(data[c][sl], *stats[c])).all(), (case, c)
        assert props["name"] == case and tuple(props["raw_size"]) == data.shape[1:] and tuple(props["spacing"]) == (1.0, 1.0, 1.0)
        assert props["bbox_used_for_cropping"] == want_p["bbox_used_for_cropping"]
        assert all(np.array_equal(props["class_locations"][k], want_p["class_locations"][k]) for k in (1, 2, 3))
        # what the prediction side takes: the properties as they come out of the pickle
        onehot = torch.nn.functional.one_hot(dev_t(z["seg"][0], dev).long().clamp(min=0), 4).permute(3, 0, 1, 2).float().contiguous()
        assert tuple(PP.labels_from_logits(onehot, props).shape) == data.shape[1:]
    return out


# ---- 5. refusals and exports ------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    data, seg, _ = R.brain_case((21, 26, 30))
    with pytest.raises(NotImplementedError) as e:                            # x spacing 2 mm -> 1 mm: the crop would double along x
        P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (2.0, 1.0, 1.0)})
    crop = [b - a for a, b in R.crop_to_nonzero(data, seg)[2]]
    assert str(crop) in str(e.value) and str([crop[0], crop[1], 2 * crop[2]]) in str(e.value), "both shapes must be named"
    with pytest.raises(RuntimeError, match="zero everywhere"):
        P.preprocess_case(dev_t(np.zeros((2, 5, 6, 7), np.float32), dev), None, {"spacing": (1.0, 1.0, 1.0)})
    with pytest.raises(RuntimeError, match="zero everywhere"):
        P.crop_to_nonzero(dev_t(np.zeros((1, 4, 4, 4), np.float32), dev))
    bad = seg.copy()
    bad[0, 10, 13, 15] = 1.5
    with pytest.raises(RuntimeError, match="no integer"):
        P.preprocess_case(dev_t(data, dev), dev_t(bad, dev), {"spacing": (1.0, 1.0, 1.0)})
    bad[0, 10, 13, 15] = 40000.0
    with pytest.raises(RuntimeError, match="no integer"):
        P.preprocess_case(dev_t(data, dev), dev_t(bad, dev), {"spacing": (1.0, 1.0, 1.0)})
    t = dev_t(data, dev)
    m = dev_t(np.ones(data.shape[1:], np.uint8), dev)
    s32 = torch.zeros(16, dtype=torch.float32, device=dev)
    for call in (lambda: ops_raw.nonzero_mask_bbox(lib, t[0]),                                   # wrong rank
                 lambda: ops_raw.nonzero_mask_bbox(lib, t.double()),                             # wrong dtype
                 lambda: ops_raw.nonzero_mask_bbox(lib, t.repeat(3, 1, 1, 1)[:9]),                # more than 8 channels
                 lambda: ops_raw.nonzero_mask_bbox(lib, t[:, :, :, ::2]),                         # non-unit x stride
                 lambda: ops_raw.crop_stats(lib, t[0]),
                 lambda: ops_raw.crop_stats(lib, t.half()),
                 lambda: ops_raw.crop_stats(lib, t[:, :, :, ::2]),
                 lambda: ops_raw.crop_stats(lib, t, masked=True),                                # the masked form without the mask
                 lambda: ops_raw.crop_stats(lib, t, (0, 0, 0), (22, 26, 30)),                    # a box outside the volume
                 lambda: ops_raw.crop_stats(lib, t, (-1, 0, 0), (5, 5, 5)),
                 lambda: ops_raw.crop_stats(lib, t, mask=m[:, :, :-1]),                           # a mask of another shape
                 lambda: ops_raw.crop_stats(lib, t, mask=m.float()),
                 lambda: ops_raw.crop_normalize(lib, t, s32),                                    # the seg outputs without the mask
                 lambda: ops_raw.crop_normalize(lib, t, s32.double(), want_seg=False),
                 lambda: ops_raw.crop_normalize(lib, t, s32[:8], want_seg=False),
                 lambda: ops_raw.crop_normalize(lib, t, s32, mask=m, seg=m.long()),               # a seg dtype the kernel does not take
                 lambda: ops_raw.crop_normalize(lib, t, s32, mask=m, seg=m[1:]),
                 lambda: ops_raw.crop_normalize(lib, t, s32, mask=m, nonzero_label=-2),
                 lambda: ops_raw.crop_normalize(lib, t.repeat(3, 1, 1, 1)[:9], s32, want_seg=False),
                 lambda: ops_raw.crop_normalize(lib, t[:, :, :, ::2], s32, want_seg=False)):
        with pytest.raises(RuntimeError):
            call()
    # the C entry refuses what the wrapper would have refused
    a = L.CropArgs()
    assert lib.dll.segm_crop_stats(a) == -1
    a.data = t.data_ptr()
    a.channels, a.depth, a.height, a.width = 9, 4, 4, 4
    assert lib.dll.segm_crop_stats(a) == -2
    assert lib.dll.segm_crop_stats_workspace_bytes(9, 4, 4, 4) == 0 and lib.dll.segm_crop_stats_workspace_bytes(4, 4, 4, 4) > 0
    b = L.NonzeroMaskBboxArgs()
    assert lib.dll.segm_nonzero_mask_bbox(b) == -1


def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
