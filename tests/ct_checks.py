"""Checks shared by tests/test_emu_ct.py (kernel sources on the CPU emulator) and tests/test_gpu_ct.py (the HIP library): every
function takes the loaded library and the device its tensors live on.  References: tests/ct_ref.py (numpy).
No condition rests on a measured number: order statistics, min, max, median and the samples are equal to numpy's (`==`, the samples
as uint32); a percentile lies within 2^-23 max(|a|, |b|) of numpy's float64 interpolation and inside [a, b]; the mean within
2^-24 |m| + 2^-40 mean|x| of the float64 mean; the CT normalisation is bit-equal to the fp32 numpy expression.  Every check first
asserts the conditions on its own input that keep it from passing vacuously."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import nifti
from segmamba_amd import ops_raw
from segmamba_amd import preprocess as P
from tests import ct_ref as CR
from tests import preprocess_ref as R
from tests import resample_ref as RR
from tests.preprocess_checks import _builtin_or_numpy, dev_t
from tests.resample_checks import data_within

NEW_EXPORTS = ("segm_fg_workspace_bytes", "segm_fg_count", "segm_fg_order_stats", "segm_fg_gather", "segm_crop_clip_normalize")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ct_fingerprint.npz")
KEYS = ("mean", "median", "min", "max", "percentile_99_5", "percentile_00_5")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def boundary_ranks(mask):
    """the foreground ranks on both sides of every segment boundary of the logical volume, with 0 and n - 1"""
    flat = np.asarray(mask).reshape(-1)
    n = int(flat.sum())
    cum = np.concatenate([[0], np.cumsum(flat)])
    r = {0, n - 1}
    for b in range(CR.SEGMENT, flat.size, CR.SEGMENT):
        r |= {int(cum[b]) - 1, int(cum[b])}
    return sorted(k for k in r if 0 <= k < n)


# ---- 1. the raw entries and `collect_foreground_intensities` on one input ----------------------------------------------------------------
def check_statistics(got, fg, name):
    """one channel's dict against numpy on its foreground values"""
    assert set(got) == set(KEYS), name
    s = np.sort(fg)
    assert got["min"] == np.min(fg) and got["max"] == np.max(fg), name
    assert got["median"] == np.median(fg), (name, got["median"], np.median(fg))
    for key, q in (("percentile_00_5", 0.5), ("percentile_99_5", 99.5)):
        a, b = CR.percentile_neighbours(s, q)
        want = CR.percentile64(fg, q)
        err = abs(float(got[key]) - float(want))
        print(f"{name} {key}: got {got[key]!r} want {want!r} err {err:.3e} bound {2.0 ** -23 * max(abs(float(a)), abs(float(b))):.3e}")
        assert err <= 2.0 ** -23 * max(abs(float(a)), abs(float(b))), (name, key)
        assert min(a, b) <= got[key] <= max(a, b), (name, key)
    m = float(np.asarray(fg, dtype=np.float64).mean())
    print(f"{name} mean: got {got['mean']!r} want {m!r} bound {CR.mean_bound(fg):.3e}")
    assert abs(float(got["mean"]) - m) <= CR.mean_bound(fg), name
    for k in KEYS:
        assert isinstance(got[k], np.float32), (name, k, type(got[k]))


def check_fingerprint(lib, dev, images, seg, name, images_t=None, num_samples=10000):
    """images (C, D, H, W) float32 and seg (1, D, H, W) as numpy; `images_t` a device tensor to send instead (a strided view)"""
    images = np.asarray(images)
    mask = np.asarray(seg)[0] > 0
    n = int(mask.sum())
    fg = CR.foreground(seg, images)
    x = dev_t(images, dev) if images_t is None else images_t
    s = dev_t(seg[0], dev)
    count, sums, state = ops_raw.fg_count(lib, x, s)
    assert count.dtype == torch.int64 and int(count) == n, (name, int(count), n)
    count2, sums2, _ = ops_raw.fg_count(lib, x, s)
    assert torch.equal(count, count2) and torch.equal(sums.view(torch.int64), sums2.view(torch.int64)), "two calls must be bit-equal"
    got = P.collect_foreground_intensities(dev_t(seg, dev), x, num_samples=num_samples)
    if n == 0:
        assert got[0] == [[] for _ in fg] and all(set(d) == set(KEYS) and all(np.isnan(v) for v in d.values()) for d in got[1])
        assert np.array_equal(_np(sums)[:len(fg)], np.zeros(len(fg)))
        return n
    for c, f in enumerate(fg):
        assert abs(float(sums[c]) - float(f.astype(np.float64).sum())) <= 2.0 ** -40 * float(np.abs(f.astype(np.float64)).sum()), (name, c)
    # order statistics: the ends, a repeated rank, ranks inside runs of equal values
    rank_sets = [[0, n - 1, n // 2, n // 2, (n - 1) // 2, min(5, n - 1), n // 3, n - 1], [n - 1], [0, 0, (2 * n) // 3]]
    for ranks in rank_sets:
        o = ops_raw.fg_order_stats(lib, state, n, ranks)
        assert o.dtype == torch.float32 and tuple(o.shape) == (len(fg), len(ranks))
        for c, f in enumerate(fg):
            want = np.sort(f)[ranks]
            assert (_np(o)[c] == want).all(), (name, c, ranks, _np(o)[c], want)
        o2 = ops_raw.fg_order_stats(lib, state, n, ranks)
        assert np.array_equal(_bits(_np(o)), _bits(_np(o2))), "two calls must be bit-equal"
    # the gather on its own: unsorted, repeats, both sides of every segment boundary
    rng = np.random.RandomState(n % 9973)
    edge = boundary_ranks(mask)
    idx = np.concatenate([edge, edge[::-1], rng.randint(0, n, 300), [n - 1, 0, 0]]).astype(np.int64)
    rng.shuffle(idx)
    g = ops_raw.fg_gather(lib, state, n, idx)
    assert g.dtype == torch.float32 and tuple(g.shape) == (len(fg), len(idx))
    for c, f in enumerate(fg):
        assert np.array_equal(_bits(_np(g)[c]), _bits(f[idx])), (name, c)
    per_channel = np.stack([np.roll(idx, 7 * c) for c in range(len(fg))])
    g2 = ops_raw.fg_gather(lib, state, n, dev_t(per_channel, dev))           # a draw per channel, already on the device
    for c, f in enumerate(fg):
        assert np.array_equal(_bits(_np(g2)[c]), _bits(f[per_channel[c]])), (name, c)
    assert torch.equal(g.view(torch.int32), ops_raw.fg_gather(lib, state, n, idx).view(torch.int32)), "two calls must be bit-equal"
    # the public function against the restatement
    want_samples, _ = CR.collect_foreground_intensities(seg, images, num_samples=num_samples)
    assert len(got[0]) == len(fg) == len(got[1])
    for c, f in enumerate(fg):
        assert isinstance(got[0][c], np.ndarray) and got[0][c].dtype == np.float32 and got[0][c].shape == (num_samples,)
        assert np.array_equal(_bits(got[0][c]), _bits(want_samples[c])), (name, c, "the samples must be the reference's draws")
        check_statistics(got[1][c], f, f"{name} channel {c}")
    again = P.collect_foreground_intensities(dev_t(seg, dev), x, num_samples=num_samples)
    for c in range(len(fg)):
        assert np.array_equal(_bits(got[0][c]), _bits(again[0][c]))
        assert all(_bits(got[1][c][k]) == _bits(again[1][c][k]) for k in KEYS), "two calls must be bit-equal"
    return n


def check_volumes(lib, dev):
    """(19, 37, 53): odd, several segments, the last one partial; (3, 5, 7): less than one segment.  Foreground: a blob across segment
    boundaries, one voxel, two voxels, every voxel, none, only the last partial segment.  Seg as float32, uint8, int16; two channels"""
    shape = (19, 37, 53)
    nvox = int(np.prod(shape))
    assert nvox == 37259 and nvox % CR.SEGMENT != 0 and nvox // CR.SEGMENT >= 8
    images = np.stack([CR.hu(shape, 1), (np.random.RandomState(2).standard_normal(shape) * 7.0 + 3.0).astype(np.float32)])
    b = CR.blob(shape)
    assert len(boundary_ranks(b)) >= 10, "the blob must straddle segment boundaries"
    last = np.zeros(nvox, dtype=bool)
    last[(nvox // CR.SEGMENT) * CR.SEGMENT + 3::5] = True
    one, two = np.zeros(shape, dtype=bool), np.zeros(shape, dtype=bool)
    one[11, 20, 31] = True
    two[0, 0, 1], two[18, 36, 52] = True, True
    masks = {"blob": b, "single": one, "two": two, "all": np.ones(shape, dtype=bool), "none": np.zeros(shape, dtype=bool),
             "last segment": last.reshape(shape)}
    counts = {}
    for k, (name, m) in enumerate(masks.items()):
        dt = (np.float32, np.uint8, np.int16)[k % 3]
        seg = np.where(m, 1 + (np.arange(nvox).reshape(shape) % 3), 0).astype(dt)
        seg[~m & (np.arange(nvox).reshape(shape) % 11 == 0)] = -1 if dt != np.uint8 else 0          # a negative label is background
        counts[name] = check_fingerprint(lib, dev, images, seg[None], f"{name} seg {np.dtype(dt).name}",
                                         num_samples=10000 if name == "blob" else 1000)
    assert counts["single"] == 1 and counts["two"] == 2 and counts["all"] == nvox and counts["none"] == 0
    assert 0 < counts["last segment"] < CR.SEGMENT
    # a NaN in a float32 seg is not foreground
    seg = np.where(b, 2.0, 0.0).astype(np.float32)
    seg[~b & (np.arange(nvox).reshape(shape) % 13 == 0)] = np.nan
    assert check_fingerprint(lib, dev, images, seg[None], "NaN in the seg") == int(b.sum())
    small = (3, 5, 7)
    rng = np.random.RandomState(4)
    for name, m in (("small random", rng.random_sample(small) < 0.4), ("small all", np.ones(small, dtype=bool))):
        check_fingerprint(lib, dev, np.stack([CR.hu(small, 5), CR.hu(small, 6)]), m.astype(np.uint8)[None], name)


def check_strided_views(lib, dev):
    """a non-contiguous channel view and an H-strided view with a unit x stride go to the kernels as they are"""
    rng = np.random.RandomState(8)
    big = np.round(rng.standard_normal((5, 19, 40, 56)) * 200.0).astype(np.float32)
    big_t = dev_t(big, dev)
    for name, view in (("every other channel", lambda a: a[::2, :, 3:40, 3:56]), ("H strided", lambda a: a[1:3, :, ::2, 2:55])):
        host, t = np.ascontiguousarray(view(big)), view(big_t)
        assert not t.is_contiguous() and t.stride(-1) == 1
        seg = (CR.blob(host.shape[1:]) * 3).astype(np.int16)
        assert len(boundary_ranks(seg > 0)) >= 6
        check_fingerprint(lib, dev, host, seg[None], name, images_t=t)


def check_values(lib, dev):
    """heavy ties, mixed signs, a constant, values that differ only in the key's last digit, only in its top digit, both zeros"""
    shape = (19, 37, 53)
    chans = CR.value_channels(shape)
    assert list(chans) == ["hu", "mixed", "constant", "last_digit", "top_digit", "zeros"]
    m = CR.blob(shape)
    keys = {k: v[m].view(np.uint32) for k, v in chans.items()}
    assert len(np.unique(chans["hu"][m])) < m.sum() // 4 and (chans["mixed"][m] < 0).any() and (chans["mixed"][m] > 0).any()
    assert len(np.unique(keys["last_digit"] >> 10)) == 1 and len(np.unique(keys["last_digit"] & 1023)) > 500
    assert len(np.unique(keys["top_digit"] & 0xfffff)) == 1 and len(np.unique(keys["top_digit"] >> 20)) > 1000
    assert np.isfinite(chans["top_digit"]).all()
    z = chans["zeros"][m]
    assert (np.signbit(z) & (z == 0)).any() and (~np.signbit(z) & (z == 0)).any(), "both zeros among the foreground"
    images = np.stack(list(chans.values()))
    check_fingerprint(lib, dev, images, m.astype(np.uint8)[None], "value patterns")


# ---- 2. the recorded fixture --------------------------------------------------------------------------------------------------------------
def check_golden(lib, dev):
    """samples and statistics the reference's own `collect_foreground_intensities` gave for the stand-in case (tests/golden/
    make_golden_ct_fingerprint.py): the samples bit-equal, the statistics as against numpy"""
    g = np.load(GOLDEN)
    data, seg = CR.ct_case()
    samples, stats = P.collect_foreground_intensities(dev_t(seg, dev), dev_t(data, dev))
    assert g["samples"].shape == (1, 10000) and np.array_equal(_bits(samples[0]), _bits(g["samples"][0]))
    want = dict(zip([str(k) for k in g["keys"]], g["statistics"][0]))
    for k in ("min", "max", "median"):
        assert stats[0][k] == want[k], k
    fg = CR.foreground(seg, data)[0]
    assert np.float32(np.median(fg)) == want["median"] and np.float32(np.mean(fg)) == want["mean"], "the fixture is this case's"
    check_statistics(stats[0], fg, "golden case")


# ---- 3. CT normalisation ----------------------------------------------------------------------------------------------------------------
PROPS2 = {"0": {"mean": 31.7, "std": 57.3, "percentile_00_5": -80.5, "percentile_99_5": 140.25},
          "1": {"mean": -3.0, "std": 1e-9, "percentile_00_5": -4.0, "percentile_99_5": 2.5}}


def check_ct_normalize(lib, dev):
    """bit-equal to the fp32 numpy expression; bounds that cut both tails; a std below 1e-8; list, str-keyed and int-keyed properties;
    a strided view; and `segm_crop_normalize` keeps its bits beside the shared kernel body"""
    shape = (13, 22, 37)
    x = np.stack([CR.hu(shape, 11), np.round(np.random.RandomState(12).standard_normal(shape) * 4.0).astype(np.float32)])
    for c in range(2):
        p = PROPS2[str(c)]
        assert (x[c] < p["percentile_00_5"]).any() and (x[c] > p["percentile_99_5"]).any(), "both tails must be cut"
    want = np.stack([CR.ct_normalize32(x[c], PROPS2[str(c)]) for c in range(2)])
    for c in range(2):
        assert np.array_equal(_bits(want[c]), _bits(CR.ct_normalize_literal(x[c], PROPS2[str(c)]))), "the restatement is the reference's lines"
    for props in (PROPS2, [PROPS2["0"], PROPS2["1"]], {0: PROPS2["0"], 1: PROPS2["1"]}):
        got = P.ct_normalize(dev_t(x, dev), props)
        assert got.dtype == torch.float32 and np.array_equal(_bits(_np(got)), _bits(want))
    big = np.zeros((2, 13, 30, 45), dtype=np.float32)
    big[:, :, 4:26, 5:42] = x
    got = P.ct_normalize(dev_t(big, dev)[:, :, 4:26, 5:42], PROPS2)
    assert np.array_equal(_bits(_np(got)), _bits(want))
    assert torch.equal(P.ct_normalize(dev_t(x, dev), PROPS2), P.ct_normalize(dev_t(x, dev), PROPS2))
    # identity statistics through the clip entry with open bounds = the plain entry
    st = torch.cat([torch.zeros(8), torch.ones(8)]).to(dev)
    st32 = torch.cat([torch.zeros(8), torch.ones(8), torch.full((8,), -3e38), torch.full((8,), 3e38)]).to(dev)
    a = ops_raw.crop_normalize(lib, dev_t(x, dev), st, want_seg=False)[0]
    b = ops_raw.crop_clip_normalize(lib, dev_t(x, dev), st32, want_seg=False)[0]
    assert np.array_equal(_bits(_np(a)), _bits(x)) and torch.equal(a, b)


def check_preprocess_case_ct(lib, dev):
    """`preprocess_case(normalization="ct")`: data bit-equal to the restatement, box, seg, counts through the class locations, and the
    added properties equal; seg as None; the keys as ints"""
    data, seg = CR.ct_case()
    props_in = {"0": {"mean": 55.0, "std": 71.0, "percentile_00_5": -90.0, "percentile_99_5": 170.0}}
    assert (data < -90.0).any() and (data > 170.0).any()
    want_d, want_s, want_p = CR.run_case_ct(data, seg, (1.0, 1.0, 1.0), props_in, all_labels=(1, 2))
    assert list(want_d.shape[1:]) != list(data.shape[1:]) and (want_s == -1).any() and {1, 2} <= set(np.unique(want_s))
    props = {"spacing": (1.0, 1.0, 1.0)}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, all_labels=(1, 2), normalization="ct",
                             foreground_intensity_properties_per_channel=props_in)
    assert d.dtype == torch.float32 and np.array_equal(_bits(_np(d)), _bits(want_d)), "the CT-normalised crop must be bit-equal"
    assert s.dtype == torch.int8 and np.array_equal(_np(s), want_s)
    for k, v in want_p.items():
        if k != "class_locations":
            assert props[k] == v, k
    for k in (1, 2):
        assert len(want_p["class_locations"][k]) > 0 and np.array_equal(props["class_locations"][k], want_p["class_locations"][k])
    assert _builtin_or_numpy(props) and b"torch" not in pickle.dumps(props)
    d2, s2 = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)}, all_labels=(1, 2), normalization="ct",
                               foreground_intensity_properties_per_channel={0: props_in["0"]})
    assert torch.equal(d, d2) and torch.equal(s, s2)
    d3, s3 = P.preprocess_case(dev_t(data, dev), None, {"spacing": (1.0, 1.0, 1.0)}, normalization="ct",
                               foreground_intensity_properties_per_channel=props_in)
    assert torch.equal(d, d3) and np.array_equal(_np(s3), R.crop_to_nonzero(data, None)[1])
    return data, seg, props_in, _np(d), _np(s)


def check_preprocess_case_ct_resampled(lib, dev):
    """spacing (0.8, 0.8, 2.0) -> (1, 1, 1): the resampled data within the resampling's own bound of the restatement applied to the
    CT-normalised crop"""
    data, seg, props_in, d0, s0 = check_preprocess_case_ct(lib, dev)
    spacing = (0.8, 0.8, 2.0)
    props = {"spacing": spacing}
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), props, all_labels=(1, 2), resample=True, normalization="ct",
                             foreground_intensity_properties_per_channel=props_in)
    new_shape = [int(round(i / j * k)) for i, j, k in zip(spacing[::-1], (1, 1, 1), d0.shape[1:])]
    assert new_shape != list(d0.shape[1:]) and props["shape_after_resample"] == new_shape
    assert tuple(d.shape) == (1,) + tuple(new_shape) and tuple(s.shape) == (1,) + tuple(new_shape) and s.dtype == torch.int8
    data_within(_np(d)[0], d0[0], new_shape, 3, True, "ct preprocess_case")
    want_s, weights = RR.zoom_labels_ref(s0[0], new_shape)
    assert RR.reachable(_np(s)[0], weights).all()
    with pytest.raises(NotImplementedError):
        P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": spacing}, normalization="ct",
                          foreground_intensity_properties_per_channel=props_in)


def check_default_route_unchanged(lib, dev):
    """`preprocess_case` with default arguments = `segm_crop_stats` + `segm_crop_normalize` called directly"""
    data, seg, _ = R.brain_case((21, 26, 30))
    d, s = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)})
    x = dev_t(data, dev)
    filled = P.create_nonzero_mask(x)
    bb = R.bbox_of(_np(filled).astype(bool))
    start, shp = [b[0] for b in bb], [b[1] - b[0] for b in bb]
    _, st = ops_raw.crop_stats(lib, x, start, shp, mask=filled, seg=dev_t(seg[0], dev))
    want_d, want_s, _ = ops_raw.crop_normalize(lib, x, st, start, shp, mask=filled, seg=dev_t(seg[0], dev))
    assert torch.equal(d.view(torch.int32), want_d.view(torch.int32)) and torch.equal(s[0].to(torch.int16), want_s)
    d2, s2 = P.preprocess_case(dev_t(data, dev), dev_t(seg, dev), {"spacing": (1.0, 1.0, 1.0)}, normalization="zscore")
    assert torch.equal(d, d2) and torch.equal(s, s2)


# ---- 4. CTCasePreprocessor on files ---------------------------------------------------------------------------------------------------------
def _write_ct_cases(root, cases):
    os.makedirs(os.path.join(root, "imagesTr"))
    os.makedirs(os.path.join(root, "labelsTr"))
    for name, (data, seg, spacing) in cases.items():
        nifti.write_nifti(os.path.join(root, "imagesTr", name), data[0], spacing)
        nifti.write_nifti(os.path.join(root, "labelsTr", name), seg[0].astype(np.uint8), spacing)


def check_ct_case_preprocessor(dev, tmp_path):
    """three cases of different shapes and spacings, one without foreground: `run_plan` against numpy on the restatement's samples, the
    JSON, `run`'s files; then an anisotropic set that takes the `has_aniso_spacing and has_aniso_voxels` branch"""
    cases = {"ct_a.nii.gz": CR.ct_case((40, 44, 48), 0) + ((0.8, 0.8, 2.0),),
             "ct_b.nii.gz": CR.ct_case((36, 50, 42), 1) + ((1.0, 1.0, 1.5),),
             "ct_c.nii.gz": CR.ct_case((30, 40, 40), 2, labels=False) + ((0.7, 0.7, 2.5),)}
    root = str(tmp_path / "set1")
    _write_ct_cases(root, cases)
    pre = P.CTCasePreprocessor(root, "imagesTr", "labelsTr")
    names = pre.get_iterable_list()
    assert names == sorted(cases)
    data, seg, props = pre.read_data("ct_a.nii.gz")
    assert data.dtype == np.float32 and data.shape == cases["ct_a.nii.gz"][0].shape and np.array_equal(seg, cases["ct_a.nii.gz"][1])
    assert props["spacing"] == pytest.approx((0.8, 0.8, 2.0)) and props["raw_size"] == (40, 44, 48) and props["name"] == "ct_a"
    samples = [CR.collect_foreground_intensities(cases[n][1], cases[n][0])[0] for n in names]
    assert samples[2] == [[]] and np.array_equal(_bits(props["intensities_per_channel"][0]), _bits(samples[0][0]))
    spacings = [pre.read_data(n)[2]["spacing"] for n in names]
    sizes = [cases[n][0].shape[1:] for n in names]
    want, aniso = CR.run_plan(spacings, sizes, samples)
    assert not aniso
    path = str(tmp_path / "plan.txt")
    plan = pre.run_plan(path)
    assert plan == want, (plan, want)
    back = json.loads(open(path).read())
    assert set(back) == {"intensity_statistics_per_channel", "fullres spacing", "median_shape", "initial_patch_size"}
    assert back["intensity_statistics_per_channel"]["0"] == want["intensity_statistics_per_channel"][0]
    assert back["fullres spacing"] == want["fullres spacing"] and back["median_shape"] == want["median_shape"]
    assert back["initial_patch_size"] == want["initial_patch_size"]
    out = str(tmp_path / "out")
    written = pre.run(back["fullres spacing"][::-1], out, [1, 2], back["intensity_statistics_per_channel"])
    assert len(written) == 3
    for n in names:
        stem = os.path.join(out, n.split(".")[0])
        z = np.load(stem + ".npz", allow_pickle=True)
        p = pickle.load(open(stem + ".pkl", "rb"))
        assert _builtin_or_numpy(p) and b"torch" not in open(stem + ".pkl", "rb").read()
        assert z["data"].dtype == np.float32 and list(z["data"].shape[1:]) == p["shape_after_resample"] == list(z["seg"].shape[1:])
        assert {"intensities_per_channel", "intensity_statistics_per_channel", "class_locations", "bbox_used_for_cropping"} <= set(p)
    # case a on its own: the written data are `preprocess_case` on the arrays
    d, s = P.preprocess_case(dev_t(cases["ct_a.nii.gz"][0], dev), dev_t(cases["ct_a.nii.gz"][1], dev), {"spacing": spacings[0]},
                             back["fullres spacing"][::-1], [1, 2], resample=True, normalization="ct",
                             foreground_intensity_properties_per_channel=back["intensity_statistics_per_channel"])
    z = np.load(os.path.join(out, "ct_a.npz"))
    assert np.array_equal(_bits(z["data"]), _bits(_np(d))) and np.array_equal(z["seg"], _np(s))
    with pytest.raises(RuntimeError, match="foreground_intensity_properties_per_channel"):
        pre.run((1, 1, 1), out, [1, 2])
    # the anisotropic branch as the reference takes it: the coarsest axis is found among the spacings (x, y, z), the voxel counts it
    # compares are the raw sizes (z, y, x) at the same index - so the third spacing is coarse and the third size is small
    thick = {f"t{k}.nii.gz": CR.ct_case((40 + 2 * k, 44, 8 + k), 5 + k) + ((0.7 + 0.1 * k, 0.7 + 0.1 * k, 4.0 + 0.5 * k),) for k in range(3)}
    root2 = str(tmp_path / "set2")
    _write_ct_cases(root2, thick)
    pre2 = P.CTCasePreprocessor(root2, "imagesTr", "labelsTr")
    names2 = pre2.get_iterable_list()
    spacings2 = [pre2.read_data(n)[2]["spacing"] for n in names2]
    sizes2 = [thick[n][0].shape[1:] for n in names2]
    want2, aniso2 = CR.run_plan(spacings2, sizes2, [CR.collect_foreground_intensities(thick[n][1], thick[n][0])[0] for n in names2])
    assert aniso2, "this set must take the anisotropic branch"
    assert pre2.run_plan(None) == want2
    assert np.array_equal(pre2.determine_fullres_target_spacing(spacings2, sizes2), np.array(want2["fullres spacing"]))
    assert np.array_equal(pre2.compute_new_shape(sizes2[0], spacings2[0], want2["fullres spacing"]),
                          CR.compute_new_shape(sizes2[0], spacings2[0], want2["fullres spacing"]))


# ---- 5. refusals, exports -----------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    shape = (5, 6, 12)
    x = dev_t(np.random.RandomState(0).standard_normal((2,) + shape).astype(np.float32), dev)
    seg = dev_t((np.arange(360).reshape(shape) % 3).astype(np.uint8), dev)
    count, _, state = ops_raw.fg_count(lib, x, seg)
    n = int(count)
    assert n == 240
    with pytest.raises(RuntimeError, match="channels"):
        ops_raw.fg_count(lib, dev_t(np.zeros((9,) + shape, dtype=np.float32), dev), seg)
    with pytest.raises(RuntimeError, match="ranks"):
        ops_raw.fg_order_stats(lib, state, n, list(range(9)))
    for bad in ([n], [-1], [0, n + 5]):
        with pytest.raises(RuntimeError, match="rank"):
            ops_raw.fg_order_stats(lib, state, n, bad)
    for bad in ([0, n], [-1, 3]):
        with pytest.raises(RuntimeError, match="index"):
            ops_raw.fg_gather(lib, state, n, np.array(bad))
    with pytest.raises(RuntimeError, match="unit stride"):
        ops_raw.fg_count(lib, x[:, :, :, ::2], seg[:, :, ::2].contiguous())
    with pytest.raises(RuntimeError, match="seg"):
        ops_raw.fg_count(lib, x, seg.to(torch.int32))
    with pytest.raises(RuntimeError, match="workspace"):
        ops_raw.fg_count(lib, x, seg, workspace=torch.empty(16, dtype=torch.int64, device=x.device))
    # the entries themselves: every refusal is a status, nothing is launched
    a = state.fresh()
    a.n, a.n_ranks, a.out = n, 9, x.data_ptr()
    assert lib.dll.segm_fg_order_stats(a) == -2
    a.n_ranks = 1
    a.ranks[0] = n
    assert lib.dll.segm_fg_order_stats(a) == -2
    a.ranks[0] = 0
    a.channels = 9
    assert lib.dll.segm_fg_order_stats(a) == -2
    a.channels = 2
    a.workspace_bytes = 64
    assert lib.dll.segm_fg_order_stats(a) == -6 and lib.dll.segm_fg_gather(a) == -6 and lib.dll.segm_fg_count(a) == -6
    a = state.fresh()
    a.seg_dtype = L.PREP_SEG_NONE
    assert lib.dll.segm_fg_count(a) == -4
    a = state.fresh()
    assert lib.dll.segm_fg_count(a) == -1, "count and sums are required"
    assert lib.dll.segm_fg_workspace_bytes(9, 100) == 0 and lib.dll.segm_fg_workspace_bytes(1, 2 ** 31) == 0
    assert lib.dll.segm_fg_workspace_bytes(1, 400 * 512 * 512) < 600 * 1024
    # CT normalisation
    with pytest.raises(RuntimeError, match="foreground_intensity_properties_per_channel"):
        P.preprocess_case(x, None, {"spacing": (1.0, 1.0, 1.0)}, normalization="ct")
    with pytest.raises(RuntimeError, match="normalization"):
        P.preprocess_case(x, None, {"spacing": (1.0, 1.0, 1.0)}, normalization="minmax")
    with pytest.raises(RuntimeError, match="missing"):
        P.ct_normalize(x, [{"mean": 0.0, "std": 1.0}] * 2)
    with pytest.raises(RuntimeError, match="channel 1"):
        P.ct_normalize(x, {"0": PROPS2["0"]})
    with pytest.raises(RuntimeError, match="stats32"):
        ops_raw.crop_clip_normalize(lib, x, torch.zeros(16, device=x.device), want_seg=False)


def check_exports(lib):
    assert lib.missing == [] and lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    for name in NEW_EXPORTS:
        assert name in L.EXPORTS and hasattr(lib.dll, name), name


# ---- 6. at size (GPU only) ------------------------------------------------------------------------------------------------------------
def check_large(lib, dev):
    """1 x 96 x 160 x 160 with about a third foreground: many workgroups flush histograms, the offsets span hundreds of segments"""
    shape = (96, 160, 160)
    m = CR.blob(shape, radii=[n / 2.33 for n in shape])
    share = m.mean()
    assert 0.28 < share < 0.38 and m.size // CR.SEGMENT == 600
    images = CR.hu(shape, 21)[None]
    check_fingerprint(lib, dev, images, m.astype(np.uint8)[None], "96 x 160 x 160")
