"""Checks shared by tests/test_emu_surface.py (kernel sources on the CPU emulator) and tests/test_gpu_surface.py (the HIP library):
`segm_border_stats` against the list route (`border_distances` + torch.sort) exactly, and the evaluation report of
segmamba_amd.metrics (asd / assd / nsd, the confusion family, case_report, evaluate_report, tools/compute_metrics.py --report) against
tests/surface_ref.py.  Every function takes the loaded library and / or the device its tensors live on."""
import functools
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw
from tests import metrics_checks as K
from tests import metrics_ref as R
from tests import surface_ref as S

ANISO = K.ANISO
SPACINGS = (None,) + ANISO
TAUS = (0.0, 1.0, 2.5)
TAUS_ANISO = (0.0, 1.1, 2.7)               # (1.5, 0.8, 1.0) has distances of exactly 1.0 and 2.5: see assert_tau_is_safe
ENTRY_CASES = ("33x47x21", "40x48x36", "slab", "wide_row")
NEW_EXPORTS = ("segm_border_stats", "segm_border_stats_workspace_bytes")
W = L.METRICS_MAX_PLANES
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x: float) -> int:
    return np.float64(x).view(np.int64).item()


@functools.lru_cache(maxsize=None)
def ref_lists(case, spacing):
    """per BraTS region the fp64 brute-force lists (P -> G, G -> P) of a label case; None for a region that is empty on a side"""
    pred, gt = K.LABEL_CASES[case]()
    out = []
    for reg in R.BRATS_REGIONS:
        a, b = R.region_mask(pred, reg), R.region_mask(gt, reg)
        out.append((R.surface_distances(a, b, spacing), R.surface_distances(b, a, spacing)) if a.any() and b.any() else None)
    return out


def assert_tau_is_safe(case, spacing, taus):
    """a condition on the INPUTS, checked on the reference: no distance lies within 1e-5 tau of a tau used with an anisotropic
    spacing, where the fp32 transform (1e-6 relative) could put a distance on the other side of it.  tau = 0 needs no check: a
    distance of 0 is a voxel on both borders, and 0 is exact in every arithmetic."""
    if spacing is None:
        return
    taus = [t for t in taus if t > 0]
    for lists in ref_lists(case, spacing):
        if lists is None:
            continue
        d = np.hstack(lists)
        for tau in taus:
            assert not (np.abs(d - tau) <= 1e-5 * tau).any(), (case, spacing, tau)


# ---- the entry against the list route ------------------------------------------------------------------------------------------------
def expected_from_lists(lib, borders, edt, items, groups, n_groups, tols, ranks):
    """item rows and group rows from `border_distances` on the same edt: list length, fp64 sum, max, (list <= tau).sum(), and
    torch.sort(joined)[rank] (NaN for a rank outside the list)"""
    host = borders.cpu().numpy()
    counts = [int(((host[v] >> b) & 1).sum()) for v, b, _ in items]
    flat = ops_raw.border_distances(lib, borders, edt, items, counts)
    lists, off = [], 0
    for c in counts:
        lists.append(flat[off:off + c])
        off += c
    rows = []
    for lst, tau in zip(lists, tols):
        n = lst.numel()
        rows.append((n, float(lst.double().sum()) if n else 0.0, float(lst.max()) if n else 0.0,
                     int((lst <= tau).sum()) if tau is not None and tau >= 0 else 0))
    picks = []
    for g in range(n_groups):
        mine = [lists[i] for i in range(len(items)) if groups[i] == g]
        s = torch.sort(torch.cat(mine)).values if mine else torch.empty(0)
        picks.append(tuple(float(s[k]) if 0 <= k < s.numel() else math.nan for k in ranks[g]))
    return counts, rows, picks


def check_stats(lib, borders, edt, items, groups, n_groups, tols, ranks):
    """one call of `border_stats` against the lists; two calls bit-equal; the rows past the items and groups"""
    counts, rows, picks = expected_from_lists(lib, borders, edt, items, groups, n_groups, tols, ranks)
    out = ops_raw.border_stats(lib, borders, edt, items, groups, n_groups, tols, ranks)
    assert out.dtype == torch.float64 and tuple(out.shape) == (6 * W,)
    again = ops_raw.border_stats(lib, borders, edt, items, groups, n_groups, tols, ranks)
    assert torch.equal(out.view(torch.int64), again.view(torch.int64))
    got = out.tolist()
    for i, (n, total, top, within) in enumerate(rows):
        cnt, s, mx, wi = got[4 * i:4 * i + 4]
        print("item", i, items[i], "count", cnt, "sum", s, "max", mx, "within", wi, "lists", (n, total, top, within))
        assert cnt == n and mx == top and wi == within
        assert abs(s - total) <= 2 * n * 2.0 ** -53 * total          # two orders of one sum of n non-negative terms
    assert got[4 * len(items):4 * W] == [0.0] * (4 * (W - len(items)))
    for g, want in enumerate(picks):
        have = got[4 * W + 2 * g:4 * W + 2 * g + 2]
        print("group", g, "ranks", ranks[g], "values", have, "sorted list", want)
        for h, w in zip(have, want):
            assert (math.isnan(h) and math.isnan(w)) or h == w, (g, ranks[g], have, want)
    assert all(math.isnan(v) for v in got[4 * W + 2 * n_groups:])
    return counts, got


def percentile_ranks(n):
    lo = int(math.floor(0.95 * (n - 1)))
    return lo, min(lo + 1, n - 1)


def check_entry_on_case(lib, dev, case, spacing):
    """all three regions and both directions in one call (6 items, 3 groups) at tau in {0, 1, 2.5} (unit spacing) or {0, 1.1, 2.7}"""
    taus = TAUS if spacing is None else TAUS_ANISO
    assert_tau_is_safe(case, spacing, taus)
    pred, gt = K.LABEL_CASES[case]()
    borders, counts = ops_raw.seg_regions(lib, K.dev_t(pred, dev), K.dev_t(gt, dev), K.table(dev))
    c = counts.tolist()
    planes, items, groups, ranks = [], [], [], []
    for r in range(3):
        assert c[0][r] > 0 and c[1][r] > 0 and c[0][r] < pred.size and c[1][r] < pred.size
        planes += [(0, r), (1, r)]
        items += [(0, r, 2 * r + 1), (1, r, 2 * r)]
        groups += [r, r]
        ranks.append(percentile_ranks(c[3][r] + c[4][r]))
    edt = ops_raw.edt_sq(lib, borders, planes, spacing)
    for tau in taus:
        got_counts, got = check_stats(lib, borders, edt, items, groups, 3, [tau] * 6, ranks)
        assert got_counts == [c[3 + (i & 1)][i >> 1] for i in range(6)]              # the region pass's border counts
    return got


def thin_pair():
    """(2, 3, 300): the voxel (0, 0, 0) of P and the voxel (0, 0, 299) of G plus a small blob each (the rest of the plane x = 0; a
    1 x 2 x 3 block at x = 296 .. 298): the voxel of G is 299 from P, squared key 89 401 > 2^16, and every other squared distance lies
    between 296^2 and 299^2 + 5, so the selection's upper digits decide"""
    pred, gt = np.zeros((2, 3, 300), np.uint8), np.zeros((2, 3, 300), np.uint8)
    pred[:, :, 0] = 1
    gt[0, 0, 299] = 1
    gt[1, 1:3, 296:299] = 1
    return pred, gt


def check_upper_digits(lib, dev, spacing):
    """a side beyond 256: segm_edt_sq_long makes the planes; every pair of ranks of a few, the ends of the list included"""
    pred, gt = thin_pair()
    borders, counts = ops_raw.seg_regions(lib, K.dev_t(pred, dev), K.dev_t(gt, dev), M._table(((1,),), torch.device(dev)))
    edt = ops_raw.edt_sq_long(lib, borders, [(0, 0), (1, 0)], spacing)
    n = int(counts[3, 0]) + int(counts[4, 0])
    items = [(0, 0, 1), (1, 0, 0)]
    if spacing is None:
        assert int(edt[0, 0, 0, 299]) == 89401 > 1 << 16
    for ranks in ((0, n - 1), percentile_ranks(n), (n // 2, n // 3), (n, -1)):
        check_stats(lib, borders, edt, items, [0, 0], 1, [300.0, -1.0], [ranks])
    # each direction a group of its own, the second with ranks out of range; a group of one voxel
    check_stats(lib, borders, edt, items, [0, 1], 2, [-1.0, 295.0], [(0, int(counts[3, 0]) - 1), (int(counts[4, 0]), -7)])
    one = torch.zeros_like(borders)
    one[0, 1, 1, 17] = 4
    one[1, 0, 2, 250] = 4
    e1 = ops_raw.edt_sq_long(lib, one, [(0, 2), (1, 2)], spacing)
    _, got = check_stats(lib, one, e1, [(0, 2, 1)], [0], 1, [1e9], [(0, 0)])
    assert got[0] == 1.0 and got[3] == 1.0 and got[1] == got[2] == got[4 * W] == got[4 * W + 1] > 200.0
    check_stats(lib, one, e1, [(0, 2, 1)], [0], 1, [-1.0], [(1, -1)])


def check_thin_host(dev, spacing):
    """the same pair through the host functions: a side beyond 256 takes the box route and, the box being 300 long, segm_edt_sq_long"""
    pred, gt = thin_pair()
    tp, tg = K.dev_t(pred, dev), K.dev_t(gt, dev)
    got = M.case_report(tp, tg, spacing, ((1,),), tolerance=298.5)
    assert_none_near(pred, gt, spacing, 298.5)
    compare_report(got, S.case_report(pred, gt, spacing, ((1,),), tolerance=298.5), spacing)
    assert 0.0 < got["Surface Dice"][0] < 1.0
    assert bits(got["Hausdorff Distance 95"][0]) == bits(M.hd95(tp, tg, spacing)) and bits(got["Hausdorff Distance"][0]) == bits(M.hd(tp, tg, spacing))
    assert got["Avg. Surface Distance"][0] == M.asd(tp, tg, spacing)
    if spacing is None:
        assert got["Hausdorff Distance"][0] == 299.0


def scattered(shape, seed):
    """two byte volumes of sparse random bits and the transform of all 16 planes (bit 7 of volume 1 is never set)"""
    rng = np.random.RandomState(seed)
    v = np.zeros((2,) + tuple(shape), np.uint8)
    for b in range(8):
        v |= ((rng.rand(*v.shape) < 0.03).astype(np.uint8) << b)
    v[:, 0, 0, 0] |= 0x7f                                                   # no plane of bits 0 .. 6 is empty
    v[1] &= 0x7f
    return v


def check_layout(lib, dev, shape, spacing=None):
    """voxel counts that are no multiple of 16 or of the 4096 voxels of a workgroup's packet row, a second volume at an odd address,
    1 and 16 items, an item without a set bit"""
    v = scattered(shape, sum(shape))
    borders = K.dev_t(v, dev)
    planes = [(vol, b) for vol in range(2) for b in range(7)]
    edt = (ops_raw.edt_sq if max(shape) <= L.EDT_MAX_LINE else ops_raw.edt_sq_long)(lib, borders, planes, spacing)
    # 1 item
    check_stats(lib, borders, edt, [(1, 3, 2)], [0], 1, [1.5], [(0, 5)])
    # 16 items in 5 groups, one group without an item, the last item without a set bit (bit 7 of volume 1)
    items = [(i & 1, (i * 3) % 7, (i * 5) % 14) for i in range(15)] + [(1, 7, 0)]
    groups = [i % 3 for i in range(15)] + [4]
    host = [int(((v[a] >> b) & 1).sum()) for a, b, _ in items]
    assert host[15] == 0 and min(host[:15]) > 0
    n = [sum(c for c, g in zip(host, groups) if g == k) for k in range(5)]
    ranks = [percentile_ranks(n[0]), (0, n[1] - 1), (n[2] // 2, n[2]), (0, 0), (0, -1)]
    _, got = check_stats(lib, borders, edt, items, groups, 5, [0.0, 1.0, 2.5, -1.0] * 4, ranks)
    assert got[60:64] == [0.0] * 4 and all(math.isnan(x) for x in got[4 * W + 6:4 * W + 10])


# ---- host functions --------------------------------------------------------------------------------------------------------------
def live_regions(pred, gt, regions=R.BRATS_REGIONS):
    out = []
    for r, reg in enumerate(regions):
        p, g = R.region_mask(pred, reg), R.region_mask(gt, reg)
        if p.any() and g.any() and not p.all() and not g.all():
            out.append(r)
    return out


def check_report_equals_case_metrics(dev, case, spacing):
    """Dice and HD95 bit for bit on every live region, HD equal to `hd`"""
    pred, gt = K.LABEL_CASES[case]()
    tp, tg = K.dev_t(pred, dev), K.dev_t(gt, dev)
    rep = M.case_report(tp, tg, spacing, metrics=["Dice", "Hausdorff Distance 95", "Hausdorff Distance"])
    cm = M.case_metrics(tp, tg, spacing)
    live = live_regions(pred, gt)
    for r in live:
        a = K.dev_t(R.region_mask(pred, R.BRATS_REGIONS[r]).astype(np.uint8), dev)
        b = K.dev_t(R.region_mask(gt, R.BRATS_REGIONS[r]).astype(np.uint8), dev)
        print(case, spacing, r, rep["Dice"][r], rep["Hausdorff Distance 95"][r], rep["Hausdorff Distance"][r], cm[r].tolist())
        assert bits(rep["Dice"][r]) == bits(cm[r, 0])
        assert bits(rep["Hausdorff Distance 95"][r]) == bits(cm[r, 1])
        assert bits(rep["Hausdorff Distance"][r]) == bits(M.hd(a, b, spacing))
    for r in set(range(3)) - set(live):
        assert math.isnan(rep["Hausdorff Distance 95"][r]) and math.isnan(rep["Hausdorff Distance"][r])
    return live


def compare_report(got, want, spacing, names=S.ALL_NAMES):
    """count entries and the surface Dice exactly; the surface entries within 2^-23 ref (unit spacing: each d is a correctly rounded
    fp32 root of an exact integer, 2^-24 relative, and the margin is twice that) or 1e-6 ref (fp32 transform)"""
    unit = spacing is None or all(float(s) == 1.0 for s in spacing)
    tol = 2.0 ** -23 if unit else 1e-6
    for m in names:
        g, w = np.asarray(got[m], np.float64), np.asarray(want[m], np.float64)
        print(m, g.tolist(), "reference", w.tolist())
        assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), m
        ok = ~np.isnan(w)
        if m in S.SURFACE_NAMES:
            assert (np.abs(g[ok] - w[ok]) <= tol * w[ok]).all(), (m, g.tolist(), w.tolist())
        else:
            assert np.array_equal(g[ok], w[ok]), (m, g.tolist(), w.tolist())


def check_report_against_reference(dev, case, spacing):
    """the whole table, both settings of nan_for_nonexisting; asd / assd / nsd and a few of the named functions per live region"""
    tolerance = 1.0 if spacing is None else 1.1
    assert_tau_is_safe(case, spacing, (tolerance,))
    pred, gt = K.LABEL_CASES[case]()
    tp, tg = K.dev_t(pred, dev), K.dev_t(gt, dev)
    for nan in (True, False):
        got = M.case_report(tp, tg, spacing, tolerance=tolerance, nan_for_nonexisting=nan)
        assert list(got) == list(M.ALL_METRICS) and all(v.dtype == np.float64 and v.shape == (3,) for v in got.values())
        compare_report(got, S.case_report(pred, gt, spacing, tolerance=tolerance, nan_for_nonexisting=nan), spacing)
    unit = spacing is None or all(float(s) == 1.0 for s in spacing)
    tol = 2.0 ** -23 if unit else 1e-6
    for r in live_regions(pred, gt):
        a, b = R.region_mask(pred, R.BRATS_REGIONS[r]), R.region_mask(gt, R.BRATS_REGIONS[r])
        ta, tb = K.dev_t(a.astype(np.uint8), dev), K.dev_t(b.astype(np.uint8), dev)
        for have, want in ((M.asd(ta, tb, spacing), S.asd(a, b, spacing)), (M.asd(tb, ta, spacing), S.asd(b, a, spacing)),
                           (M.assd(ta, tb, spacing), S.assd(a, b, spacing))):
            assert abs(have - want) <= tol * want, (have, want)
        assert M.nsd(ta, tb, tolerance, spacing) == S.nsd(a, b, tolerance, spacing) == got["Surface Dice"][r]
        assert M.confusion(ta, tb) == S.confusion(a, b)
        assert M.avg_surface_distance(ta, tb, voxel_spacing=spacing) == M.asd(ta, tb, spacing) == got["Avg. Surface Distance"][r]
        assert M.hausdorff_distance_95(a, b, voxel_spacing=spacing) == M.hd95(ta, tb, spacing)
        want = S.count_metrics(a, b)
        assert M.dice(ta, tb) == want["Dice"] and M.jaccard(ta, tb) == want["Jaccard"] and M.recall(ta, tb) == want["Recall"]
        assert M.total_positives_test(ta, tb) == want["Total Positives Test"] and isinstance(M.total_positives_test(ta, tb), int)
        p, q = want["Precision"], want["Recall"]
        assert M.fscore(ta, tb) == 2 * p * q / (p + q)


def check_existence_rules(dev):
    """empty, full, 1 x 1 x 1 and a ground truth that fills the volume: NaN or 0 exactly where the reference's rules put them"""
    cases = {n: K.LABEL_CASES[n]() for n in ("1x1x1", "touches_every_face")}
    pred, gt = R.small_case((21, 30, 25), island=False)
    cases["all_empty"] = (np.zeros_like(pred), np.zeros_like(gt))
    cases["empty_pred"] = (np.zeros_like(pred), gt)
    cases["empty_gt"] = (pred, np.zeros_like(gt))
    cases["full_pred"] = (np.full_like(pred, 3), gt)
    for name, (p, g) in cases.items():
        for nan in (True, False):
            print(name, "nan_for_nonexisting", nan)
            got = M.case_report(K.dev_t(p, dev), K.dev_t(g, dev), nan_for_nonexisting=nan)
            compare_report(got, S.case_report(p, g, nan_for_nonexisting=nan), None)
    got = M.case_report(*[K.dev_t(a, dev) for a in cases["touches_every_face"]])
    assert math.isnan(got["Hausdorff Distance 95"][1]) and math.isnan(got["Surface Dice"][1]) and not math.isnan(got["Dice"][1])   # WT: gt full
    assert not math.isnan(got["Hausdorff Distance 95"][0])
    got = M.case_report(*[K.dev_t(a, dev) for a in cases["1x1x1"]], nan_for_nonexisting=False)
    assert all(got[m].tolist() == [0.0] * 3 for m in S.SURFACE_NAMES + ("Surface Dice",))
    empty, some = cases["all_empty"][0], (gt == 3)
    for fn in (M.asd, M.assd, lambda a, b: M.nsd(a, b, 1.0)):
        with pytest.raises(RuntimeError, match="The first supplied array does not contain any binary object."):
            fn(empty, some)
        with pytest.raises(RuntimeError, match="The second supplied array does not contain any binary object."):
            fn(some, empty)
    assert math.isnan(M.avg_surface_distance(empty, some)) and M.avg_surface_distance(empty, some, nan_for_nonexisting=False) == 0.0
    assert math.isnan(M.dice(empty, empty)) and M.dice(empty, empty, nan_for_nonexisting=False) == 0.0
    assert math.isnan(M.fscore(empty, some))


TEN_REGIONS = ((1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3), (3, 1), (2,), (1,))


def check_ten_regions(dev, spacing=None):
    pred, gt = K.LABEL_CASES["33x47x21"]()
    got = M.case_report(K.dev_t(pred, dev), K.dev_t(gt, dev), spacing, TEN_REGIONS, tolerance=2.5)
    assert all(v.shape == (10,) for v in got.values())
    compare_report(got, S.case_report(pred, gt, spacing, TEN_REGIONS, tolerance=2.5), spacing)
    assert bits(got["Avg. Surface Distance"][0]) == bits(got["Avg. Surface Distance"][9])          # the same region in both groups


def check_counts_only_launch_nothing_else(dev, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a kernel beyond segm_seg_regions was launched")
    for name in ("edt_sq", "edt_sq_long", "planes_bbox", "border_distances", "border_stats"):
        monkeypatch.setattr(ops_raw, name, refuse)
    pred, gt = K.LABEL_CASES["33x47x21"]()
    got = M.case_report(K.dev_t(pred, dev), K.dev_t(gt, dev), metrics=["Dice", "Jaccard"])
    want = S.case_report(pred, gt)
    assert list(got) == ["Dice", "Jaccard"]
    compare_report(got, want, None, names=("Dice", "Jaccard"))
    with pytest.raises(AssertionError):
        M.case_report(K.dev_t(pred, dev), K.dev_t(gt, dev), metrics=["Dice", "Avg. Surface Distance"])


def tiny_cases():
    a = R.small_case((20, 30, 25))
    b = R.small_case((21, 30, 25), island=False)
    b[0][b[0] == 3] = 1                                                  # the second prediction lacks ET
    return [a, b]


def check_evaluate_report(dev):
    cases = tiny_cases()
    spacings = [(1, 1, 1), ANISO[0]]
    per_case, mean = M.evaluate_report([(K.dev_t(p, dev), K.dev_t(g, dev), sp) for (p, g), sp in zip(cases, spacings)], tolerance=2.7)
    assert list(per_case) == list(M.ALL_METRICS) == list(mean)
    for i, ((p, g), sp) in enumerate(zip(cases, spacings)):
        assert_none_near(p, g, sp, 2.7)
        compare_report({m: v[i] for m, v in per_case.items()}, S.case_report(p, g, sp, tolerance=2.7), sp)
    for m in per_case:
        assert per_case[m].shape == (2, 3) and mean[m].shape == (3,)
        with np.errstate(all="ignore"):
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert np.array_equal(mean[m], np.nanmean(per_case[m], axis=0), equal_nan=True)
    assert math.isnan(per_case["Hausdorff Distance"][1, 2]) and mean["Hausdorff Distance"][2] == per_case["Hausdorff Distance"][0, 2]
    empty_cases, empty_mean = M.evaluate_report([], metrics=["Dice"])
    assert empty_cases["Dice"].shape == (0, 3) and np.isnan(empty_mean["Dice"]).all()


def assert_none_near(pred, gt, spacing, tau):
    if spacing is None or all(float(s) == 1.0 for s in spacing):
        return
    for reg in R.BRATS_REGIONS:
        a, b = R.region_mask(pred, reg), R.region_mask(gt, reg)
        if a.any() and b.any():
            assert not (np.abs(R.joined(a, b, spacing) - tau) <= 1e-5 * tau).any()


def check_report_tool(dev, tmp_path):
    """tools/compute_metrics.py --report: the JSON holds case_report per case and the mean; the default output does not change"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("compute_metrics_tool", os.path.join(ROOT, "tools", "compute_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    cases = tiny_cases()
    for i, (pred, gt) in enumerate(cases):
        np.save(tmp_path / "pred" / f"case{i}.npy", pred)
        np.save(tmp_path / "gt" / f"case{i}.npy", gt)
    plain = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt")])
    rep_file = tmp_path / "out" / "report.json"
    res = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--report", str(rep_file), "--tolerance", "2.5",
                     "--labels", "1,3"])
    assert plain.shape == (2, 3, 2) and res.shape == (2, 2, 2)
    rec = json.load(open(rep_file))
    assert rec["regions"] == [[1], [3]] and rec["tolerance"] == 2.5 and sorted(rec["cases"]) == ["case0.npy", "case1.npy"]
    per_case, mean = M.evaluate_report([(K.dev_t(p, dev), K.dev_t(g, dev)) for p, g in cases], ((1,), (3,)), tolerance=2.5)
    for m in M.ALL_METRICS:
        for i in range(2):
            want = [None if np.isnan(v) else float(v) for v in per_case[m][i]]
            assert rec["cases"][f"case{i}.npy"][m] == want, m
        assert rec["mean"][m] == [None if np.isnan(v) else float(v) for v in mean[m]]
    assert rec["cases"]["case1.npy"]["Hausdorff Distance"][1] is None


# ---- refusals (nothing is launched) and exports ------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    ok = torch.zeros(1, 4, 5, 6, dtype=torch.uint8, device=dev)
    e = torch.zeros(1, 4, 5, 6, dtype=torch.int32, device=dev)
    bad = [
        lambda: ops_raw.border_stats(lib, ok[0], e, [(0, 0, 0)], [0], 1),                           # no volume dimension
        lambda: ops_raw.border_stats(lib, ok, e.double(), [(0, 0, 0)], [0], 1),                      # dtype
        lambda: ops_raw.border_stats(lib, ok, e[:, :3], [(0, 0, 0)], [0], 1),                        # shapes differ
        lambda: ops_raw.border_stats(lib, ok, e, [], [], 1),                                          # no item
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)] * 17, [0] * 17, 1),
        lambda: ops_raw.border_stats(lib, ok, e, [(1, 0, 0)], [0], 1),                               # volume index
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 8, 0)], [0], 1),                               # bit index
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 1)], [0], 1),                               # plane index
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [1], 1),                               # group index
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [0], 0),
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [0], 17),
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [0, 0], 1),
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [0], 1, [1.0, 2.0]),                   # one tolerance per item
        lambda: ops_raw.border_stats(lib, ok, e, [(0, 0, 0)], [0], 1, None, [(0, 0), (0, 0)]),       # one pair of ranks per group
        lambda: M.asd(ok[0], ok[0, :3]),
        lambda: M.assd(ok[0, 0], ok[0, 0]),
        lambda: M.nsd(ok[0], ok[0], -1.0),
        lambda: M.case_report(ok[0], ok[0], metrics=["Dice", "Hausdorff"]),
        lambda: M.case_report(ok[0], ok[0], tolerance=float("nan")),
        lambda: M.case_report(ok[0], ok[0, :3]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the C entry itself, without launching
    dll = lib.dll
    assert dll.segm_border_stats(None) == -1
    a = L.BorderStatsArgs()
    assert dll.segm_border_stats(a) == -1                                                            # SEGM_E_NULL
    out = torch.zeros(6 * W, dtype=torch.float64, device=dev)
    nbytes = dll.segm_border_stats_workspace_bytes(120, 1)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=dev)

    def fresh():
        a = L.BorderStatsArgs()
        a.voxels, a.n_volumes, a.n_planes, a.n_items, a.n_groups = 120, 1, 1, 1, 1
        a.borders, a.edt, a.out, a.workspace, a.workspace_bytes = ok.data_ptr(), e.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes
        return a
    marker = out.clone()
    for field, value, status in (("voxels", 0, -2), ("voxels", L.METRICS_MAX_VOXELS + 1, -2), ("n_items", 0, -2), ("n_items", 17, -2),
                                 ("n_groups", 0, -2), ("n_groups", 17, -2), ("n_volumes", 0, -2), ("n_planes", 0, -2), ("fp32", 2, -4),
                                 ("borders", None, -1), ("edt", None, -1), ("out", None, -1),
                                 ("workspace", None, -6), ("workspace_bytes", nbytes - 1, -6), ("workspace", ws.data_ptr() + 4, -6)):
        a = fresh()
        setattr(a, field, value)
        assert dll.segm_border_stats(a) == status, (field, value)
    for field, value in (("border_volume", 1), ("border_volume", -1), ("border_bit", 8), ("edt_plane", 1), ("item_group", 1), ("item_group", -1)):
        a = fresh()
        getattr(a, field)[0] = value
        assert dll.segm_border_stats(a) == -2, (field, value)
    a = fresh()                                                                                       # 4 items of one group x 2^30 voxels
    a.voxels, a.n_items = L.METRICS_MAX_VOXELS, 4
    assert dll.segm_border_stats(a) == -2
    assert torch.equal(out.view(torch.int64), marker.view(torch.int64))                             # nothing was written
    assert dll.segm_border_stats(fresh()) == 0
    assert dll.segm_border_stats_workspace_bytes(0, 1) == 0 and dll.segm_border_stats_workspace_bytes(120, 0) == 0
    assert dll.segm_border_stats_workspace_bytes(120, 17) == 0 and dll.segm_border_stats_workspace_bytes(L.METRICS_MAX_VOXELS + 1, 1) == 0
    assert dll.segm_border_stats_workspace_bytes(4 * 4096 + 1, 3) - dll.segm_border_stats_workspace_bytes(4 * 4096, 3) == 3 * (8 + 12)


def check_exports(lib):
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10
    assert C_sizeof_args() == 8 + 6 * 4 + 4 * 64 + 64 + 256 + 6 * 8


def C_sizeof_args():
    import ctypes
    return ctypes.sizeof(L.BorderStatsArgs)
