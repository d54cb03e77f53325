"""Checks shared by tests/test_emu_metrics.py (kernel sources on the CPU emulator) and tests/test_gpu_metrics.py (the HIP library):
every function takes the loaded library and the device its tensors live on.  References: tests/metrics_ref.py."""
import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw
from tests import metrics_ref as R

INT_SENTINEL = 2 ** 31 - 1
ANISO = ((1.5, 0.8, 1.0), (5.0, 0.9375, 0.9375))
NEW_EXPORTS = ("segm_seg_regions", "segm_seg_regions_workspace_bytes", "segm_edt_sq", "segm_border_distances",
               "segm_border_distances_workspace_bytes")


def slab_case():
    """a 1-thick slab"""
    gt = R.nested_labels((1, 30, 27), (0, 15, 13), (1, 9, 8), lobe=False)
    pred = R.nested_labels((1, 30, 27), (0, 14, 15), (1, 9, 8), scale=0.9, lobe=False)
    return pred, gt


LABEL_CASES = {
    "33x47x21": lambda: R.small_case((33, 47, 21)),
    "40x48x36": lambda: R.small_case((40, 48, 36), shift=(2, 1, -2)),
    "touches_every_face": lambda: R.full_case((9, 11, 13)),
    "1x1x1": lambda: (np.ones((1, 1, 1), np.uint8), np.full((1, 1, 1), 3, np.uint8)),
    "slab": slab_case,
    "wide_row": lambda: R.small_case((7, 9, 150), shift=(0, 1, -9)),
}


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def table(dev, regions=R.BRATS_REGIONS):
    return M._table(regions, torch.device(dev))


# ---- 1. borders and counts ------------------------------------------------------------------------------------------------------
def check_borders_and_counts(lib, dev, pred, gt):
    borders, counts = ops_raw.seg_regions(lib, dev_t(pred, dev), dev_t(gt, dev), table(dev))
    want = R.counts(pred, gt)
    got = counts.cpu().numpy()
    print("counts", got[:, :3].tolist(), "reference", want.tolist())
    assert np.array_equal(got[:, :3], want)
    assert not got[:, 3:].any()                                          # regions the table does not define
    assert np.array_equal(borders[0].cpu().numpy(), R.border_planes(pred))
    assert np.array_equal(borders[1].cpu().numpy(), R.border_planes(gt))
    b2, c2 = ops_raw.seg_regions(lib, dev_t(pred, dev), dev_t(gt, dev), table(dev))
    assert torch.equal(b2, borders) and torch.equal(c2, counts)


# ---- 2. distance transform ------------------------------------------------------------------------------------------------------
def edt_planes(shape):
    """one byte volume of bit planes: 0 a blob near the origin plus a 2^3 island in the opposite corner; 1 the island alone; 2 exactly one
    set voxel; 3 every voxel set; 4 a sparse lattice; 5 the WT border of a label case; 6 nothing set"""
    D, H, W = shape
    v = np.zeros(shape, dtype=np.uint8)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    isl = (z >= max(D - 2, 0)) & (y >= max(H - 2, 0)) & (x >= max(W - 2, 0))
    blob = (z * z * 4 + y * y + x * x * 2 <= 20) & ~isl
    v |= ((blob | isl).astype(np.uint8) << 0)
    v |= (isl.astype(np.uint8) << 1)
    v[D // 3, (2 * H) // 3, W // 4] |= 1 << 2
    v |= 1 << 3
    v |= (((x * 7 + y * 3 + z * 11) % 37 == 0).astype(np.uint8) << 4)
    if min(shape) >= 8:
        v |= (R.border(R.region_mask(R.small_case(shape)[1], (1, 2, 3))).astype(np.uint8) << 5)
    return v


EDT_SHAPES = [(33, 47, 21), (40, 48, 36), (5, 7, 150), (3, 130, 9), (140, 4, 5), (1, 1, 1), (1, 20, 70)]


def check_edt(lib, dev, shape, spacing=None):
    v = edt_planes(shape)
    planes = [(0, b) for b in range(7)]
    e = ops_raw.edt_sq(lib, dev_t(v[None], dev), planes, spacing)
    unit = spacing is None
    assert e.dtype == (torch.int32 if unit else torch.float32)
    got = e.cpu().numpy()
    assert not got[3].any()                                               # every voxel set: distance 0 everywhere
    assert (got[6] == (INT_SENTINEL if unit else np.inf)).all()           # nothing set: the sentinel
    for b in (0, 1, 2, 4, 5):
        mask = ((v >> b) & 1).astype(bool)
        if not mask.any():
            assert (got[b] == (INT_SENTINEL if unit else np.inf)).all()
            continue
        ref = R.edt_sq(mask, spacing)
        if unit:
            assert np.array_equal(got[b].astype(np.int64), ref), (shape, b)
        else:
            err = np.abs(got[b].astype(np.float64) - ref)
            worst = float((err / np.maximum(ref, 1e-300)).max())
            print("edt", shape, spacing, "plane", b, "worst relative error", worst)
            assert (err <= 1e-6 * ref).all(), (shape, b, worst)
    assert torch.equal(e, ops_raw.edt_sq(lib, dev_t(v[None], dev), planes, spacing))
    if unit:                                                              # the far island alone: distances span the whole volume
        assert got[1].max() == sum(max(n - 2, 0) ** 2 for n in shape)


def check_edt_against_scipy(lib, dev, shape):
    v = edt_planes(shape)
    e = ops_raw.edt_sq(lib, dev_t(v[None], dev), [(0, b) for b in (0, 1, 2, 4)]).cpu().numpy()
    for i, b in enumerate((0, 1, 2, 4)):
        assert np.array_equal(e[i].astype(np.int64), R.scipy_edt_sq_int((v >> b) & 1))
    pred, gt = R.small_case(shape)
    borders, _ = ops_raw.seg_regions(lib, dev_t(pred, dev), dev_t(gt, dev), table(dev))
    for r, reg in enumerate(R.BRATS_REGIONS):
        assert np.array_equal(((borders[1].cpu().numpy() >> r) & 1).astype(bool), R.scipy_border(R.region_mask(gt, reg)))


# ---- 3. dc / surface_distances / hd95 / hd ---------------------------------------------------------------------------------------
def check_binary_metrics(dev, pred, gt, spacings=(None,) + ANISO, with_scipy=False):
    for reg in R.BRATS_REGIONS:
        a, b = R.region_mask(pred, reg), R.region_mask(gt, reg)
        ta, tb = dev_t(a.astype(np.uint8), dev), dev_t(b.astype(np.uint8), dev)
        assert M.dc(ta, tb) == R.dc(a, b)
        if not (a.any() and b.any()):
            for fn in (M.surface_distances, M.hd95, M.hd):
                with pytest.raises(RuntimeError):
                    fn(ta, tb)
            continue
        for sp in spacings:
            ref_sd = R.surface_distances(a, b, sp)
            sd = M.surface_distances(ta, tb, sp)
            assert sd.dtype == torch.float32 and sd.shape == (len(ref_sd),)
            got = sd.cpu().numpy()
            if sp is None:                                                # same voxel order, correctly rounded roots of exact integers
                assert np.array_equal(got, ref_sd.astype(np.float32))
                both = torch.cat([sd, M.surface_distances(tb, ta)]).sort().values.cpu().numpy()
                assert np.array_equal(both, np.sort(R.joined(a, b)).astype(np.float32))
            else:
                assert np.allclose(got, ref_sd, rtol=1e-6, atol=0.0)
            for name, fn, ref in (("hd95", M.hd95, R.hd95), ("hd", M.hd, R.hd)):
                want, have = ref(a, b, sp), fn(ta, tb, sp)
                print(name, reg, sp, have, "reference", want)
                assert abs(have - want) <= 1e-6 * want, (name, reg, sp, have, want)
            if with_scipy:
                assert abs(M.hd95(ta, tb, sp) - R.scipy_hd95(a, b, sp)) <= 1e-6 * R.scipy_hd95(a, b, sp)
        assert M.hd95(ta, ta) == 0.0 and M.hd(tb, tb) == 0.0
        assert M.hd95(a, b) == M.hd95(ta, tb)                             # numpy arrays are accepted


# ---- 4. case_metrics / validation_dice / evaluate ----------------------------------------------------------------------------------
def check_case(dev, pred, gt, spacing=(1, 1, 1)):
    got = M.case_metrics(dev_t(pred, dev), dev_t(gt, dev), spacing)
    want = R.case_metrics(pred, gt, spacing)
    print("case_metrics", got.tolist(), "reference", want.tolist())
    assert got.shape == (3, 2)
    assert np.array_equal(got[:, 0], want[:, 0])
    assert (np.abs(got[:, 1] - want[:, 1]) <= 1e-6 * want[:, 1]).all()
    assert np.array_equal(M.validation_dice(dev_t(pred, dev), dev_t(gt, dev)), R.validation_dice(pred, gt))
    return got


def check_empty_rules(dev):
    pred, gt = R.small_case((21, 30, 25), island=False)
    full = check_case(dev, pred, gt)
    assert (full[:, 0] > 0).all() and (full[:, 1] != 50).all()
    no_et = pred.copy()
    no_et[no_et == 3] = 1                                                # the prediction lacks ET; TC and WT keep their voxels
    got = check_case(dev, no_et, gt)
    assert got[2].tolist() == [0.0, 50.0]
    assert np.array_equal(got[:2], full[:2])
    gt_no_et = gt.copy()
    gt_no_et[gt_no_et == 3] = 1                                          # both lack ET
    got = check_case(dev, no_et, gt_no_et)
    assert got[2].tolist() == [0.0, 50.0] and (got[:2, 1] != 50).all()
    assert M.validation_dice(dev_t(no_et, dev), dev_t(gt_no_et, dev))[2] == 1.0
    assert M.validation_dice(dev_t(no_et, dev), dev_t(gt, dev))[2] == 0.0
    empty = np.zeros_like(pred)
    assert M.case_metrics(empty, empty).tolist() == [[0.0, 50.0]] * 3
    assert M.validation_dice(empty, empty).tolist() == [1.0, 1.0, 1.0]
    assert M.dc(empty, empty) == 0.0
    for fn in (M.surface_distances, M.hd95, M.hd):
        with pytest.raises(RuntimeError):
            fn(empty, (gt == 3))
        with pytest.raises(RuntimeError):
            fn((gt == 3), empty)
    # a batch of label volumes is counted as one volume (3_train.py passes the whole batch)
    bp, bg = np.stack([pred, no_et]), np.stack([gt, gt_no_et])
    assert np.array_equal(M.validation_dice(dev_t(bp, dev), dev_t(bg, dev)), R.validation_dice(bp, bg))
    # evaluate: per-case results, mean and standard deviation
    cases = [(pred, gt), (no_et, gt, (1, 1, 1)), (dev_t(pred, dev), dev_t(gt, dev), (1.5, 0.8, 1.0))]
    res, mean, std = M.evaluate(cases)
    want = np.stack([R.case_metrics(pred, gt), R.case_metrics(no_et, gt), R.case_metrics(pred, gt, (1.5, 0.8, 1.0))])
    assert res.shape == (3, 3, 2) and np.allclose(res, want, rtol=1e-6, atol=0.0)
    assert np.array_equal(mean, res.mean(axis=0)) and np.array_equal(std, res.std(axis=0))
    # region_masks = convert_labels
    rm = M.region_masks(dev_t(gt, dev)).cpu().numpy()
    assert rm.dtype == np.float32 and np.array_equal(rm, np.stack([R.region_mask(gt, r) for r in R.BRATS_REGIONS]).astype(np.float32))
    # distance_transform_edt in scipy's meaning: 0 outside the mask, the distance to the nearest zero voxel inside
    mask = R.region_mask(gt, (1, 2, 3))
    for sp in (None, (1.5, 0.8, 1.0)):
        d = M.distance_transform_edt(dev_t(mask, dev), sp).cpu().numpy().astype(np.float64)
        want = np.sqrt(R.edt_sq(~mask, sp).astype(np.float64))
        assert d.dtype == np.float64 and not d[~mask].any() and np.allclose(d, want, rtol=1e-6, atol=0.0)


# ---- 5. refusals (nothing is launched) ----------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    tab = table(dev)
    bad = [
        lambda: ops_raw.seg_regions(lib, ok.int(), ok, tab),                                   # dtype
        lambda: ops_raw.seg_regions(lib, ok, ok.float(), tab),
        lambda: ops_raw.seg_regions(lib, ok.transpose(0, 2), ok.transpose(0, 2), tab),         # not contiguous
        lambda: ops_raw.seg_regions(lib, ok, ok[:3], tab),                                     # shapes differ
        lambda: ops_raw.seg_regions(lib, ok, ok, tab[:100]),                                   # table length
        lambda: ops_raw.seg_regions(lib, ok, ok, tab.int()),
        lambda: ops_raw.seg_regions(lib, ok[0], ok[0], tab),                                   # 2-D
        lambda: ops_raw.edt_sq(lib, ok, [(0, 0)]),                                             # no volume dimension
        lambda: ops_raw.edt_sq(lib, ok[None].int(), [(0, 0)]),
        lambda: ops_raw.edt_sq(lib, ok[None].transpose(1, 3), [(0, 0)]),
        lambda: ops_raw.edt_sq(lib, ok[None], [(1, 0)]),                                       # volume index
        lambda: ops_raw.edt_sq(lib, ok[None], [(0, 8)]),                                       # bit index
        lambda: ops_raw.edt_sq(lib, ok[None], []),
        lambda: ops_raw.edt_sq(lib, ok[None], [(0, 0)] * 17),
        lambda: ops_raw.edt_sq(lib, ok[None], [(0, 0)], (1.0, 0.0, 1.0)),                      # spacing
        lambda: ops_raw.edt_sq(lib, torch.zeros(1, 2, 2, L.EDT_MAX_LINE + 1, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.edt_sq(lib, torch.zeros(1, 2, L.EDT_MAX_LINE + 1, 2, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.edt_sq(lib, torch.zeros(1, L.EDT_MAX_LINE + 1, 2, 2, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.border_distances(lib, ok[None], torch.zeros(1, 4, 5, 6, device=dev).double(), [(0, 0, 0)], [0]),
        lambda: ops_raw.border_distances(lib, ok[None], torch.zeros(1, 4, 5, 7, dtype=torch.int32, device=dev), [(0, 0, 0)], [0]),
        lambda: ops_raw.border_distances(lib, ok[None], torch.zeros(1, 4, 5, 6, dtype=torch.int32, device=dev), [(0, 0, 1)], [0]),
        lambda: ops_raw.border_distances(lib, ok[None], torch.zeros(1, 4, 5, 6, dtype=torch.int32, device=dev), [(0, 0, 0)], [1, 2]),
        lambda: M.dc(ok, ok[:3]),
        lambda: M.hd95(ok[0], ok[0]),
        lambda: M.case_metrics(ok, ok, regions=[(1,)] * 9),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the C entry itself reports a line beyond the staged length, and bad arguments, without launching
    a = L.EdtSqArgs()
    assert lib.dll.segm_edt_sq(a) == -1                                                       # SEGM_E_NULL
    buf = torch.zeros(16, dtype=torch.uint8, device=dev)
    a.volumes, a.out = buf.data_ptr(), buf.data_ptr()
    a.depth, a.height, a.width, a.n_volumes, a.n_planes = 1, 1, L.EDT_MAX_LINE + 1, 1, 1
    a.spacing_z = a.spacing_y = a.spacing_x = 1.0
    assert lib.dll.segm_edt_sq(a) == -2                                                       # SEGM_E_SHAPE
    a.width = 2
    a.spacing_y = 2.0
    assert lib.dll.segm_edt_sq(a) == -4                                                       # int32 form with a non-unit spacing
    s = L.SegRegionsArgs()
    assert lib.dll.segm_seg_regions(s) == -1
    s.pred = s.gt = s.table = s.border_pred = s.border_gt = s.counts = buf.data_ptr()
    assert lib.dll.segm_seg_regions(s) == -2
    s.depth = s.height = s.width = 2
    assert lib.dll.segm_seg_regions(s) == -6                                                  # SEGM_E_WORKSPACE
    b = L.BorderDistancesArgs()
    assert lib.dll.segm_border_distances(b) == -1
    assert lib.dll.segm_edt_sq(None) == -1 and lib.dll.segm_seg_regions(None) == -1 and lib.dll.segm_border_distances(None) == -1
    assert lib.dll.segm_seg_regions_workspace_bytes(0) == 0 and lib.dll.segm_seg_regions_workspace_bytes(4097) == 2 * 40 * 4
    assert lib.dll.segm_border_distances_workspace_bytes(4096, 3) == 3 * 4


# ---- 7. exports --------------------------------------------------------------------------------------------------------------------
def check_exports(lib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "segmamba_hip.h")).read()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10


# ---- 6. brute force on the device (plain ATen), for the cases at BraTS size --------------------------------------------------------
def torch_min_sq_dist(points, targets, spacing, dev, budget=1 << 26):
    """tests/metrics_ref.min_sq_dist with torch on `dev`: integer coordinates, int32 arithmetic at unit spacing, fp64 (spacing as rounded
    to fp32) otherwise; chunked so that a chunk holds at most `budget` pairs"""
    unit = spacing is None or all(float(s) == 1.0 for s in spacing)
    p = torch.as_tensor(np.asarray(points), dtype=torch.int32, device=dev)
    t = torch.as_tensor(np.asarray(targets), dtype=torch.int32, device=dev)
    sp = None if unit else torch.as_tensor(R.fp32_spacing(spacing), dtype=torch.float64, device=dev)
    out = []
    chunk = max(1, budget // max(1, len(t)))
    for i in range(0, len(p), chunk):
        acc = None
        for ax in range(3):
            d = p[i:i + chunk, ax, None] - t[None, :, ax]
            d = d * d if unit else (d.double() * sp[ax]) ** 2
            acc = d if acc is None else acc + d
        out.append(acc.min(dim=1).values)
    return torch.cat(out).cpu().numpy()
