"""Checks shared by tests/test_emu_edt_long.py (kernel sources on the CPU emulator) and tests/test_gpu_edt_long.py (the HIP library):
the linear-time distance transform `edt_sq_long`, `planes_bbox`, and the box route of segmamba_amd.metrics for volumes with a side
beyond 256.  Every function takes the loaded library and / or the device its tensors live on.  References: tests/metrics_ref.py
(numpy brute force on thin volumes, scipy.ndimage at label level)."""
import functools
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

INT_SENTINEL = K.INT_SENTINEL
ANISO = K.ANISO
NEW_EXPORTS = ("segm_edt_sq_long", "segm_edt_sq_long_workspace_bytes", "segm_planes_bbox")
# thin volumes (the brute-force reference is affordable) with a side on either side of 256, of 64 and of a workgroup's 256 columns:
# 300 and 2048 along x, 257 / 2048 along y, 258 / 2048 along z, 70 columns (no multiple of 64) x 600, one voxel
THIN_SHAPES = [(2, 3, 300), (3, 257, 5), (258, 2, 4), (1, 1, 2048), (2, 2048, 3), (2048, 1, 2), (2, 600, 70), (1, 1, 1)]
LONG_CASE = (24, 300, 280)


def have_scipy() -> bool:
    try:
        import scipy.ndimage  # noqa: F401
        return True
    except ImportError:
        return False


@functools.lru_cache(maxsize=None)
def planes_of(shape):
    return K.edt_planes(shape)


@functools.lru_cache(maxsize=None)
def ref_edt(shape, bit, spacing=None):
    """brute force of plane `bit` of planes_of(shape): int64 at unit spacing, fp64 otherwise; None for a plane without a set bit"""
    mask = ((planes_of(shape) >> bit) & 1).astype(bool)
    if not mask.any():
        return None
    ref = R.edt_sq(mask, spacing)
    ref.setflags(write=False)
    return ref


# ---- 1. int32, every voxel -----------------------------------------------------------------------------------------------------------
def check_int_exact(lib, dev, shape):
    v = planes_of(shape)
    planes = [(0, b) for b in range(7)]
    vol = K.dev_t(v[None], dev)
    e = ops_raw.edt_sq_long(lib, vol, planes)
    assert e.dtype == torch.int32 and tuple(e.shape) == (7,) + tuple(shape)
    got = e.cpu().numpy()
    assert not got[3].any()                                               # every voxel set
    assert (got[6] == INT_SENTINEL).all()                                 # nothing set
    for b in (0, 1, 2, 4, 5):
        ref = ref_edt(shape, b)
        if ref is None:
            assert (got[b] == INT_SENTINEL).all(), (shape, b)
            continue
        assert np.array_equal(got[b].astype(np.int64), ref), (shape, b)
        if have_scipy():
            assert np.array_equal(got[b].astype(np.int64), R.scipy_edt_sq_int((v >> b) & 1)), (shape, b)
    assert got[1].max() == sum(max(n - 2, 0) ** 2 for n in shape)          # the far island alone: distances span the volume
    assert torch.equal(e, ops_raw.edt_sq_long(lib, vol, planes))


# ---- 2. int32 against the brute-force kernel ----------------------------------------------------------------------------------------------
def check_int_equals_brute_kernel(lib, dev, shape):
    vol = K.dev_t(planes_of(shape)[None], dev)
    planes = [(0, b) for b in range(7)]
    assert torch.equal(ops_raw.edt_sq_long(lib, vol, planes), ops_raw.edt_sq(lib, vol, planes))


# ---- 3. fp32 ---------------------------------------------------------------------------------------------------------------------------
def check_fp32(lib, dev, shape, spacing):
    """within 1e-6 relative of fp64 brute force (the bound of the brute-force kernel: the values are rounded as it rounds them)"""
    v = planes_of(shape)
    bits = (0, 1, 2, 4, 6, 3)
    vol = K.dev_t(v[None], dev)
    e = ops_raw.edt_sq_long(lib, vol, [(0, b) for b in bits], spacing)
    assert e.dtype == torch.float32
    got = e.cpu().numpy().astype(np.float64)
    assert np.isposinf(got[4]).all() and not got[5].any()
    worst = 0.0
    for i, b in enumerate(bits[:4]):
        ref = ref_edt(shape, b, tuple(spacing))
        if ref is None:
            assert np.isposinf(got[i]).all()
            continue
        err = np.abs(got[i] - ref)
        worst = max(worst, float((err / np.maximum(ref, 1e-300)).max()))
        assert (err <= 1e-6 * ref).all(), (shape, spacing, b, worst)
    print("edt_sq_long", shape, spacing, "worst relative error against fp64 brute force", worst)
    assert torch.equal(e, ops_raw.edt_sq_long(lib, vol, [(0, b) for b in bits], spacing))


def check_fp32_near_brute_kernel(lib, dev, shape, spacing):
    vol = K.dev_t(planes_of(shape)[None], dev)
    planes = [(0, b) for b in range(7)]
    a = ops_raw.edt_sq_long(lib, vol, planes, spacing).cpu().numpy().astype(np.float64)
    b = ops_raw.edt_sq(lib, vol, planes, spacing).cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isinf(a), np.isinf(b))
    fin = np.isfinite(b)
    worst = float((np.abs(a[fin] - b[fin]) / np.maximum(b[fin], 1e-300)).max()) if fin.any() else 0.0
    print("edt_sq_long against edt_sq", shape, spacing, "worst relative difference", worst)
    assert (np.abs(a[fin] - b[fin]) <= 1e-6 * b[fin]).all(), (shape, spacing, worst)


# ---- 4. a workgroup reuses its stack area ------------------------------------------------------------------------------------------------
def check_stack_reuse(lib, dev):
    shape = (3, 300, 200)
    vol = K.dev_t(planes_of(shape)[None], dev)
    planes = [(0, b) for b in (0, 1, 2, 4, 5, 6)]
    for sp in (None, ANISO[0]):
        want = ops_raw.edt_sq_long(lib, vol, planes, sp)
        for cap in (1, 3):                                                # 18 batches in y and 1410 in z on one and on three workgroups
            assert torch.equal(ops_raw.edt_sq_long(lib, vol, planes, sp, max_workgroups=cap), want), (sp, cap)
        assert torch.equal(ops_raw.edt_sq_long(lib, vol, planes, sp, max_workgroups=1 << 20), want)      # above the default: no effect


# ---- 5. boxes --------------------------------------------------------------------------------------------------------------------------
def np_box(mask):
    idx = np.argwhere(mask)
    if len(idx) == 0:
        return [0x7f7f7f7f, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f, 0]
    lo, hi = idx.min(0), idx.max(0) + 1
    return [int(lo[0]), int(hi[0]), int(lo[1]), int(hi[1]), int(lo[2]), int(hi[2])]


def check_boxes(lib, dev, vols, items):
    got = ops_raw.planes_bbox(lib, K.dev_t(vols, dev), items)
    assert got.dtype == torch.int32 and tuple(got.shape) == (L.METRICS_MAX_PLANES, 6)
    got = got.cpu().numpy()
    for i, it in enumerate(items):
        mask = (vols[it[0]] >> it[1]) & 1
        if len(it) == 4:
            mask = mask | ((vols[it[2]] >> it[3]) & 1)
        assert got[i].tolist() == np_box(mask), (vols.shape, it, got[i].tolist(), np_box(mask))
    for i in range(len(items), L.METRICS_MAX_PLANES):                     # unused rows are marked empty
        assert got[i].tolist() == np_box(np.zeros((1, 1, 1), bool))
    assert np.array_equal(ops_raw.planes_bbox(lib, K.dev_t(vols, dev), items).cpu().numpy(), got)


def check_planes_bbox(lib, dev):
    # single voxels at each corner, one per bit; bit 7 of volume 1 everywhere; bit 6 nowhere
    for shape in [(5, 9, 48), (4, 7, 21), (3, 2, 2048), (6, 5, 1), (2, 3, 1040), (1, 1, 1)]:
        D, H, W = shape
        v = np.zeros((2,) + shape, dtype=np.uint8)
        corners = [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]
        for b, c in enumerate(corners[:6]):
            v[(0,) + c] |= 1 << b
        v[1] |= 1 << 7
        v[(1,) + corners[7]] |= 1
        v[1, D // 2, H // 2, W // 3] |= 2
        items = [(0, b) for b in range(7)] + [(1, 7), (1, 0), (1, 1), (0, 0, 1, 0), (0, 2, 1, 1), (0, 6, 1, 6), (1, 1, 0, 5), (0, 6, 1, 7)]
        check_boxes(lib, dev, v, items)
    # more rows than the grid has waves (4096): a wave takes several; set voxels away from the faces
    v = np.zeros((2, 70, 60, 32), dtype=np.uint8)
    v[0, 3, 59, 30] = v[0, 66, 2, 17] = v[1, 69, 31, 0] = 1
    check_boxes(lib, dev, v, [(0, 0), (0, 0, 1, 0), (1, 1)])
    # the borders of a label case, as the box route asks for them
    pred, gt = R.small_case((12, 40, 70))
    b = np.stack([R.border_planes(pred), R.border_planes(gt)])
    check_boxes(lib, dev, b, [(0, r, 1, r) for r in range(3)] + [(0, 1), (1, 2)])


# ---- 6 / 7. label level: the box route on a large volume ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case(shape, island, permuted):
    pred, gt = R.small_case(shape, island=island)
    if permuted:
        pred, gt = np.ascontiguousarray(pred.transpose(1, 2, 0)), np.ascontiguousarray(gt.transpose(1, 2, 0))
    return pred, gt


@functools.lru_cache(maxsize=None)
def scipy_case_reference(shape, island, permuted, spacing):
    """(Dice per region, scipy hd95 per region, per region the sorted joined distance list as fp32 at unit spacing else None)"""
    pred, gt = long_case(shape, island, permuted)
    sp = None if all(float(s) == 1.0 for s in spacing) else spacing
    dice, h95, lists = [], [], []
    for reg in R.BRATS_REGIONS:
        a, b = R.region_mask(pred, reg), R.region_mask(gt, reg)
        dice.append(R.dc(a, b))
        ab, ba = R.scipy_surface_distances(a, b, sp), R.scipy_surface_distances(b, a, sp)
        h95.append(float(np.percentile(np.hstack((ab, ba)), 95)))
        if sp is None:                                                    # the fp32-rounded roots of the exact integers
            ints = (np.rint(ab ** 2), np.rint(ba ** 2))
            lists.append(tuple(np.sort(np.sqrt(i)).astype(np.float32) for i in ints))
        else:
            lists.append(None)
    return dice, h95, lists


class CallCounter:
    """counts the calls of ops_raw functions that segmamba_amd.metrics makes"""

    def __init__(self, monkeypatch, names=("edt_sq", "edt_sq_long", "planes_bbox")):
        self.n = {k: 0 for k in names}
        for k in names:
            monkeypatch.setattr(ops_raw, k, self._wrap(k, getattr(ops_raw, k)))

    def reset(self):
        self.n = {k: 0 for k in self.n}

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.n[name] += 1
            return fn(*a, **kw)
        return counted


def check_label_route(dev, monkeypatch, shape, island, permuted, spacing, expect_long):
    pytest.importorskip("scipy.ndimage")
    pred, gt = long_case(shape, island, permuted)
    assert max(pred.shape) > L.EDT_MAX_LINE
    dice, h95, lists = scipy_case_reference(shape, island, permuted, tuple(spacing))
    calls = CallCounter(monkeypatch)
    tp, tg = K.dev_t(pred, dev), K.dev_t(gt, dev)
    got = M.case_metrics(tp, tg, spacing)
    print("case_metrics", pred.shape, spacing, got.tolist(), "reference", dice, h95, "calls", calls.n)
    assert got.shape == (3, 2)
    assert got[:, 0].tolist() == dice
    for r in range(3):
        assert abs(got[r, 1] - h95[r]) <= 1e-6 * h95[r], (r, got[r, 1], h95[r])
    assert calls.n["planes_bbox"] == 1 and calls.n["edt_sq"] + calls.n["edt_sq_long"] == 3
    if expect_long:
        assert calls.n["edt_sq_long"] > 0
    else:
        assert calls.n["edt_sq_long"] == 0 and calls.n["edt_sq"] == 3
    if lists[0] is not None:
        for r, reg in enumerate(R.BRATS_REGIONS):
            a, b = K.dev_t(R.region_mask(pred, reg).astype(np.uint8), dev), K.dev_t(R.region_mask(gt, reg).astype(np.uint8), dev)
            for x, y, want in ((a, b, lists[r][0]), (b, a, lists[r][1])):
                have = M.surface_distances(x, y).sort().values.cpu().numpy()
                assert have.dtype == np.float32 and np.array_equal(have, want), (reg, len(have), len(want))
    assert np.array_equal(M.case_metrics(tp, tg, spacing), got)


# ---- 8. the routes agree on small volumes ------------------------------------------------------------------------------------------------
def check_route_equality(dev, monkeypatch, case):
    pred, gt = K.LABEL_CASES[case]()
    tp, tg = K.dev_t(pred, dev), K.dev_t(gt, dev)
    monkeypatch.delenv("SEGM_EDT_LONG", raising=False)
    want_unit, want_aniso = M.case_metrics(tp, tg), M.case_metrics(tp, tg, ANISO[0])
    calls = CallCounter(monkeypatch)
    for mode in ("1", "box"):
        monkeypatch.setenv("SEGM_EDT_LONG", mode)
        calls.reset()
        unit, aniso = M.case_metrics(tp, tg), M.case_metrics(tp, tg, ANISO[0])
        print(case, "SEGM_EDT_LONG =", mode, unit.tolist(), aniso.tolist(), calls.n)
        assert np.array_equal(unit, want_unit), (case, mode)
        assert (np.abs(aniso - want_aniso) <= 1e-6 * np.abs(want_aniso)).all(), (case, mode)
        assert calls.n["planes_bbox"] == 2
        assert calls.n["edt_sq" if mode == "1" else "edt_sq_long"] == 0
    monkeypatch.setenv("SEGM_EDT_LONG", "sometimes")
    with pytest.raises(RuntimeError):
        M.case_metrics(tp, tg)


def check_empty_rules_under_switch(dev, monkeypatch, mode):
    monkeypatch.setenv("SEGM_EDT_LONG", mode)
    K.check_empty_rules(dev)


# ---- 9. distance_transform_edt ------------------------------------------------------------------------------------------------------------
def check_distance_transform_edt(dev):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = np.ones((3, 300, 5), dtype=bool)
    mask[1, 7, 2] = mask[0, 290, 4] = mask[2, 150:153, 0] = False
    for sp in (None, (1.5, 0.8, 1.0)):
        d = M.distance_transform_edt(K.dev_t(mask, dev), sp)
        assert d.dtype == torch.float32 and tuple(d.shape) == mask.shape
        want = ndi.distance_transform_edt(mask, sampling=None if sp is None else R.fp32_spacing(sp))
        got = d.cpu().numpy().astype(np.float64)
        assert not got[~mask].any() and np.allclose(got, want, rtol=1e-6, atol=0.0)
    with pytest.raises(RuntimeError):
        M.distance_transform_edt(torch.ones(1, 2049, 2, dtype=torch.uint8, device=dev))


# ---- 11. refusals (nothing is launched) and exports ----------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    big = L.EDT_LONG_MAX_LINE + 1
    bad = [
        lambda: ops_raw.edt_sq_long(lib, ok, [(0, 0)]),                                        # no volume dimension
        lambda: ops_raw.edt_sq_long(lib, ok[None].int(), [(0, 0)]),
        lambda: ops_raw.edt_sq_long(lib, ok[None].transpose(1, 3), [(0, 0)]),
        lambda: ops_raw.edt_sq_long(lib, ok[None], [(1, 0)]),                                  # volume index
        lambda: ops_raw.edt_sq_long(lib, ok[None], [(0, 8)]),                                  # bit index
        lambda: ops_raw.edt_sq_long(lib, ok[None], []),
        lambda: ops_raw.edt_sq_long(lib, ok[None], [(0, 0)] * 17),
        lambda: ops_raw.edt_sq_long(lib, ok[None], [(0, 0)], (1.0, 0.0, 1.0)),                 # spacing
        lambda: ops_raw.edt_sq_long(lib, ok[None], [(0, 0)], max_workgroups=-1),
        lambda: ops_raw.edt_sq_long(lib, torch.zeros(1, 2, 2, big, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.edt_sq_long(lib, torch.zeros(1, 2, big, 2, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.edt_sq_long(lib, torch.zeros(1, big, 2, 2, dtype=torch.uint8, device=dev), [(0, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok, [(0, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok[None].int(), [(0, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok[None].transpose(1, 3), [(0, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok[None], [(1, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok[None], [(0, 8)]),
        lambda: ops_raw.planes_bbox(lib, ok[None], [(0, 0, 1, 0)]),                            # second volume index
        lambda: ops_raw.planes_bbox(lib, ok[None], [(0, 0, 0)]),
        lambda: ops_raw.planes_bbox(lib, ok[None], []),
        lambda: ops_raw.planes_bbox(lib, ok[None], [(0, 0)] * 17),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the C entries
    assert lib.dll.segm_edt_sq_long(None) == -1 and lib.dll.segm_planes_bbox(None) == -1
    a = L.EdtSqLongArgs()
    assert lib.dll.segm_edt_sq_long(a) == -1                                                  # SEGM_E_NULL
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    a.volumes, a.out = buf.data_ptr(), buf.data_ptr()
    a.n_volumes, a.n_planes = 1, 1
    a.spacing_z = a.spacing_y = a.spacing_x = 1.0
    for shape in [(0, 1, 1), (1, 0, 1), (1, 1, 0), (big, 1, 1), (1, big, 1), (1, 1, big)]:
        a.depth, a.height, a.width = shape
        assert lib.dll.segm_edt_sq_long(a) == -2, shape                                       # SEGM_E_SHAPE
        assert lib.dll.segm_edt_sq_long_workspace_bytes(*shape, 1, 0) == 0
    a.depth, a.height, a.width = 2, 3, 4
    a.spacing_y = 2.0
    assert lib.dll.segm_edt_sq_long(a) == -4                                                  # int32 form with a non-unit spacing
    a.spacing_y = 1.0
    a.fp32 = 2
    assert lib.dll.segm_edt_sq_long(a) == -4
    a.fp32 = 0
    assert lib.dll.segm_edt_sq_long(a) == -6                                                  # SEGM_E_WORKSPACE: none given
    need = lib.dll.segm_edt_sq_long_workspace_bytes(2, 3, 4, 1, 0)
    assert need == 2 * 3 * 256 * 8                # y: two batches of three entries; z: one batch of two
    ws = torch.zeros(need // 8, dtype=torch.int64, device=dev)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need - 1
    assert lib.dll.segm_edt_sq_long(a) == -6                                                  # one byte too small
    a.max_workgroups = -1
    a.workspace_bytes = need
    assert lib.dll.segm_edt_sq_long(a) == -2
    assert lib.dll.segm_edt_sq_long_workspace_bytes(2, 3, 4, 0, 0) == 0 and lib.dll.segm_edt_sq_long_workspace_bytes(2, 3, 4, 1, 2) == 0
    # sized by the grid: 1024 workgroups of 512 entries x 256 threads x 8 bytes at 400 x 512 x 512, from two planes on
    assert lib.dll.segm_edt_sq_long_workspace_bytes(400, 512, 512, 2, 1) == lib.dll.segm_edt_sq_long_workspace_bytes(400, 512, 512, 16, 0) == 1 << 30
    b = L.PlanesBboxArgs()
    assert lib.dll.segm_planes_bbox(b) == -1
    b.volumes, b.boxes = buf.data_ptr(), buf.data_ptr()
    b.n_volumes, b.n_items = 1, 1
    assert lib.dll.segm_planes_bbox(b) == -2                                                  # sides 0
    b.depth, b.height, b.width = 2, 2, 2
    b.item_volume2[0] = -1
    b.item_bit[0] = 8
    assert lib.dll.segm_planes_bbox(b) == -2
    b.item_bit[0] = 0
    b.item_volume2[0] = 1
    assert lib.dll.segm_planes_bbox(b) == -2
    b.item_volume2[0] = -1
    b.n_items = 17
    assert lib.dll.segm_planes_bbox(b) == -2


def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert re.search(r"#define\s+SEGM_EDT_LONG_MAX_LINE\s+2048\b", header) and L.EDT_LONG_MAX_LINE == 2048
    assert re.search(r"#define\s+SEGM_EDT_MAX_LINE\s+256\b", header) and L.EDT_MAX_LINE == 256
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10


# ---- 12. the tool ------------------------------------------------------------------------------------------------------------------------
def check_tool(tmp_path):
    pytest.importorskip("scipy.ndimage")
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("compute_metrics_tool", os.path.join(root, "tools", "compute_metrics.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    (tmp_path / "pred").mkdir()
    (tmp_path / "gt").mkdir()
    want = []
    for i in range(2):
        pred, gt = R.small_case((20, 270, 30), shift=(1, -2 - i, 1))
        np.save(tmp_path / "pred" / f"case{i}.npy", pred)
        np.save(tmp_path / "gt" / f"case{i}.npy", gt)
        want.append([[R.dc(R.region_mask(pred, reg), R.region_mask(gt, reg)),
                      R.scipy_hd95(R.region_mask(pred, reg), R.region_mask(gt, reg))] for reg in R.BRATS_REGIONS])
    out = tmp_path / "result" / "metrics.npy"
    res = tool.main(["--pred", str(tmp_path / "pred"), "--gt", str(tmp_path / "gt"), "--out", str(out)])
    assert res.shape == (2, 3, 2) and np.array_equal(np.load(out), res)
    assert np.array_equal(res[:, :, 0], np.asarray(want)[:, :, 0])
    assert np.allclose(res, np.asarray(want), rtol=1e-6, atol=0.0)
