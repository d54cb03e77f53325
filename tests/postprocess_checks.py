"""Checks shared by tests/test_emu_postprocess.py (kernel sources on the CPU emulator) and tests/test_gpu_postprocess.py (the HIP
library): every function takes the loaded library and the device its tensors live on.  References: tests/postprocess_ref.py.
Everything about components, sizes, selection, hole filling and numbering is exact (array_equal)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP
from tests import metrics_ref as MR
from tests import postprocess_ref as R

NEW_EXPORTS = ("segm_resample_argmax", "segm_ccl_roots", "segm_ccl_roots_workspace_bytes", "segm_ccl_sizes", "segm_ccl_select",
               "segm_ccl_select_workspace_bytes")


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _small(shape, which, **kw):
    pred, gt = MR.small_case(shape, **kw)
    return {"pred_wt": MR.region_mask(pred, (1, 2, 3)), "gt_wt": MR.region_mask(gt, (1, 2, 3)), "pred_shell": pred == 2,
            "pred_tc": MR.region_mask(pred, (1, 3)), "pred_et": pred == 3}[which].astype(np.uint8)


MASK_CASES = {
    "33x47x21_pred_wt": lambda: _small((33, 47, 21), "pred_wt"),
    "33x47x21_gt_wt": lambda: _small((33, 47, 21), "gt_wt"),
    "33x47x21_pred_shell": lambda: _small((33, 47, 21), "pred_shell"),
    "40x48x36_pred_tc": lambda: _small((40, 48, 36), "pred_tc", shift=(2, 1, -2)),
    "40x48x36_pred_et": lambda: _small((40, 48, 36), "pred_et", shift=(2, 1, -2)),
    "checkerboard": lambda: R.checkerboard((9, 10, 67)),
    "cubes_edge": lambda: R.cubes((8, 9, 10), "edge"),
    "cubes_corner": lambda: R.cubes((8, 9, 10), "corner"),
    "crossing_17x70x131": R.crossing,
    "empty": lambda: np.zeros((5, 6, 7), np.uint8),
    "full": lambda: np.ones((5, 9, 70), np.uint8),
    "1x1x1": lambda: np.ones((1, 1, 1), np.uint8),
    "slab": lambda: (MR.nested_labels((1, 30, 27), (0, 15, 13), (1, 9, 8), lobe=False) == 2).astype(np.uint8),
    "tie": R.tie_case,
}
# conditions on the inputs (figures computed with scipy.ndimage.label when the cases were written): name -> component sizes in memory order
KNOWN_SIZES = {"33x47x21_pred_wt": [8, 3631], "33x47x21_gt_wt": [4522, 18], "33x47x21_pred_shell": [2672], "cubes_edge": [27, 27],
               "cubes_corner": [27, 27], "full": [5 * 9 * 70], "1x1x1": [1], "empty": [], "tie": [12, 5, 12]}


# ---- 1. roots, sizes, numbering ------------------------------------------------------------------------------------------------------
def check_components(lib, dev, mask, reference=R.roots_propagate, with_scipy=False):
    """roots / sizes / touches / numbering of the mask AND of its complement against the restatement; two calls bit-equal"""
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    for invert in (False, True):
        want = reference(m == 0) if invert else reference(m)
        roots = ops_raw.ccl_roots(lib, dev_t(m, dev), invert=invert)
        assert roots.dtype == torch.int32 and tuple(roots.shape) == m.shape
        got = roots.cpu().numpy()
        print("components", m.shape, "invert", invert, "roots", int((want == np.arange(m.size).reshape(m.shape)).sum()))
        assert np.array_equal(got, want)
        assert torch.equal(roots, ops_raw.ccl_roots(lib, dev_t(m, dev), invert=invert))
        sizes, touches = ops_raw.ccl_sizes(lib, roots)
        ws, wt = R.sizes_from_roots(want)
        assert sizes.dtype == torch.int32 and np.array_equal(sizes.cpu().numpy(), ws)
        assert touches.dtype == torch.uint8 and np.array_equal(touches.cpu().numpy(), wt)
        _, info = ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST)
        n, root, size = info.tolist()
        assert n == int((ws > 0).sum()) and size == int(ws.max())
        assert root == (int(np.flatnonzero(ws.reshape(-1) == ws.max())[-1]) if n else -1)
    # bit planes: the same mask as bit 5 of a volume with other bits set gives the same roots
    noise = ((np.arange(m.size).reshape(m.shape) * 7) % 32).astype(np.uint8)
    planes = (noise | (m << 5)).astype(np.uint8)
    assert np.array_equal(ops_raw.ccl_roots(lib, dev_t(planes, dev), bit=5).cpu().numpy(), reference(m))
    labels, num = PP.label(dev_t(m, dev))
    wl, wn = R.number(reference(m))
    assert labels.dtype == torch.int32 and num == wn and np.array_equal(labels.cpu().numpy(), wl)
    if with_scipy:
        sl, sn = R.scipy_label(m)
        assert num == sn and np.array_equal(labels.cpu().numpy(), sl)


def check_known_sizes(dev, name):
    m = MASK_CASES[name]()
    roots = PP.component_roots(dev_t(m, dev)).cpu().numpy()
    sizes, _ = R.sizes_from_roots(roots)
    got = sizes.reshape(-1)[sizes.reshape(-1) > 0].tolist()
    print(name, "component sizes", got)
    assert got == KNOWN_SIZES[name]
    n, big = PP.component_summary(dev_t(m, dev))
    assert n == len(got) and big == (max(got) if got else 0)


# ---- 2. selection and hole filling ---------------------------------------------------------------------------------------------------
def check_selection(dev, mask, with_scipy=False):
    m = np.ascontiguousarray(mask, dtype=np.uint8)
    t = dev_t(m, dev)
    big = PP.largest_connected_domain(t)
    assert big.dtype == torch.uint8 and np.array_equal(big.cpu().numpy(), R.largest_connected_domain(m))
    assert torch.equal(big, PP.largest_connected_domain(t))
    filled = PP.binary_fill_holes(t)
    assert filled.dtype == torch.uint8 and np.array_equal(filled.cpu().numpy(), R.fill_holes(m))
    assert np.array_equal(PP.binary_fill_holes(m).cpu().numpy(), filled.cpu().numpy())        # numpy arrays are accepted
    sizes = R.sizes_from_roots(R.roots_propagate(m))[0]
    for n in sorted({1, int(sizes.max()), int(sizes.max()) + 1} | {int(s) for s in sizes[sizes > 0][:2]} | {int(s) + 1 for s in sizes[sizes > 0][:2]}):
        assert np.array_equal(PP.remove_small_components(t, n).cpu().numpy(), R.min_size(m, n)), n
    if with_scipy:
        assert np.array_equal(filled.cpu().numpy(), R.scipy_fill(m))
        if m.any():
            lab, num = R.scipy_label(m)
            cnt = np.bincount(lab.reshape(-1))[1:]
            if (cnt == cnt.max()).sum() == 1:                             # ties are stated against the rule only
                assert np.array_equal(big.cpu().numpy(), R.scipy_fill(lab == 1 + int(cnt.argmax())))


def check_holes(dev, name, with_scipy=False):
    m, added = R.hole_cases()[name]
    filled = PP.binary_fill_holes(dev_t(m, dev)).cpu().numpy()
    print(name, "filling adds", int(filled.sum()) - int(m.sum()), "expected", added)
    assert np.array_equal(filled, R.fill_holes(m))
    assert int(filled.sum()) - int(m.sum()) == added
    assert not (m & ~filled).any()
    if with_scipy:
        assert np.array_equal(filled, R.scipy_fill(m))


def check_tie_and_boundaries(dev):
    m = R.tie_case()
    t = dev_t(m, dev)
    want = np.zeros_like(m)
    want[4, 5:7, 60:66] = 1                                               # of the two 12-voxel components the later one
    assert np.array_equal(PP.largest_connected_domain(t).cpu().numpy(), want)
    for n, kept in ((5, 29), (6, 24), (12, 24), (13, 0)):                 # min_size - 1 / min_size at both component sizes
        assert int(PP.remove_small_components(t, n).sum().item()) == kept, n
    empty = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    assert not PP.largest_connected_domain(empty).any()                   # the reference raises IndexError here
    assert not PP.binary_fill_holes(empty).any() and PP.label(empty)[1] == 0
    assert PP.component_summary(empty) == (0, 0)


def check_postprocess_labels(dev, labels):
    t = dev_t(labels, dev)
    for keep, fill in (("largest", True), ("largest", False), (10, True)):
        got = PP.postprocess_labels(t, keep=keep, fill_holes=fill)
        assert got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), R.postprocess_labels(labels, keep=keep, fill=fill)), (keep, fill)
    assert np.array_equal(t.cpu().numpy(), labels)                        # the input is not modified


# ---- 3. refusals and exports -----------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    roots = ops_raw.ccl_roots(lib, ok)
    sizes, touches = ops_raw.ccl_sizes(lib, roots)
    logits = torch.zeros(4, 4, 5, 6, device=dev)
    other = "cpu" if str(dev) != "cpu" else None
    bad = [
        lambda: ops_raw.ccl_roots(lib, ok.int()),                                              # dtype
        lambda: ops_raw.ccl_roots(lib, ok[0]),                                                 # 2-D
        lambda: ops_raw.ccl_roots(lib, ok.transpose(0, 2)),                                    # not contiguous
        lambda: ops_raw.ccl_roots(lib, ok, bit=8),
        lambda: ops_raw.ccl_roots(lib, ok, out=torch.zeros(4, 5, 6, dtype=torch.int64, device=dev)),
        lambda: ops_raw.ccl_roots(lib, ok, out=torch.zeros(4, 5, 7, dtype=torch.int32, device=dev)),
        lambda: ops_raw.ccl_roots(lib, ok, out=torch.zeros(4, 6, 5, dtype=torch.int32, device=dev).transpose(1, 2)),
        lambda: ops_raw.ccl_sizes(lib, roots.long()),
        lambda: ops_raw.ccl_sizes(lib, roots[0]),
        lambda: ops_raw.ccl_select(lib, roots, sizes.long(), L.CCL_LARGEST),
        lambda: ops_raw.ccl_select(lib, roots, sizes[:3], L.CCL_LARGEST),
        lambda: ops_raw.ccl_select(lib, roots, sizes, 3),                                      # mode
        lambda: ops_raw.ccl_select(lib, roots, sizes, L.CCL_FILL),                             # no touches
        lambda: ops_raw.ccl_select(lib, roots, sizes, L.CCL_MIN_SIZE, min_size=-1),
        lambda: ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST, out=torch.zeros(4, 5, 6, dtype=torch.int32, device=dev)),
        lambda: ops_raw.resample_argmax(lib, logits.double()),
        lambda: ops_raw.resample_argmax(lib, logits[0]),                                       # no class dimension
        lambda: ops_raw.resample_argmax(lib, torch.zeros(9, 2, 2, 2, device=dev)),             # more than 8 classes
        lambda: ops_raw.resample_argmax(lib, logits.transpose(2, 3)),                          # no unit stride along w
        lambda: ops_raw.resample_argmax(lib, logits, (4, 5, 6), (1, 0, 0), (4, 5, 6)),         # the box leaves the output
        lambda: ops_raw.resample_argmax(lib, logits, (4, 5, 6), (0, 0, 0), (4, 0, 6)),
        lambda: ops_raw.resample_argmax(lib, logits, table=torch.zeros(100, dtype=torch.uint8, device=dev)),
        lambda: ops_raw.resample_argmax(lib, logits, out=torch.zeros(4, 5, 6, dtype=torch.int32, device=dev)),
        lambda: ops_raw.resample_argmax(lib, logits, out=torch.zeros(4, 5, 7, dtype=torch.uint8, device=dev)),
        lambda: PP.label(ok[0]),
        lambda: PP.largest_connected_domain(ok[None]),
        lambda: PP.labels_from_logits(logits[0]),
        lambda: PP.labels_from_logits(logits, {"shape_after_cropping_before_resample": [4, 5, 6], "shape_before_cropping": [9, 9, 9],
                                               "bbox_used_for_cropping": [[0, 4], [0, 5], [0, 7]]}),
    ]
    if other is not None:                                                                      # mismatching devices
        bad += [lambda: ops_raw.ccl_roots(lib, ok, out=torch.zeros(4, 5, 6, dtype=torch.int32, device=other)),
                lambda: ops_raw.ccl_select(lib, roots, sizes.to(other), L.CCL_LARGEST),
                lambda: ops_raw.resample_argmax(lib, logits, table=torch.zeros(256, dtype=torch.uint8, device=other))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the C entries: null pointers, a volume of 2^31 voxels (by shape arithmetic only: nothing is touched), a too-small workspace
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    dll = lib.dll
    assert dll.segm_ccl_roots(None) == -1 and dll.segm_ccl_sizes(None) == -1 and dll.segm_ccl_select(None) == -1
    assert dll.segm_resample_argmax(None) == -1
    a = L.CclRootsArgs()
    assert dll.segm_ccl_roots(a) == -1                                                         # SEGM_E_NULL
    a.volume = a.roots = buf.data_ptr()
    assert dll.segm_ccl_roots(a) == -2                                                         # SEGM_E_SHAPE: no size
    a.depth, a.height, a.width, a.bit = 2048, 1024, 1024, -1
    assert dll.segm_ccl_roots(a) == -2                                                         # 2^31 voxels
    a.depth, a.height, a.width = 65536, 65536, 1
    assert dll.segm_ccl_roots(a) == -2
    a.depth, a.height, a.width = 2, 2, 2
    a.bit = 9
    assert dll.segm_ccl_roots(a) == -2
    a.bit = 0
    assert dll.segm_ccl_roots(a) == -6                                                         # SEGM_E_WORKSPACE: none
    a.workspace, a.workspace_bytes = buf.data_ptr(), 31
    assert dll.segm_ccl_roots(a) == -6                                                         # one byte short
    assert dll.segm_ccl_roots_workspace_bytes(8) == 32 and dll.segm_ccl_roots_workspace_bytes(0) == 0
    assert dll.segm_ccl_roots_workspace_bytes(2 ** 31) == 0 and dll.segm_ccl_roots_workspace_bytes(2 ** 31 - 1) == 4 * (2 ** 31 - 1)
    s = L.CclSizesArgs()
    assert dll.segm_ccl_sizes(s) == -1
    s.roots = s.sizes = s.touches = buf.data_ptr()
    assert dll.segm_ccl_sizes(s) == -2
    c = L.CclSelectArgs()
    assert dll.segm_ccl_select(c) == -1
    c.roots = c.sizes = c.out = c.info = buf.data_ptr()
    c.mode = 7
    assert dll.segm_ccl_select(c) == -2
    c.mode = L.CCL_FILL
    assert dll.segm_ccl_select(c) == -1                                                        # touches required
    c.mode = L.CCL_LARGEST
    assert dll.segm_ccl_select(c) == -2
    c.depth, c.height, c.width = 2, 2, 2
    assert dll.segm_ccl_select(c) == -6
    assert dll.segm_ccl_select_workspace_bytes(4096) == 16 and dll.segm_ccl_select_workspace_bytes(4097) == 32
    assert dll.segm_ccl_select_workspace_bytes(2 ** 31) == 0
    r = L.ResampleArgmaxArgs()
    assert dll.segm_resample_argmax(r) == -1
    r.logits = r.labels = buf.data_ptr()
    assert dll.segm_resample_argmax(r) == -2                                                   # no classes
    r.classes = 4
    r.in_depth = r.in_height = r.in_width = r.box_depth = r.box_height = r.box_width = r.out_depth = r.out_height = r.out_width = 2
    r.stride_c, r.stride_z, r.stride_y = 8, 4, 2
    r.dtype = 5
    assert dll.segm_resample_argmax(r) == -4                                                   # SEGM_E_DTYPE
    r.dtype = 0
    r.box_x = 1
    assert dll.segm_resample_argmax(r) == -2                                                   # the box leaves the output
    r.box_x = 0
    r.regions = buf.data_ptr()
    assert dll.segm_resample_argmax(r) == -1                                                   # regions without a table
    r.regions = None
    r.logits = buf.data_ptr() + 2
    assert dll.segm_resample_argmax(r) == -2                                                   # fp32 logits on a 2-byte boundary
    r.logits = buf.data_ptr()
    r.out_depth, r.out_height, r.out_width = 2048, 1024, 1024
    assert dll.segm_resample_argmax(r) == -2


def check_exports(lib):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", open(os.path.join(root, "include", "segmamba_hip.h")).read()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10


# ---- 4. the label map ------------------------------------------------------------------------------------------------------------------
def check_argmax_identity(lib, dev, shape=(9, 11, 24)):
    """integer-valued logits with ties: exactly the host argmax (first index wins), for three dtypes, contiguous and strided, on the
    16-byte path (w % 4 == 0) and off it"""
    for shp in (shape, (shape[0], shape[1], shape[2] + 3)):
        v = R.tie_logits(shp)
        want = torch.from_numpy(v).argmax(0).to(torch.uint8).numpy()
        ties = int(((v == v.max(0)).sum(0) > 1).sum())
        assert ties > 0.2 * want.size                                       # a condition on the input: ties are common
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            t = dev_t(v, dev).to(dt)                                        # small integers: exact in every type
            assert np.array_equal(ops_raw.resample_argmax(lib, t).cpu().numpy(), want), (shp, dt)
            wide = torch.zeros((6,) + tuple(shp[:2]) + (shp[2] + 5,), dtype=dt, device=dev)
            wide[1:5, :, :, 2:2 + shp[2]] = t
            view = wide[1:5, :, :, 2:2 + shp[2]]                            # a channel slice of a larger tensor, rows not on 16 bytes
            assert not view.is_contiguous()
            assert np.array_equal(ops_raw.resample_argmax(lib, view).cpu().numpy(), want), (shp, dt, "strided")
        two = ops_raw.resample_argmax(lib, dev_t(v, dev)[:2])                # two classes
        assert np.array_equal(two.cpu().numpy(), torch.from_numpy(v[:2]).argmax(0).to(torch.uint8).numpy())
        one = ops_raw.resample_argmax(lib, dev_t(v, dev)[:1])
        assert not one.any()


def check_paste_and_regions(lib, dev):
    v = R.tie_logits((6, 7, 12))
    lab = torch.from_numpy(v).argmax(0).to(torch.uint8).numpy()
    t = dev_t(v, dev)
    tab = M._table(MR.BRATS_REGIONS, torch.device(dev))
    tab_np = tab.cpu().numpy()
    for out_shape, start in (((10, 12, 20), (2, 3, 4)), ((10, 12, 21), (1, 2, 5)), ((6, 9, 12), (0, 2, 0)), ((8, 7, 14), (2, 0, 2)),
                             ((6, 7, 12), (0, 0, 0))):
        got, planes = ops_raw.resample_argmax(lib, t, out_shape, start, (6, 7, 12), table=tab)
        want = R.paste(lab, out_shape, start)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), (out_shape, start)
        assert planes.dtype == torch.uint8 and np.array_equal(planes.cpu().numpy(), tab_np[want]), (out_shape, start)
        buf = torch.full(out_shape, 77, dtype=torch.uint8, device=dev)      # a caller's buffer is overwritten everywhere
        assert ops_raw.resample_argmax(lib, t, out_shape, start, (6, 7, 12), out=buf) is buf
        assert np.array_equal(buf.cpu().numpy(), want)
    labels, planes = PP.labels_from_logits(t, regions=MR.BRATS_REGIONS)
    assert np.array_equal(labels.cpu().numpy(), lab) and np.array_equal(planes.cpu().numpy(), tab_np[lab])
    assert np.array_equal(PP.labels_from_logits(v[None]).cpu().numpy(), lab)   # numpy, with the batch dimension of 1


def band_compare(got, logits, box_shape, what):
    """the band rule: `got` must equal the fp64 restatement's label wherever the fp64 margin between the best and the second-best class
    exceeds 4 x max |ATen fp32 F.interpolate - fp64 restatement| on this input; inside the band only the two best classes are allowed;
    at most 1e-3 of the voxels may lie inside the band (a condition on the input)"""
    v = np.asarray(logits, dtype=np.float32)
    ref = R.resample_fp64(v, box_shape)
    aten = F.interpolate(torch.from_numpy(v)[None], size=tuple(box_shape), mode="trilinear", align_corners=False)[0].numpy()
    band = 4.0 * float(np.abs(aten.astype(np.float64) - ref).max())
    order = np.argsort(-ref, axis=0, kind="stable")
    best, second = order[0], order[1]
    top = np.take_along_axis(ref, order[:2], axis=0)
    clear = (top[0] - top[1]) > band
    excluded = 1.0 - float(clear.mean())
    mism_clear = int((got[clear] != best[clear]).sum())
    mism_band = int(((got != best) & (got != second) & ~clear).sum())
    aten_mism = int((aten.argmax(0) != best).sum())
    share = [round(float((best == c).mean()), 3) for c in range(v.shape[0])]
    print(what, "band", band, "excluded share", excluded, "mismatches outside the band", mism_clear, "inside, not among the two best",
          mism_band, "ATen fp32 labels != fp64 labels", aten_mism, "class shares", share)
    assert excluded <= 1e-3, f"{what}: the INPUT is wrong - {excluded} of the voxels lie within the band {band}"
    assert mism_clear == 0 and mism_band == 0
    return best.astype(np.uint8)


def check_resampling(lib, dev, in_shape=(32, 40, 36), out_shapes=((45, 50, 47), (20, 33, 36))):
    v = R.smooth_logits(in_shape).numpy()
    for box in out_shapes:
        got = ops_raw.resample_argmax(lib, dev_t(v, dev), box_shape=box)
        assert tuple(got.shape) == tuple(box)
        band_compare(got.cpu().numpy(), v, box, f"resample {in_shape} -> {box}")
        full = tuple(n + 5 for n in box)                                    # resampled AND pasted
        got2 = ops_raw.resample_argmax(lib, dev_t(v, dev), full, (2, 3, 1), box)
        assert np.array_equal(got2.cpu().numpy(), R.paste(got.cpu().numpy(), full, (2, 3, 1)))
        assert torch.equal(got, ops_raw.resample_argmax(lib, dev_t(v, dev), box_shape=box))
    for dt in (torch.bfloat16, torch.float16):                              # 16-bit logits: the reference sees the rounded values
        v16 = torch.from_numpy(v).to(dt)
        got = ops_raw.resample_argmax(lib, v16.to(dev), box_shape=out_shapes[0])
        band_compare(got.cpu().numpy(), v16.float().numpy(), out_shapes[0], f"resample {dt} {in_shape} -> {out_shapes[0]}")


def check_predict_labels(dev, in_shape=(24, 30, 28), box=(31, 36, 33)):
    """Predictor.predict_labels against predict_raw_probability -> argmax -> predict_noncrop_probability of the unchanged methods (on the
    host), under the band rule, with the properties as ints and as 0-d tensors"""
    from segmamba_amd.predictor import Predictor
    v = R.smooth_logits(in_shape, seed=3)
    start, full = (3, 0, 5), (40, 36, 41)
    props = {"shape_after_cropping_before_resample": list(box), "shape_before_cropping": list(full),
             "bbox_used_for_cropping": [[s, s + n] for s, n in zip(start, box)]}
    as_tensors = {"shape_after_cropping_before_resample": [torch.tensor(n) for n in box],
                  "shape_before_cropping": [torch.tensor(n) for n in full],
                  "bbox_used_for_cropping": [[torch.tensor(s), torch.tensor(s + n)] for s, n in zip(start, box)]}
    old = Predictor.predict_noncrop_probability(Predictor.predict_raw_probability(v[None], props).argmax(dim=0), props)
    for p in (props, as_tensors):
        got = Predictor.predict_labels(v[None].to(dev), p)
        assert got.dtype == torch.uint8 and tuple(got.shape) == full
        g = got.cpu().numpy()
        z, y, x = start
        inner = g[z:z + box[0], y:y + box[1], x:x + box[2]]
        best = band_compare(inner, v.numpy(), box, "predict_labels")
        assert np.array_equal(g, R.paste(inner, full, start))              # zeros outside the box
        differ = int((g != old).sum())
        print("predict_labels vs the parent's route: voxels that differ", differ, "fp64 labels vs the parent's route",
              int((R.paste(best, full, start) != old).sum()))
    ident = {"shape_after_cropping_before_resample": list(in_shape), "shape_before_cropping": list(in_shape),
             "bbox_used_for_cropping": [[0, n] for n in in_shape]}
    old = Predictor.predict_noncrop_probability(Predictor.predict_raw_probability(v, ident).argmax(dim=0), ident)
    assert np.array_equal(Predictor.predict_labels(v.to(dev), ident).cpu().numpy(), old)      # identity size: exact


# ---- 5. propagation on the device with plain ATen (reference at BraTS size) ---------------------------------------------------------------
def torch_roots(mask: torch.Tensor) -> torch.Tensor:
    """tests/postprocess_ref.roots_propagate with ATen ops on the mask's device, plus pointer jumping so that the number of rounds
    stays small for blobs"""
    m = mask.bool()
    n = m.numel()
    big = n
    lab = torch.where(m, torch.arange(n, device=m.device).reshape(m.shape), torch.full((), big, device=m.device))
    while True:
        p = F.pad(lab, (1, 1, 1, 1, 1, 1), value=big)
        new = lab
        for sl in ((slice(0, -2), slice(1, -1), slice(1, -1)), (slice(2, None), slice(1, -1), slice(1, -1)),
                   (slice(1, -1), slice(0, -2), slice(1, -1)), (slice(1, -1), slice(2, None), slice(1, -1)),
                   (slice(1, -1), slice(1, -1), slice(0, -2)), (slice(1, -1), slice(1, -1), slice(2, None))):
            new = torch.minimum(new, p[sl])
        new = torch.where(m, new, torch.full((), big, device=m.device))
        flat = torch.cat([new.reshape(-1), torch.full((1,), big, device=m.device)])
        for _ in range(3):
            flat = flat[flat]                                               # a label is a voxel index of the same component
        new = flat[:-1].reshape(m.shape)
        if torch.equal(new, lab):
            break
        lab = new
    return torch.where(m, lab, torch.full((), -1, device=m.device)).to(torch.int32)


def torch_fill(mask: torch.Tensor) -> torch.Tensor:
    m = mask.bool()
    r = torch_roots(~m).long()
    face = torch.zeros_like(m)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = True, True, True, True, True, True
    touch = torch.zeros(m.numel(), dtype=torch.bool, device=m.device)
    touch[r[(r >= 0) & face]] = True
    hole = (r >= 0) & ~touch[r.clamp(min=0)]
    return (m | hole).to(torch.uint8)


def torch_largest(mask: torch.Tensor) -> torch.Tensor:
    r = torch_roots(mask).long()
    cnt = torch.bincount(r[r >= 0], minlength=r.numel())
    if int(cnt.max()) == 0:
        return torch.zeros_like(mask, dtype=torch.uint8)
    winner = torch.nonzero(cnt == cnt.max()).reshape(-1)[-1]
    return (r == winner).to(torch.uint8)
