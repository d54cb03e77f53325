"""Checks shared by tests/test_emu_ccl_labels.py (kernel sources on the CPU emulator) and tests/test_gpu_ccl_labels.py (the HIP
library): labelled connected components (csrc/ccl_roots.hip, csrc/ccl_labels.hip), the per-class selection, the arg-max beyond 8 classes and the host
functions on top.  Every function takes the loaded library and the device its tensors live on.  References: tests/ccl_labels_ref.py.
Every comparison is exact (array_equal); nothing here has a tolerance."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import nifti
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP
from tests import ccl_labels_ref as LR
from tests import postprocess_checks as K
from tests import postprocess_ref as R

NEW_EXPORTS = ("segm_ccl_label_roots", "segm_ccl_label_roots_workspace_bytes", "segm_ccl_label_select",
               "segm_ccl_label_select_workspace_bytes")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def dev_t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                          # a copy: the shared references are read-only


# ---- 1. roots ------------------------------------------------------------------------------------------------------------------------
def check_roots(lib, dev, name, with_scipy=False):
    """-1 where the label is 0; on `labels == c` what the BINARY entry gives for that mask; the numpy restatement; two calls bit-equal"""
    lab, want = LR.case(name)
    t = dev_t(lab, dev)
    roots = ops_raw.ccl_label_roots(lib, t)
    assert roots.dtype == torch.int32 and tuple(roots.shape) == lab.shape
    got = roots.cpu().numpy()
    classes = [int(c) for c in np.unique(lab[lab != 0])]
    print(name, lab.shape, "classes", classes, "components", int((want == np.arange(lab.size).reshape(lab.shape)).sum()))
    assert (got[lab == 0] == -1).all()
    for c in classes:
        m = lab == c
        binary = ops_raw.ccl_roots(lib, dev_t(m.astype(np.uint8), dev)).cpu().numpy()
        assert np.array_equal(got[m], binary[m]), c
    assert np.array_equal(got, want)
    assert torch.equal(roots, ops_raw.ccl_label_roots(lib, t))
    buf = torch.full(lab.shape, 77, dtype=torch.int32, device=dev)
    assert ops_raw.ccl_label_roots(lib, t, out=buf) is buf and torch.equal(buf, roots)
    assert torch.equal(PP.label_component_roots(t), roots)
    if with_scipy:
        for c in classes:
            sl, sn = R.scipy_label(lab == c)
            wl, wn = R.number(np.where(lab == c, got, -1))
            assert wn == sn and np.array_equal(wl, sl), c


def check_known_winners(lib, dev):
    """conditions the cases state: 70 sheets of 30 voxels whose winners by the tie rule are the last sheets of each label; the
    checkerboard's voxels are their own components and the winners the last voxel of each label"""
    lab, _ = LR.case("stripes_x")
    t = dev_t(lab, dev)
    roots = ops_raw.ccl_label_roots(lib, t)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    info = ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_LARGEST)[1].cpu().numpy()
    s = sizes.cpu().numpy().reshape(-1)
    assert int((s > 0).sum()) == 70 and set(s[s > 0].tolist()) == {30}
    assert info[1].tolist() == [24, 69, 30] and info[2].tolist() == [23, 67, 30] and info[3].tolist() == [23, 68, 30]
    lab, _ = LR.case("checker_4x6x66")
    t = dev_t(lab, dev)
    roots = ops_raw.ccl_label_roots(lib, t)
    n = lab.size
    assert np.array_equal(roots.cpu().numpy().reshape(-1), np.arange(n))
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    info = ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_LARGEST)[1].cpu().numpy()
    last = {int(lab.reshape(-1)[n - 1]): n - 1, int(lab.reshape(-1)[n - 2]): n - 2}
    assert info[1].tolist() == [n // 2, last[1], 1] and info[2].tolist() == [n // 2, last[2], 1]


# ---- 2. selection ----------------------------------------------------------------------------------------------------------------------
def check_selection(lib, dev, name):
    """LARGEST, MIN_SIZE at 1 / at the size of the second largest component / one above the largest, and `info`, per class"""
    lab, ref_roots = LR.case(name)
    t = dev_t(lab, dev)
    roots = ops_raw.ccl_label_roots(lib, t)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    out, info = ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_LARGEST)
    assert out.dtype == torch.uint8 and info.dtype == torch.int64 and tuple(info.shape) == (256, 3)
    assert np.array_equal(out.cpu().numpy(), LR.select(lab, ref_roots, "largest"))
    want_info = LR.info(lab, ref_roots)
    assert np.array_equal(info.cpu().numpy(), want_info)
    out2, info2 = ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_LARGEST)
    assert torch.equal(out, out2) and torch.equal(info, info2)
    all_sizes = sorted(np.concatenate([sz for _, sz in LR.class_sizes(lab, ref_roots).values()] + [np.zeros(0, np.int64)]).tolist())
    second = all_sizes[-2] if len(all_sizes) > 1 else 1
    for n in sorted({0, 1, int(second), int(all_sizes[-1]) + 1 if all_sizes else 2}):
        got, info_n = ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_MIN_SIZE, min_size=n)
        assert np.array_equal(got.cpu().numpy(), LR.select(lab, ref_roots, "min_size", n)), n
        assert np.array_equal(info_n.cpu().numpy(), want_info)
    assert np.array_equal(t.cpu().numpy(), lab)                           # the input is not modified
    summary = PP.class_component_summary(t)
    assert summary == {c: (int(want_info[c, 0]), int(want_info[c, 2])) for c in range(1, 256) if want_info[c, 0]}


def check_tie(lib, dev):
    lab, _ = LR.case("tie")
    want = np.zeros_like(lab)
    want[4, 5:7, 60:66] = 1                                               # of the two 12-voxel components of label 1 the later one
    want[lab == 2] = 2                                                    # the larger component of another label does not compete
    got = PP.keep_largest_per_class(dev_t(lab, dev))
    assert np.array_equal(got.cpu().numpy(), want)
    assert PP.class_component_summary(dev_t(lab, dev)) == {1: (3, 12), 2: (1, 30)}


def check_apply(lib, dev):
    """labels 2 and 255 pass through untouched (their second components survive) while label 1 is reduced"""
    lab = LR.apply_case()
    ref_roots = LR.label_roots(lab)
    t = dev_t(lab, dev)
    apply = np.ones(256, dtype=np.uint8)
    apply[[2, 255]] = 0
    roots = ops_raw.ccl_label_roots(lib, t)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    for mode, name, n in ((L.CCL_LARGEST, "largest", 0), (L.CCL_MIN_SIZE, "min_size", 5)):
        got = ops_raw.ccl_label_select(lib, t, roots, sizes, mode, min_size=n, apply=dev_t(apply, dev))[0].cpu().numpy()
        assert np.array_equal(got, LR.select(lab, ref_roots, name, n, apply)), name
        assert np.array_equal(got[(lab == 2) | (lab == 255)], lab[(lab == 2) | (lab == 255)])
        assert int((got == 1).sum()) < int((lab == 1).sum())
        assert int((LR.select(lab, ref_roots, name, n) == 255).sum()) < int((lab == 255).sum())    # a condition: unselected would lose
    got = PP.keep_largest_per_class(t, classes=[1, 128]).cpu().numpy()
    assert np.array_equal(got, LR.select(lab, ref_roots, "largest", 0, apply))
    got = PP.keep_largest_per_class(t, classes=[1, 128], keep=5).cpu().numpy()
    assert np.array_equal(got, LR.select(lab, ref_roots, "min_size", 5, apply))


def parent_route(lib, t, fill):
    """what the parent commit offers for the same result: a loop over the classes of `_keep(labels == c, "largest")` (and `_fill`),
    recombined"""
    out = torch.zeros_like(t)
    kept = {}
    for c in [int(c) for c in torch.unique(t).tolist() if c]:
        kept[c] = PP._keep(lib, (t == c).to(torch.uint8), "largest")
        out[kept[c] != 0] = c
    if fill:
        for c in sorted(kept):
            out[(out == 0) & (PP._fill(lib, kept[c]) != 0)] = c
    return out


def check_against_parent_route(lib, dev, labels):
    t = dev_t(labels, dev)
    for fill in (False, True):
        got = PP.keep_largest_per_class(t, fill_holes=fill)
        assert got.dtype == torch.uint8 and torch.equal(got, parent_route(lib, t, fill)), fill
    assert np.array_equal(t.cpu().numpy(), labels)
    assert np.array_equal(PP.keep_largest_per_class(np.asarray(labels).astype(np.int64)).cpu().numpy(),
                          PP.keep_largest_per_class(t).cpu().numpy())     # numpy and other integer types are accepted


# ---- 3. the arg-max beyond 8 classes ------------------------------------------------------------------------------------------------------
def tie_logits(classes, shape, seed=1):
    """integer-valued logits with deliberate ties between a class and one 2, 5 and (where it exists) 9 classes later, and between all"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-3, 4, size=(classes,) + tuple(shape)).astype(np.float32)
    top = v.max(0)
    k = rng.integers(0, 5, size=shape)
    first = rng.integers(0, classes, size=shape)
    for j, step in enumerate((2, 5, 9)):
        for c in range(classes):
            sel = (k == j) & (first == c)
            v[c][sel] = top[sel] + 1
            v[(c + step) % classes][sel] = top[sel] + 1
    v[:, k == 3] = 2.0
    v[classes - 1, 0, 0, 0] = 9.0                                         # the last class alone at the top of one voxel,
    v[[0, classes - 1], 0, 0, 1] = 9.0                                    # and tied with class 0 at the next
    return v


def check_argmax_many_classes(lib, dev, shape=(5, 7, 24)):
    """10 and 32 classes at identity size, held the way postprocess_checks.check_argmax_identity holds 4: ties (the first of equals wins),
    three dtypes, rows on and off 16 bytes, a channel-strided view"""
    for classes in (10, 32):
        for shp in (shape, (shape[0], shape[1], shape[2] + 3)):
            v = tie_logits(classes, shp)
            want = torch.from_numpy(v).argmax(0).to(torch.uint8).numpy()
            ties = int(((v == v.max(0)).sum(0) > 1).sum())
            assert ties > 0.2 * want.size and want[0, 0, 0] == classes - 1 and want[0, 0, 1] == 0     # conditions on the input
            for dt in (torch.float32, torch.bfloat16, torch.float16):
                t = dev_t(v, dev).to(dt)                                    # small integers: exact in every type
                got = ops_raw.resample_argmax(lib, t, max_classes=L.RESAMPLE_CLASS_LIMIT)
                assert np.array_equal(got.cpu().numpy(), want), (classes, shp, dt)
                wide = torch.zeros((classes + 2,) + tuple(shp[:2]) + (shp[2] + 5,), dtype=dt, device=dev)
                wide[1:1 + classes, :, :, 2:2 + shp[2]] = t
                view = wide[1:1 + classes, :, :, 2:2 + shp[2]]
                assert not view.is_contiguous()
                got = ops_raw.resample_argmax(lib, view, max_classes=L.RESAMPLE_CLASS_LIMIT)
                assert np.array_equal(got.cpu().numpy(), want), (classes, shp, dt, "strided")
            assert np.array_equal(PP.labels_from_logits(dev_t(v, dev)).cpu().numpy(), want)
    from segmamba_amd.predictor import Predictor
    v = tie_logits(10, shape)
    assert np.array_equal(Predictor.predict_labels(dev_t(v, dev)[None]).cpu().numpy(), torch.from_numpy(v).argmax(0).numpy())


def check_argmax_resampled_10(lib, dev, in_shape=(12, 20, 18), box=(15, 25, 23)):
    """10 classes resampled and pasted into a larger volume, under the band rule of postprocess_checks.check_resampling"""
    v = R.smooth_logits(in_shape, classes=10).numpy()
    got = ops_raw.resample_argmax(lib, dev_t(v, dev), box_shape=box, max_classes=L.RESAMPLE_CLASS_LIMIT)
    assert tuple(got.shape) == tuple(box)
    best = K.band_compare(got.cpu().numpy(), v, box, f"resample 10 classes {in_shape} -> {box}")
    assert len(np.unique(best)) >= 8                                      # a condition on the input: most classes win somewhere
    full = tuple(n + 5 for n in box)
    got2 = ops_raw.resample_argmax(lib, dev_t(v, dev), full, (2, 3, 1), box, max_classes=L.RESAMPLE_CLASS_LIMIT)
    assert np.array_equal(got2.cpu().numpy(), R.paste(got.cpu().numpy(), full, (2, 3, 1)))
    props = {"shape_after_cropping_before_resample": list(box), "shape_before_cropping": list(full),
             "bbox_used_for_cropping": [[s, s + n] for s, n in zip((2, 3, 1), box)]}
    assert torch.equal(PP.labels_from_logits(dev_t(v, dev), props), got2)


def check_argmax_refusals(lib, dev):
    with pytest.raises(RuntimeError):
        ops_raw.resample_argmax(lib, torch.zeros(33, 2, 2, 2, device=dev), max_classes=L.RESAMPLE_CLASS_LIMIT)
    with pytest.raises(RuntimeError):
        ops_raw.resample_argmax(lib, torch.zeros(9, 2, 2, 2, device=dev))                      # the raw wrapper's default bound stays 8
    with pytest.raises(RuntimeError):
        ops_raw.resample_argmax(lib, torch.zeros(9, 2, 2, 2, device=dev), max_classes=33)
    with pytest.raises(RuntimeError):
        PP.labels_from_logits(torch.zeros(33, 2, 2, 2, device=dev))
    assert L.RESAMPLE_MAX_CLASSES == 8 and L.RESAMPLE_CLASS_LIMIT == 32
    assert not ops_raw.resample_argmax(lib, torch.zeros(9, 2, 2, 2, device=dev), max_classes=9).any()
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    r = L.ResampleArgmaxArgs()
    r.logits, r.labels = buf.data_ptr(), buf.data_ptr() + 256
    r.in_depth = r.in_height = r.in_width = r.box_depth = r.box_height = r.box_width = r.out_depth = r.out_height = r.out_width = 1
    r.stride_c, r.stride_z, r.stride_y = 1, 1, 1
    r.classes = 33
    assert lib.dll.segm_resample_argmax(r) == -2                          # SEGM_E_SHAPE
    r.classes = 32
    assert lib.dll.segm_resample_argmax(r) == 0


# ---- 4. refusals and exports -----------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    roots = ops_raw.ccl_label_roots(lib, ok)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    other = "cpu" if str(dev) != "cpu" else None
    i32 = dict(dtype=torch.int32, device=dev)
    bad = [
        lambda: ops_raw.ccl_label_roots(lib, ok.int()),                                         # dtype
        lambda: ops_raw.ccl_label_roots(lib, ok[0]),                                            # 2-D
        lambda: ops_raw.ccl_label_roots(lib, ok.transpose(0, 2)),                               # not contiguous
        lambda: ops_raw.ccl_label_roots(lib, ok[:0]),                                           # empty
        lambda: ops_raw.ccl_label_roots(lib, ok, out=torch.zeros(4, 5, 6, dtype=torch.int64, device=dev)),
        lambda: ops_raw.ccl_label_roots(lib, ok, out=torch.zeros(4, 5, 7, **i32)),
        lambda: ops_raw.ccl_label_roots(lib, ok, out=torch.zeros(4, 6, 5, **i32).transpose(1, 2)),
        lambda: ops_raw.ccl_label_select(lib, ok.int(), roots, sizes, L.CCL_LARGEST),
        lambda: ops_raw.ccl_label_select(lib, ok, roots.long(), sizes, L.CCL_LARGEST),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes.long(), L.CCL_LARGEST),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes[:3], L.CCL_LARGEST),
        lambda: ops_raw.ccl_label_select(lib, ok, roots[:, :, :5], sizes, L.CCL_LARGEST),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, 3),                             # mode
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_FILL),                    # FILL is not a mode here
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_MIN_SIZE, min_size=-1),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_LARGEST, apply=torch.zeros(100, dtype=torch.uint8, device=dev)),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_LARGEST, apply=torch.zeros(256, **i32)),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_LARGEST, out=torch.zeros(4, 5, 6, **i32)),
        lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_LARGEST, out=torch.zeros(4, 5, 7, dtype=torch.uint8, device=dev)),
        lambda: PP.label_component_roots(ok[0]),
        lambda: PP.keep_largest_per_class(ok[None]),
        lambda: PP.keep_largest_per_class(ok.float()),
        lambda: PP.keep_largest_per_class(ok, classes=[0]),
        lambda: PP.keep_largest_per_class(ok, classes=[256]),
        lambda: PP.class_component_summary(ok[0]),
    ]
    if other is not None:                                                                       # mismatching devices
        bad += [lambda: ops_raw.ccl_label_roots(lib, ok, out=torch.zeros(4, 5, 6, dtype=torch.int32, device=other)),
                lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes.to(other), L.CCL_LARGEST),
                lambda: ops_raw.ccl_label_select(lib, ok, roots, sizes, L.CCL_LARGEST, apply=torch.ones(256, dtype=torch.uint8, device=other))]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")


def check_c_refusals(lib, dev):
    """every C refusal returns its code and launches nothing: the output buffers keep their fill"""
    dll = lib.dll
    buf = torch.full((128,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
    marks = torch.full((1024,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
    assert dll.segm_ccl_label_roots(None) == -1 and dll.segm_ccl_label_select(None) == -1
    a = L.CclLabelRootsArgs()
    assert dll.segm_ccl_label_roots(a) == -1                              # SEGM_E_NULL
    a.labels = buf.data_ptr()
    assert dll.segm_ccl_label_roots(a) == -1                              # no roots
    a.roots = marks.data_ptr()
    assert dll.segm_ccl_label_roots(a) == -2                              # SEGM_E_SHAPE: no size
    a.depth, a.height, a.width = 2048, 1024, 1024
    assert dll.segm_ccl_label_roots(a) == -2                              # 2^31 voxels
    a.depth, a.height, a.width = 65536, 65536, 1
    assert dll.segm_ccl_label_roots(a) == -2
    a.depth, a.height, a.width = 2, 2, 2
    a.roots = marks.data_ptr() + 2
    assert dll.segm_ccl_label_roots(a) == -2                              # misaligned roots
    a.roots = marks.data_ptr()
    assert dll.segm_ccl_label_roots(a) == -6                              # SEGM_E_WORKSPACE: none
    a.workspace, a.workspace_bytes = marks.data_ptr() + 512, 31
    assert dll.segm_ccl_label_roots(a) == -6                              # one byte short
    a.workspace, a.workspace_bytes = marks.data_ptr() + 514, 32
    assert dll.segm_ccl_label_roots(a) == -6                              # misaligned
    assert dll.segm_ccl_label_roots_workspace_bytes(8) == 32 and dll.segm_ccl_label_roots_workspace_bytes(0) == 0
    assert dll.segm_ccl_label_roots_workspace_bytes(2 ** 31) == 0 and dll.segm_ccl_label_roots_workspace_bytes(2 ** 31 - 1) == 4 * (2 ** 31 - 1)
    c = L.CclLabelSelectArgs()
    assert dll.segm_ccl_label_select(c) == -1
    c.labels = c.roots = c.sizes = buf.data_ptr()
    c.out = marks.data_ptr()
    assert dll.segm_ccl_label_select(c) == -1                             # no info
    c.info = marks.data_ptr() + 64
    c.mode = 7
    assert dll.segm_ccl_label_select(c) == -2
    c.mode = L.CCL_FILL
    assert dll.segm_ccl_label_select(c) == -2                             # FILL is not a mode here
    c.mode = L.CCL_MIN_SIZE
    c.depth, c.height, c.width = 2, 2, 2
    c.min_size = -1
    assert dll.segm_ccl_label_select(c) == -2
    c.min_size = 0
    c.depth = 0
    assert dll.segm_ccl_label_select(c) == -2
    c.depth, c.height, c.width = 2048, 1024, 1024
    assert dll.segm_ccl_label_select(c) == -2
    c.depth, c.height, c.width = 2, 2, 2
    for field in ("roots", "sizes", "info"):
        keep = getattr(c, field)
        setattr(c, field, keep + 2)
        assert dll.segm_ccl_label_select(c) == -2, field                  # misaligned
        setattr(c, field, keep)
    assert dll.segm_ccl_label_select(c) == -6                             # no workspace
    need = dll.segm_ccl_label_select_workspace_bytes(8)
    assert need == 256 * 2 * 8 and dll.segm_ccl_label_select_workspace_bytes(0) == 0 and dll.segm_ccl_label_select_workspace_bytes(2 ** 31) == 0
    big = torch.full((need // 8,), 0x5a5a5a5a5a5a5a5a, dtype=torch.int64, device=dev)
    c.workspace, c.workspace_bytes = big.data_ptr(), need - 1
    assert dll.segm_ccl_label_select(c) == -6                             # one byte short
    if str(dev) != "cpu":
        torch.cuda.synchronize()
    assert bool((marks == 0x5a5a5a5a5a5a5a5a).all()) and bool((big == 0x5a5a5a5a5a5a5a5a).all())      # nothing was launched


def check_exports(lib):
    import re
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10                               # additive: the ABI number stays
    header = open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()
    assert "#define SEGM_RESAMPLE_MAX_CLASSES 8" in header and "#define SEGM_RESAMPLE_CLASS_LIMIT 32" in header


# ---- 5. the host side ----------------------------------------------------------------------------------------------------------------------
def check_save_organs(dev, tmp_path):
    from segmamba_amd.predictor import Predictor
    lab, _ = LR.case("ten_class_20x30x70")
    names = [f"organ_{i}" for i in range(1, 10)]
    p = Predictor(None)
    paths = p.save_organs_to_nii(dev_t(lab, dev), [torch.tensor(1.0), torch.tensor(0.9), torch.tensor(2.5)], str(tmp_path / "plain"), names)
    assert [os.path.basename(q) for q in paths] == [n + ".nii.gz" for n in names]
    for i, q in enumerate(paths):
        got, spacing = nifti.read_nifti(q)
        assert got.dtype == np.uint8 and np.array_equal(got, (lab == i + 1).astype(np.uint8)), i
        assert spacing == (1.0, float(np.float32(0.9)), 2.5)
    shrunk = 0
    paths = p.save_organs_to_nii(np.array(lab), (1, 1, 1), str(tmp_path / "post"), names, postprocess=True)     # numpy in
    for i, q in enumerate(paths):
        got = nifti.read_nifti(q)[0]
        assert np.array_equal(got, R.largest_connected_domain((lab == i + 1).astype(np.uint8))), i
        shrunk += int(got.sum()) < int((lab == i + 1).sum())
    assert shrunk == 9                                                    # a condition on the input: every organ had islands
    hollow = np.array(LR.case("shell_around_ball")[0])
    paths = p.save_organs_to_nii(dev_t(hollow, dev)[None], (1, 1, 1), str(tmp_path / "hollow"), ["shell", "ball"], postprocess=True)
    got = [nifti.read_nifti(q)[0] for q in paths]
    assert np.array_equal(got[0], (hollow != 0).astype(np.uint8)) and np.array_equal(got[1], (hollow == 2).astype(np.uint8))
    for bad in (lambda: p.save_organs_to_nii(lab[0], (1, 1, 1), str(tmp_path / "x"), names),
                lambda: p.save_organs_to_nii(lab, (1, 1, 1), str(tmp_path / "x"), []),
                lambda: p.save_organs_to_nii(lab, (1, 1, 1), str(tmp_path / "x"), ["a", "a"])):
        with pytest.raises(RuntimeError):
            bad()


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def check_tools(dev, tmp_path):
    """--per-class and --organs of tools/finish_predictions.py on a two-case directory, then --labels of tools/compute_metrics.py"""
    finish, compute = _tool("finish_predictions"), _tool("compute_metrics")
    for d in ("logits", "gt"):
        (tmp_path / d).mkdir()
    labels = {}
    for i in range(2):
        lab = LR.ten_class((12 + i, 20, 66), seed=5 + i)
        onehot = np.stack([(lab == c) for c in range(10)]).astype(np.float32) * 3.0
        if i == 0:
            np.save(tmp_path / "logits" / "case0.npy", onehot)
        else:
            np.savez(tmp_path / "logits" / "case1.npz", logits=onehot, spacing=np.array([1.0, 1.5, 2.0]))
        labels[i] = lab
        nifti.write_nifti(str(tmp_path / "gt" / f"case{i}.nii.gz"), lab)
    organs = [f"o{i}" for i in range(1, 10)]
    written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "pred"), "--organs", ",".join(organs)])
    assert len(written) == 2 * (1 + 9)
    for i in range(2):
        case = written[10 * i:10 * i + 10]
        assert os.path.basename(case[0]) == f"case{i}.nii.gz" and np.array_equal(nifti.read_nifti(case[0])[0], labels[i])
        for k, q in enumerate(case[1:]):
            assert q == str(tmp_path / "pred" / f"case{i}" / f"{organs[k]}.nii.gz")
            assert np.array_equal(nifti.read_nifti(q)[0], (labels[i] == k + 1).astype(np.uint8))
    assert nifti.read_nifti(written[11])[1] == (1.0, 1.5, 2.0)
    written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "pc"), "--per-class"])
    assert [os.path.basename(w) for w in written] == ["case0.nii.gz", "case1.nii.gz"]
    for i in range(2):
        want = LR.select(labels[i], LR.label_roots(labels[i]), "largest")
        assert (want != labels[i]).any() and np.array_equal(nifti.read_nifti(written[i])[0], want)
    with pytest.raises(RuntimeError):
        finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "no"), "--per-class", "--postprocess"])
    res = compute.main(["--pred", str(tmp_path / "pc"), "--gt", str(tmp_path / "gt"), "--labels", "1,2,3,4,5,6,7,8,9"])
    assert res.shape == (2, 9, 2)
    for i in range(2):
        pc = nifti.read_nifti(written[i])[0]
        assert np.array_equal(res[i], M.case_metrics(pc, labels[i], regions=[(c,) for c in range(1, 10)], max_regions=None))
    assert (res[:, :, 0] > 0.5).all() and (res[:, :, 0] < 1.0).all()      # islands and speckle went: near, not equal to, the truth


class Readbacks:
    """counts the launches and the device-to-host copies that segmamba_amd.metrics makes: the calls of its kernels' wrappers, of
    `_readback`, and of Tensor.tolist / Tensor.cpu inside the module"""

    def __init__(self, monkeypatch):
        self.calls = {}
        for k in ("seg_regions", "edt_sq", "edt_sq_long", "planes_bbox", "border_distances"):
            monkeypatch.setattr(ops_raw, k, self._wrap(k, getattr(ops_raw, k)))
        monkeypatch.setattr(M, "_readback", self._wrap("_readback", M._readback))

    def _wrap(self, name, fn):
        def counted(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **kw)
        return counted

    def take(self):
        out, self.calls = self.calls, {}
        return out


def check_metrics_groups(dev, monkeypatch):
    """nine one-label regions (`max_regions=None`) = the call with regions 1 .. 8 and the call with region 9; up to eight regions every call makes the
    launches and readbacks it made (one seg_regions, one transform, one gather; on the box route two `_readback`s)"""
    pred = LR.ten_class((20, 30, 70), seed=1)
    gt = LR.ten_class((20, 30, 70), seed=2)
    pred[pred == 9] = 0                                                   # an empty prediction for region 9: the [0, 50] rule
    tp, tg = dev_t(pred, dev), dev_t(gt, dev)
    nine = [(c,) for c in range(1, 10)]
    monkeypatch.delenv("SEGM_EDT_LONG", raising=False)
    brats_before = M.case_metrics(tp, tg)
    calls = Readbacks(monkeypatch)
    got = M.case_metrics(tp, tg, regions=nine, max_regions=None)
    assert calls.take() == {"seg_regions": 2, "edt_sq": 1, "border_distances": 1}          # region 9 is not live: no second transform
    want = np.concatenate([M.case_metrics(tp, tg, regions=nine[:8]), M.case_metrics(tp, tg, regions=nine[8:])])
    assert got.shape == (9, 2) and np.array_equal(got, want) and got[8].tolist() == [0.0, 50.0]
    calls.take()
    assert np.array_equal(M.case_metrics(tp, tg), brats_before)
    assert calls.take() == {"seg_regions": 1, "edt_sq": 1, "border_distances": 1}
    monkeypatch.setenv("SEGM_EDT_LONG", "box")
    assert np.array_equal(M.case_metrics(tp, tg), brats_before)
    three = calls.take()
    assert three["_readback"] == 2 and three["seg_regions"] == 1 and three["planes_bbox"] == 1
    assert np.array_equal(M.case_metrics(tp, tg, regions=nine, max_regions=None), want)
    assert calls.take()["_readback"] == 3                                 # two for regions 1 .. 8, one for region 9 (nothing live)
    monkeypatch.delenv("SEGM_EDT_LONG", raising=False)
    gt9 = M.case_metrics(tg, tg, regions=nine, max_regions=None)
    assert gt9[:, 0].tolist() == [1.0] * 9 and gt9[:, 1].tolist() == [0.0] * 9
    assert np.array_equal(M.validation_dice(tp, tg, nine),
                          np.concatenate([M.validation_dice(tp, tg, nine[:8]), M.validation_dice(tp, tg, nine[8:])]))
    masks = M.region_masks(tp, nine)
    assert tuple(masks.shape) == (9,) + pred.shape and all(torch.equal(masks[c - 1], (tp == c).float()) for c in range(1, 10))
    results, mean, _ = M.evaluate([(tp, tg), (tg, tg)], nine, max_regions=None)
    assert results.shape == (2, 9, 2) and np.array_equal(results[0], want) and np.array_equal(mean, (want + gt9) / 2)
    with pytest.raises(RuntimeError):
        M._table(nine, torch.device(dev))                                 # a kernel call still carries at most 8 region planes
    with pytest.raises(RuntimeError):
        M.case_metrics(tp, tg, regions=nine)                              # the default bound stays (tests/metrics_checks.py pins it)
    with pytest.raises(RuntimeError):
        M.case_metrics(tp, tg, regions=nine[:3], max_regions=2)
