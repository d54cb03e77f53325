"""Checks shared by tests/test_emu_ccl_conn.py (kernel sources on the CPU emulator) and tests/test_gpu_ccl_conn.py (the HIP library):
connected components at connectivity 1, 2 and 3 (csrc/ccl_roots.hip), of a mask and per class of a label volume, and the `connectivity`
keyword of the host functions above them.  Every function takes the loaded library and the device its tensors live on.  References:
tests/ccl_conn_ref.py (numpy, no scipy).  Every comparison is exact; nothing here has a tolerance."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import nifti
from segmamba_amd import ops_raw
from segmamba_amd import postprocess as PP
from tests import ccl_conn_ref as CR
from tests import ccl_labels_ref as LR
from tests import postprocess_ref as R

NEW_EXPORTS = ("segm_ccl_roots_conn", "segm_ccl_label_roots_conn")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5a5a5a5a5a5a5a5a
SMALL = 20000


def dev_t(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)                          # a copy: the shared references are read-only


def conn_roots(lib, volume, bit, invert, c):
    """segm_ccl_roots_conn itself, at every c"""
    out = torch.full(volume.shape, -7, dtype=torch.int32, device=volume.device)
    nbytes = lib.dll.segm_ccl_roots_workspace_bytes(volume.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=volume.device)
    a = L.CclRootsConnArgs()
    a.depth, a.height, a.width = volume.shape
    a.bit, a.invert, a.connectivity = bit, invert, c
    a.volume, a.roots, a.workspace, a.workspace_bytes, a.stream = volume.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(volume)
    lib.check(lib.dll.segm_ccl_roots_conn(a), "segm_ccl_roots_conn")
    return out


def conn_label_roots(lib, labels, c):
    out = torch.full(labels.shape, -7, dtype=torch.int32, device=labels.device)
    nbytes = lib.dll.segm_ccl_label_roots_workspace_bytes(labels.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=labels.device)
    a = L.CclLabelRootsConnArgs()
    a.depth, a.height, a.width = labels.shape
    a.connectivity = c
    a.labels, a.roots, a.workspace, a.workspace_bytes, a.stream = labels.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(labels)
    lib.check(lib.dll.segm_ccl_label_roots_conn(a), "segm_ccl_label_roots_conn")
    return out


def legacy_roots(lib, volume, bit=-1, invert=0, reserved=0):
    """segm_ccl_roots itself, with its own struct (ops_raw.ccl_roots calls segm_ccl_roots_conn at every c)"""
    out = torch.full(volume.shape, -7, dtype=torch.int32, device=volume.device)
    nbytes = lib.dll.segm_ccl_roots_workspace_bytes(volume.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=volume.device)
    a = L.CclRootsArgs()
    a.depth, a.height, a.width = volume.shape
    a.bit, a.invert, a.reserved = bit, invert, reserved
    a.volume, a.roots, a.workspace, a.workspace_bytes, a.stream = volume.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(volume)
    lib.check(lib.dll.segm_ccl_roots(a), "segm_ccl_roots")
    return out


def legacy_label_roots(lib, labels, reserved=0):
    out = torch.full(labels.shape, -7, dtype=torch.int32, device=labels.device)
    nbytes = lib.dll.segm_ccl_label_roots_workspace_bytes(labels.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=labels.device)
    a = L.CclLabelRootsArgs()
    a.depth, a.height, a.width, a.reserved = *labels.shape, reserved
    a.labels, a.roots, a.workspace, a.workspace_bytes, a.stream = labels.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(labels)
    lib.check(lib.dll.segm_ccl_label_roots(a), "segm_ccl_label_roots")
    return out


# ---- 1. the binary entry ----------------------------------------------------------------------------------------------------------------
def check_mask(lib, dev, name):
    """for c = 1, 2, 3: the roots equal the reference at every voxel with `bit = -1`, with the mask in one bit of a byte whose other
    bits are noise, and with that bit inverted; the stated component counts; c = 1 through the new entry = segm_ccl_roots; two calls
    bit-equal.  Volumes of up to SMALL voxels also: bit 7, the complement inverted, the inverse with bit = -1, component_roots."""
    m = CR.mask(name)
    t = dev_t(m, dev)
    bit = 1 + len(name) % 7                                               # 1 .. 7, fixed per case
    noise = np.random.default_rng(len(name)).integers(0, 256, size=m.shape).astype(np.uint8) & np.uint8(~(1 << bit) & 0xff)
    packed = dev_t(noise | (m << bit).astype(np.uint8), dev)
    small = m.size <= SMALL                                               # the larger volumes skip what repeats a check made above
    for c in CR.CONNECTIVITIES:
        want = CR.mask_roots(name, c)
        n = CR.components(want)
        print(name, m.shape, "c", c, "components", n)
        if name in CR.KNOWN:
            assert n == CR.KNOWN[name][c], (name, c, n)
        got = ops_raw.ccl_roots(lib, t, connectivity=c)
        assert got.dtype == torch.int32 and tuple(got.shape) == m.shape
        assert np.array_equal(got.cpu().numpy(), want), (name, c)
        assert torch.equal(got, ops_raw.ccl_roots(lib, t, connectivity=c)), (name, c)
        assert torch.equal(got, ops_raw.ccl_roots(lib, packed, bit=bit, connectivity=c)), (name, c, bit)
        inv = ops_raw.ccl_roots(lib, packed, bit=bit, invert=True, connectivity=c)
        assert np.array_equal(inv.cpu().numpy(), CR.mask_roots(name, c, True)), (name, c, bit, "inverted")
        if small:
            assert torch.equal(got, ops_raw.ccl_roots(lib, dev_t(m << 7, dev), bit=7, connectivity=c)), (name, c)
            assert torch.equal(got, ops_raw.ccl_roots(lib, dev_t(1 - m, dev), invert=True, connectivity=c)), (name, c)
            assert torch.equal(inv, ops_raw.ccl_roots(lib, t, invert=True, connectivity=c)), (name, c, "inverted")
            assert torch.equal(PP.component_roots(t, connectivity=c), got)
    assert torch.equal(conn_roots(lib, t, -1, 0, 1), legacy_roots(lib, t))                    # c = 1: the existing entry's result
    if small:
        assert torch.equal(conn_roots(lib, packed, bit, 1, 1), legacy_roots(lib, packed, bit, 1))
        assert torch.equal(conn_roots(lib, t, -1, 0, 3), ops_raw.ccl_roots(lib, t, connectivity=3))
    assert np.array_equal(t.cpu().numpy(), m)                             # the input is not modified


def check_reference_against_scipy(names):
    """the numpy reference = scipy.ndimage.label with generate_binary_structure(3, c): roots and component counts"""
    for name in names:
        for c in CR.CONNECTIVITIES:
            for invert in (False, True):
                want, _, n = CR.scipy_roots(CR.mask(name) == (0 if invert else 1), c)
                got = CR.mask_roots(name, c, invert)
                assert np.array_equal(got, want), (name, c, invert)
                assert CR.components(got) == n
                if name in CR.KNOWN and not invert:
                    assert n == CR.KNOWN[name][c], (name, c, n)
    from scipy import ndimage
    for c, n in ((1, 124), (2, 124), (3, 97)):
        filled = ndimage.binary_fill_holes(CR.hollow_cube(), structure=ndimage.generate_binary_structure(3, c))
        assert int(filled.sum()) == n and np.array_equal(filled, CR.fill_holes(CR.hollow_cube(), c))
    for name, known in CR.KNOWN_LABELS.items():
        lab = CR.labels(name)
        for c in CR.CONNECTIVITIES:
            assert sum(CR.scipy_roots(lab == k, c)[2] for k in np.unique(lab[lab != 0])) == known[c], (name, c)


# ---- 2. the labelled entry --------------------------------------------------------------------------------------------------------------
def check_labels(lib, dev, name):
    """for c = 1, 2, 3: -1 on the background; per class what the BINARY entry gives on `labels == k` at the same c; the numpy
    reference; c = 1 through the new entry = segm_ccl_label_roots; two calls bit-equal"""
    lab = CR.labels(name)
    t = dev_t(lab, dev)
    classes = [int(k) for k in np.unique(lab[lab != 0])]
    for c in CR.CONNECTIVITIES:
        want = CR.labels_roots(name, c)
        n = CR.components(want)
        print(name, lab.shape, "c", c, "classes", classes, "components", n)
        if name in CR.KNOWN_LABELS:
            assert n == CR.KNOWN_LABELS[name][c], (name, c, n)
        roots = ops_raw.ccl_label_roots(lib, t, connectivity=c)
        assert roots.dtype == torch.int32 and tuple(roots.shape) == lab.shape
        got = roots.cpu().numpy()
        assert (got[lab == 0] == -1).all()
        for k in classes:
            m = lab == k
            binary = ops_raw.ccl_roots(lib, dev_t(m.astype(np.uint8), dev), connectivity=c).cpu().numpy()
            assert np.array_equal(got[m], binary[m]), (name, c, k)
        assert np.array_equal(got, want), (name, c)
        buf = torch.full(lab.shape, 77, dtype=torch.int32, device=dev)
        assert ops_raw.ccl_label_roots(lib, t, out=buf, connectivity=c) is buf and torch.equal(buf, roots)      # the second call
        if lab.size <= SMALL:
            assert torch.equal(PP.label_component_roots(t, connectivity=c), roots)
    assert torch.equal(conn_label_roots(lib, t, 1), legacy_label_roots(lib, t))               # c = 1: the existing entry's result
    if lab.size <= SMALL:
        assert torch.equal(conn_label_roots(lib, t, 3), ops_raw.ccl_label_roots(lib, t, connectivity=3))
    assert np.array_equal(t.cpu().numpy(), lab)


def check_legacy_entries_ignore_reserved(lib, dev):
    """segm_ccl_roots and segm_ccl_label_roots are connectivity 1 whatever their `reserved` field holds: with reserved = 3, the value
    that the layout-identical *_conn struct reads as its connectivity, the roots are the reference at 1, which differs from that at 3
    (hand case: 5 against 3 components)"""
    for got, want1, want3 in (
            (legacy_roots(lib, dev_t(CR.mask("hand"), dev), reserved=3), CR.mask_roots("hand", 1), CR.mask_roots("hand", 3)),
            (legacy_label_roots(lib, dev_t(CR.labels("diagonal_island"), dev), reserved=3), CR.labels_roots("diagonal_island", 1),
             CR.labels_roots("diagonal_island", 3))):
        assert not np.array_equal(want1, want3) and CR.components(want1) > CR.components(want3)
        assert np.array_equal(got.cpu().numpy(), want1)
    assert CR.components(CR.mask_roots("hand", 1)) == 5 and CR.components(CR.mask_roots("hand", 3)) == 3


# ---- 3. the host functions ----------------------------------------------------------------------------------------------------------------
def check_host_mask_functions(lib, dev, name):
    """label, largest_connected_domain, remove_small_components, component_summary at c = 1, 2, 3 against the numpy restatement on the
    reference roots (equal sizes: the last root wins; holes at background connectivity 1); the default = the call without the keyword"""
    m = CR.mask(name)
    t = dev_t(m, dev)
    for c in CR.CONNECTIVITIES:
        want = CR.mask_roots(name, c)
        lab, num = PP.label(t, connectivity=c)
        want_lab, want_num = R.number(want)
        assert lab.dtype == torch.int32 and num == want_num and np.array_equal(lab.cpu().numpy(), want_lab), (name, c)
        assert torch.equal(PP.label(t, return_num=False, connectivity=c), lab)
        sizes = np.bincount(want[want >= 0], minlength=1)
        big = int(sizes.max()) if sizes.size else 0
        assert PP.component_summary(t, connectivity=c) == (want_num, big), (name, c)
        largest = R.largest(m, roots=want)
        got = PP.largest_connected_domain(t, connectivity=c)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), CR.fill_holes(largest, 1)), (name, c)
        second = int(np.sort(sizes[sizes > 0])[-2]) if (sizes > 0).sum() > 1 else 1
        for n in sorted({1, 2, second, big + 1}):
            got = PP.remove_small_components(t, n, connectivity=c)
            assert np.array_equal(got.cpu().numpy(), R.min_size(m, n, roots=want)), (name, c, n)
    assert torch.equal(PP.label(t, connectivity=1)[0], PP.label(t)[0])
    assert torch.equal(PP.largest_connected_domain(t, connectivity=1), PP.largest_connected_domain(t))
    assert torch.equal(PP.remove_small_components(t, 2, connectivity=1), PP.remove_small_components(t, 2))
    assert PP.component_summary(t, connectivity=1) == PP.component_summary(t)
    assert torch.equal(PP.binary_fill_holes(t, connectivity=1), PP.binary_fill_holes(t))
    assert torch.equal(PP.component_roots(t, connectivity=1), PP.component_roots(t))


def check_label_equals_scipy(dev, names):
    for name in names:
        t = dev_t(CR.mask(name), dev)
        for c in CR.CONNECTIVITIES:
            _, want, n = CR.scipy_roots(CR.mask(name), c)
            lab, num = PP.label(t, connectivity=c)
            assert num == n and np.array_equal(lab.cpu().numpy(), want), (name, c)


def check_tie_rule(dev):
    """two components of 3 voxels that exist only from c = 2 on (an L of edge neighbours each) and a single voxel: the later L wins"""
    m = np.zeros((6, 9, 70), dtype=np.uint8)
    for z, y, x in ((1, 1, 5), (1, 2, 6), (1, 3, 7), (4, 5, 62), (4, 6, 63), (4, 7, 64), (0, 0, 0)):
        m[z, y, x] = 1
    t = dev_t(m, dev)
    assert PP.component_summary(t) == (7, 1) and PP.component_summary(t, connectivity=2) == (3, 3)
    want = np.zeros_like(m)
    want[4, 5, 62] = want[4, 6, 63] = want[4, 7, 64] = 1
    for c in (2, 3):
        assert np.array_equal(PP.largest_connected_domain(t, connectivity=c).cpu().numpy(), want)
    only = np.zeros_like(m)
    only[4, 7, 64] = 1                                                    # c = 1: seven single voxels, the last one wins
    assert np.array_equal(PP.largest_connected_domain(t).cpu().numpy(), only)


def check_fill_holes(dev):
    """`binary_fill_holes(connectivity)` is the BACKGROUND's: the hollow cube whose inside reaches the outside through one corner keeps
    its 97 voxels at 3 and is filled to 124 at 1 and 2.  Inside largest_connected_domain / keep_largest_per_class the background stays
    at 1 whatever the foreground's connectivity: 124 at every c."""
    cube = CR.hollow_cube()
    t = dev_t(cube, dev)
    assert int(cube.sum()) == 97
    for c, n in ((1, 124), (2, 124), (3, 97)):
        got = PP.binary_fill_holes(t, connectivity=c)
        assert got.dtype == torch.uint8 and int(got.sum().item()) == n, (c, int(got.sum().item()))
        assert np.array_equal(got.cpu().numpy(), CR.fill_holes(cube, c))
    assert int(PP.binary_fill_holes(t).sum().item()) == 124
    for c in CR.CONNECTIVITIES:
        assert int(PP.largest_connected_domain(t, connectivity=c).sum().item()) == 124, c
        assert int(PP.keep_largest_per_class(t * 5, fill_holes=True, connectivity=c).sum().item()) == 5 * 124, c
        assert int((PP.postprocess_labels(t, regions=[(1,)], connectivity=c) != 0).sum().item()) == 97         # voxels are only removed
    for name in ("random_5x5x65_03", "random_9x10x131_06"):
        for c in CR.CONNECTIVITIES:
            got = PP.binary_fill_holes(dev_t(CR.mask(name), dev), connectivity=c)
            assert np.array_equal(got.cpu().numpy(), CR.fill_holes(CR.mask(name), c)), (name, c)


def loop_route(lib, t, fill, c):
    """the per-class loop of the binary functions at connectivity c, recombined (holes at background connectivity 1)"""
    out = torch.zeros_like(t)
    kept = {}
    for k in [int(k) for k in torch.unique(t).tolist() if k]:
        kept[k] = PP._keep(lib, (t == k).to(torch.uint8), "largest", connectivity=c)
        out[kept[k] != 0] = k
    if fill:
        for k in sorted(kept):
            out[(out == 0) & (PP._fill(lib, kept[k]) != 0)] = k
    return out


def check_keep_largest_per_class(lib, dev, name):
    """keep_largest_per_class(connectivity=c) = the per-class loop of the binary functions at c = the numpy selection on the reference
    roots; the summary per class; postprocess_labels per region against its numpy restatement at c"""
    lab = CR.labels(name)
    t = dev_t(lab, dev)
    for c in CR.CONNECTIVITIES:
        want_roots = CR.labels_roots(name, c)
        got = PP.keep_largest_per_class(t, connectivity=c)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), LR.select(lab, want_roots, "largest")), (name, c)
        for fill in (False, True):
            assert torch.equal(PP.keep_largest_per_class(t, fill_holes=fill, connectivity=c), loop_route(lib, t, fill, c)), (name, c, fill)
        assert np.array_equal(PP.keep_largest_per_class(t, keep=3, connectivity=c).cpu().numpy(), LR.select(lab, want_roots, "min_size", 3))
        info = LR.info(lab, want_roots)
        assert PP.class_component_summary(t, connectivity=c) == {k: (int(info[k, 0]), int(info[k, 2])) for k in range(1, 256) if info[k, 0]}
        regions = [(1, 2, 3), (2, 3), (3,)]
        want = lab.copy()
        for reg in regions:
            m = np.isin(want, reg)
            kept = CR.fill_holes(R.largest(m, roots=CR.roots(m, c)), 1)
            want[m & (kept == 0)] = 0
        assert np.array_equal(PP.postprocess_labels(t, regions=regions, connectivity=c).cpu().numpy(), want), (name, c)
    assert torch.equal(PP.keep_largest_per_class(t, connectivity=1), PP.keep_largest_per_class(t))
    assert torch.equal(PP.keep_largest_per_class(t, fill_holes=True, connectivity=1), PP.keep_largest_per_class(t, fill_holes=True))
    assert PP.class_component_summary(t, connectivity=1) == PP.class_component_summary(t)
    assert torch.equal(PP.postprocess_labels(t, connectivity=1), PP.postprocess_labels(t))
    assert torch.equal(PP.label_component_roots(t, connectivity=1), PP.label_component_roots(t))


def check_diagonal_island(dev):
    """what the feature is for: the island that hangs on its organ by a corner goes at c = 1 and 2 and stays at 3"""
    lab = CR.labels("diagonal_island")
    t = dev_t(lab, dev)
    for c in (1, 2):
        got = PP.keep_largest_per_class(t, connectivity=c).cpu().numpy()
        assert got[4, 4, 64] == 0 and got[4, 4, 65] == 0 and got[1, 7, 40] == 0 and int((got == 1).sum()) == 54
    got = PP.keep_largest_per_class(t, connectivity=3).cpu().numpy()
    assert got[4, 4, 64] == 1 and got[4, 4, 65] == 1 and got[1, 7, 40] == 0 and int((got == 1).sum()) == 56
    assert PP.class_component_summary(t) == {1: (2, 54), 2: (2, 60)}
    assert PP.class_component_summary(t, connectivity=3) == {1: (1, 56), 2: (2, 60)}


# ---- 4. refusals and exports ------------------------------------------------------------------------------------------------------------
def check_value_errors(lib, dev):
    ok = torch.zeros(4, 5, 6, dtype=torch.uint8, device=dev)
    for c in (0, 4, -1, 1.5, "3", None, True):
        calls = [lambda: ops_raw.ccl_roots(lib, ok, connectivity=c), lambda: ops_raw.ccl_label_roots(lib, ok, connectivity=c),
                 lambda: PP.component_roots(ok, connectivity=c), lambda: PP.label(ok, connectivity=c),
                 lambda: PP.binary_fill_holes(ok, connectivity=c), lambda: PP.remove_small_components(ok, 2, connectivity=c),
                 lambda: PP.largest_connected_domain(ok, connectivity=c), lambda: PP.component_summary(ok, connectivity=c),
                 lambda: PP.postprocess_labels(ok, connectivity=c), lambda: PP.postprocess_labels(ok, regions=[], connectivity=c),
                 lambda: PP.label_component_roots(ok, connectivity=c), lambda: PP.keep_largest_per_class(ok, connectivity=c),
                 lambda: PP.class_component_summary(ok, connectivity=c)]
        for i, call in enumerate(calls):
            with pytest.raises(ValueError):
                call()
                pytest.fail(f"connectivity {c!r}: call {i} did not raise")
    bad2d = ok[0]                                                         # a bad volume too: the connectivity is looked at first
    for call in (lambda: ops_raw.ccl_roots(lib, bad2d, connectivity=0), lambda: ops_raw.ccl_label_roots(lib, bad2d, connectivity=0),
                 lambda: PP.component_roots(bad2d, connectivity=0), lambda: PP.label(bad2d, connectivity=0),
                 lambda: PP.binary_fill_holes(bad2d, connectivity=0), lambda: PP.remove_small_components(bad2d, 2, connectivity=0),
                 lambda: PP.largest_connected_domain(bad2d, connectivity=0), lambda: PP.component_summary(bad2d, connectivity=0),
                 lambda: PP.postprocess_labels(bad2d, connectivity=0), lambda: PP.label_component_roots(bad2d, connectivity=0),
                 lambda: PP.keep_largest_per_class(bad2d, connectivity=0), lambda: PP.class_component_summary(bad2d, connectivity=0)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(RuntimeError):
        PP.label(bad2d, connectivity=3)                                   # the other refusals stay what they are
    with pytest.raises(RuntimeError):
        ops_raw.ccl_roots(lib, ok.int(), connectivity=3)
    with pytest.raises(RuntimeError):
        ops_raw.ccl_label_roots(lib, ok[0], connectivity=2)
    with pytest.raises(RuntimeError):
        ops_raw.ccl_roots(lib, ok, bit=8, connectivity=2)


def check_c_refusals(lib, dev):
    """every C refusal returns its code and launches nothing: the output buffer keeps its fill, at every connectivity"""
    dll = lib.dll
    buf = torch.full((128,), FILL, dtype=torch.int64, device=dev)
    marks = torch.full((1024,), FILL, dtype=torch.int64, device=dev)
    assert dll.segm_ccl_roots_conn(None) == -1 and dll.segm_ccl_label_roots_conn(None) == -1
    for conn in (1, 2, 3):
        for a, vol in ((L.CclRootsConnArgs(), "volume"), (L.CclLabelRootsConnArgs(), "labels")):
            entry = dll.segm_ccl_roots_conn if vol == "volume" else dll.segm_ccl_label_roots_conn
            if vol == "volume":
                a.bit = -1
            a.connectivity = conn
            assert entry(a) == -1                                         # SEGM_E_NULL
            setattr(a, vol, buf.data_ptr())
            assert entry(a) == -1                                         # no roots
            a.roots = marks.data_ptr()
            setattr(a, vol, None)
            assert entry(a) == -1                                         # no volume
            setattr(a, vol, buf.data_ptr())
            assert entry(a) == -2                                         # SEGM_E_SHAPE: no size
            a.depth, a.height, a.width = 2048, 1024, 1024
            assert entry(a) == -2                                         # 2^31 voxels
            a.depth, a.height, a.width = 65536, 65536, 1
            assert entry(a) == -2
            a.depth, a.height, a.width = 2, 2, -2
            assert entry(a) == -2
            a.depth, a.height, a.width = 2, 2, 2
            a.workspace, a.workspace_bytes = marks.data_ptr() + 512, 32
            for bad in (0, 4, -1, 26):
                a.connectivity = bad
                assert entry(a) == -2, bad                                # the connectivity, everything else in order
            a.connectivity = conn
            if vol == "volume":
                for bit, inv in ((8, 0), (-2, 0), (0, 2), (0, -1)):
                    a.bit, a.invert = bit, inv
                    assert entry(a) == -2, (bit, inv)
                a.bit, a.invert = -1, 0
            a.roots = marks.data_ptr() + 2
            assert entry(a) == -2                                         # misaligned roots
            a.roots = marks.data_ptr()
            a.workspace, a.workspace_bytes = None, 32
            assert entry(a) == -6                                         # SEGM_E_WORKSPACE: none
            a.workspace, a.workspace_bytes = marks.data_ptr() + 512, 31
            assert entry(a) == -6                                         # one byte short
            a.workspace, a.workspace_bytes = marks.data_ptr() + 514, 32
            assert entry(a) == -6                                         # misaligned
    if str(dev) != "cpu":
        torch.cuda.synchronize()
    assert bool((marks == FILL).all()) and bool((buf == FILL).all())      # nothing was launched
    a = L.CclRootsConnArgs()                                              # and the call in order runs
    a.depth, a.height, a.width, a.bit, a.connectivity = 2, 2, 2, -1, 3
    a.volume, a.roots, a.workspace, a.workspace_bytes = buf.data_ptr(), marks.data_ptr(), marks.data_ptr() + 512, 32
    assert dll.segm_ccl_roots_conn(a) == 0
    if str(dev) != "cpu":
        torch.cuda.synchronize()
    assert marks[:4].view(torch.int32).tolist() == [0] * 8 and bool((marks[4:64] == FILL).all())


def check_exports(lib):
    header = open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()      # additive: the ABI number stays
    for struct, cls in (("segm_ccl_roots_conn_args", L.CclRootsConnArgs), ("segm_ccl_label_roots_conn_args", L.CclLabelRootsConnArgs)):
        body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [f.strip().split()[-1].lstrip("*") for decl in body.split(";") for f in decl.split(",") if f.strip()]
        assert fields == [f[0] for f in cls._fields_], (struct, fields)
    assert [f[0] for f in L.CclRootsArgs._fields_][5] == "reserved" and L.CclRootsConnArgs._fields_[5][0] == "connectivity"
    import ctypes
    assert ctypes.sizeof(L.CclRootsConnArgs) == ctypes.sizeof(L.CclRootsArgs)
    assert ctypes.sizeof(L.CclLabelRootsConnArgs) == ctypes.sizeof(L.CclLabelRootsArgs)


# ---- 5. the predictor and the tool ----------------------------------------------------------------------------------------------------------
def check_predictor(dev, tmp_path):
    from segmamba_amd.predictor import Predictor
    lab = CR.labels("diagonal_island")
    p = Predictor(None)
    for c, ones in ((1, 54), (3, 56)):
        q = p.save_to_nii(dev_t((lab == 1).astype(np.uint8), dev), (1, 1, 1), str(tmp_path / f"one{c}"), "organ", postprocess=True, connectivity=c)
        assert int(nifti.read_nifti(q)[0].sum()) == ones
        paths = p.save_organs_to_nii(dev_t(lab, dev), (1, 1, 1), str(tmp_path / f"organs{c}"), ["a", "b"], postprocess=True, connectivity=c)
        got = [nifti.read_nifti(q)[0] for q in paths]
        assert int(got[0].sum()) == ones and int(got[1].sum()) == 60
    q = p.save_to_nii(dev_t((lab == 1).astype(np.uint8), dev), (1, 1, 1), str(tmp_path / "default"), "organ", postprocess=True)
    assert int(nifti.read_nifti(q)[0].sum()) == 54
    with pytest.raises(ValueError):
        p.save_to_nii(dev_t((lab == 1).astype(np.uint8), dev), (1, 1, 1), str(tmp_path / "bad"), "organ", postprocess=True, connectivity=4)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    return tool


def check_tool(dev, tmp_path):
    """tools/finish_predictions.py --per-class --connectivity 3 keeps the diagonal island that the default (and --connectivity 1)
    removes; --postprocess takes the flag too; a value outside 1 .. 3 is refused by the parser"""
    finish = _tool("finish_predictions")
    lab = CR.labels("diagonal_island")
    (tmp_path / "logits").mkdir()
    np.save(tmp_path / "logits" / "case0.npy", np.stack([(lab == k) for k in range(3)]).astype(np.float32) * 3.0)
    out = {}
    for key, extra in (("default", []), ("c1", ["--connectivity", "1"]), ("c3", ["--connectivity", "3"])):
        written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / key), "--per-class"] + extra)
        assert [os.path.basename(w) for w in written] == ["case0.nii.gz"]
        out[key] = nifti.read_nifti(written[0])[0]
    assert np.array_equal(out["default"], out["c1"])
    assert np.array_equal(out["default"], LR.select(lab, CR.labels_roots("diagonal_island", 1), "largest"))
    assert np.array_equal(out["c3"], LR.select(lab, CR.labels_roots("diagonal_island", 3), "largest"))
    assert out["default"][4, 4, 64] == 0 and out["c3"][4, 4, 64] == 1 and out["c3"][4, 4, 65] == 1 and out["c3"][1, 7, 40] == 0
    for c in (1, 3):
        written = finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / f"pp{c}"), "--postprocess",
                               "--connectivity", str(c)])
        want = PP.postprocess_labels(dev_t(lab, dev), connectivity=c).cpu().numpy()
        assert np.array_equal(nifti.read_nifti(written[0])[0], want)
    with pytest.raises(SystemExit):
        finish.main(["--logits", str(tmp_path / "logits"), "--out", str(tmp_path / "no"), "--per-class", "--connectivity", "4"])
