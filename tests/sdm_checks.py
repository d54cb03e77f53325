"""Checks shared by tests/test_emu_sdm.py (kernel sources on the CPU emulator) and tests/test_gpu_sdm.py (the HIP library):
`segm_sdm_masks` and `segm_sdm_compose` (csrc/sdm.hip) and the host module segmamba_amd/sdm.py against tests/sdm_ref.py, the numpy
float64 restatement of the reference's dataset_sdm_edge.py.  Every function takes the loaded library and / or the device its tensors
live on; the host functions find the library through segmamba_amd.lib.

Acceptance: inside, outside, edge, boundary and counts exactly; sdf and sdm within one fp32 ulp of the fp32-rounded restatement,
per element |got - fl32(ref)| <= numpy.spacing(|fl32(ref)|) - the restatement's distances are correctly rounded float64 roots of
exact integers and its quotient is one float64 division, the device's fp64 sqrt and division may move the single rounding to fp32 by
one step and no more; exactly 0 on boundary voxels, exactly +-1 where the restatement has +-1, all-zero sdf on dead planes; two calls
bit-equal."""
import contextlib
import ctypes
import importlib.util
import os
import pickle
import re

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import metrics as M
from segmamba_amd import ops_raw
from segmamba_amd import sdm as T
from segmamba_amd.dataloading import CaseDataset, PatchLoader
from tests import preprocess_ref as PR
from tests import sdm_ref as S

NEW_EXPORTS = ("segm_sdm_masks", "segm_sdm_compose")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BRATS = S.BRATS_REGIONS
EIGHT = ((1,), (2,), (3,), (1, 2), (1, 3), (2, 3), (1, 2, 3), (4, 1))       # every bit of the table's bytes
SHAPES_X = [(d, h, w) for w in (63, 64, 65) for d, h in ((3, 4), (4, 5), (5, 3))]


def dev_t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@contextlib.contextmanager
def no_sync(dev):
    """on the GPU: any device-to-host copy or wait inside raises"""
    if str(dev).startswith("cuda"):
        torch.cuda.set_sync_debug_mode("error")
        try:
            yield
        finally:
            torch.cuda.set_sync_debug_mode("default")
    else:
        yield


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def fixture_labels():
    """the case of tests/golden/sdm_edge.npz: 9 x 10 x 24 int16, WT touches the faces z = 0 and x = 23, one voxel of -1"""
    v = np.zeros((9, 10, 24), np.int16)
    v[1:8, 1:9, 2:20] = 2
    v[2:7, 2:8, 4:16] = 1
    v[3:6, 3:7, 6:12] = 3
    v[0:3, 0:4, 20:24] = 2
    v[8, 9, 0] = -1
    return v


def random_labels(shape, seed, dtype=np.uint8):
    """boxes of the labels 1 - 3 and a sprinkle of single voxels, labels 0 - 4"""
    rng = np.random.RandomState(seed)
    v = np.zeros(shape, dtype)
    for _ in range(6):
        lo = [rng.randint(0, s) for s in shape]
        hi = [min(s, a + 1 + rng.randint(0, max(1, s // 2 + 1))) for a, s in zip(lo, shape)]
        v[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.randint(1, 4)
    sprinkle = rng.rand(*shape) < 0.03
    v[sprinkle] = rng.randint(0, 5, size=int(sprinkle.sum()))
    return v


def named_case(name):
    """-> (labels (n, D, H, W), regions)"""
    if name == "fixture":
        return fixture_labels()[None], BRATS
    if name == "1x1x1":                                                    # TC and WT full, ET empty
        return np.ones((1, 1, 1, 1), np.uint8), BRATS
    if name == "touches_every_face":                                       # WT reaches all six faces, a hole in its middle
        v = np.full((7, 8, 9), 2, np.uint8)
        v[3, 3:5, 3:6] = 0
        v[2:5, 1:3, 1:4] = 1
        return v[None], BRATS
    if name == "single_voxel":
        v = np.zeros((5, 6, 7), np.uint8)
        v[2, 3, 4] = 3
        return v[None], BRATS
    if name == "two_voxel_slab":                                           # no voxel off the inner boundary: the reference's assert fails
        v = np.zeros((6, 7, 9), np.uint8)
        v[2:4] = 1
        return v[None], BRATS
    if name == "empty_and_full":                                           # label 2 everywhere: TC and ET empty, WT full
        return np.full((1, 4, 5, 6), 2, np.uint8), BRATS
    if name == "eight_regions":
        return random_labels((6, 7, 20), 8)[None], EIGHT
    if name == "far_corner":                                               # 40 x 40 x 41 = 64 full workgroups of 1024 voxels and one of 64:
        v = np.zeros((40, 40, 41), np.uint8)                               # the farthest voxel from the region is the last voxel
        v[0, 0, 0] = 1
        return v[None], ((1,),)
    if name == "long_row":                                                 # a side beyond 256: segm_edt_sq_long
        v = np.zeros((2, 3, 300), np.uint8)
        v[:, :, 0] = 1
        v[1, 1:3, 296:299] = 3
        return v[None], BRATS
    raise KeyError(name)


NAMED = ("fixture", "1x1x1", "touches_every_face", "single_voxel", "two_voxel_slab", "empty_and_full", "eight_regions", "far_corner",
         "long_row")


# ---- the restatement as bit volumes ------------------------------------------------------------------------------------------------------
def ref_masks(labels, regions):
    """-> bits (4, n, D, H, W) uint8 and counts (n, 8) int64 from tests/sdm_ref.py, region r in bit r"""
    labels = np.asarray(labels)
    bits = np.zeros((4,) + labels.shape, np.uint8)
    counts = np.zeros((labels.shape[0], 8), np.int64)
    for v, vol in enumerate(labels):
        for r, reg in enumerate(regions):
            m = np.isin(vol, list(reg))
            bits[0, v] |= m.astype(np.uint8) << r
            bits[1, v] |= (~m).astype(np.uint8) << r
            bits[2, v] |= S.get_edge_points(m).astype(np.uint8) << r
            bits[3, v] |= S.find_boundaries_inner(m).astype(np.uint8) << r
            counts[v, r] = int(m.sum())
    return bits, counts


def assert_within_one_ulp(got, ref64, what):
    want = np.asarray(ref64, np.float64).astype(np.float32)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = np.spacing(np.abs(want)).astype(np.float64)
    worst = float((err / tol).max()) if err.size else 0.0
    print(what, "max |got - fl32(ref)| in ulp of the reference:", worst, "elements off by one step:", int((err > 0).sum()), "of", err.size)
    assert (err <= tol).all(), (what, worst)


def run_raw(lib, labels_t, regions):
    """one group through the raw wrappers: masks, the distance transform routed by size, compose with all three outputs"""
    n, shape = labels_t.shape[0], tuple(labels_t.shape[1:])
    R = len(regions)
    assert n * R <= L.METRICS_MAX_PLANES // 2
    bits, counts = ops_raw.sdm_masks(lib, labels_t, M._table(regions, labels_t.device), R)
    seeds = bits[:2].reshape((2 * n,) + shape)
    pairs = [(v, r) for v in range(n) for r in range(R)]
    planes = [pl for v, r in pairs for pl in ((n + v, r), (v, r))]
    edt = M._edt_sq(lib, seeds, planes, None, "")
    outs = [torch.full((n * R,) + shape, 7.0, dtype=torch.float32, device=labels_t.device) for _ in range(3)]
    ops_raw.sdm_compose(lib, bits, counts, edt, [(v, r, 2 * i, 2 * i + 1, i) for i, (v, r) in enumerate(pairs)], *outs)
    return bits, counts, edt, outs


def compare_targets(labels, regions, sdf, sdm, edge, what):
    """sdf, sdm, edge (n, R, D, H, W) numpy fp32 against the restatement"""
    ref_edge, ref_sdf, ref_sdm = S.targets(labels, regions)
    assert np.array_equal(edge, ref_edge.astype(np.float32)), what
    assert_within_one_ulp(sdf, ref_sdf, what + " sdf")
    assert_within_one_ulp(sdm, ref_sdm, what + " sdm")
    for v in range(labels.shape[0]):
        for r, reg in enumerate(regions):
            m = np.isin(labels[v], list(reg))
            bnd = S.find_boundaries_inner(m)
            assert not sdf[v, r][bnd].any(), (what, v, r, "boundary voxels are exactly 0")
            if not m.any() or m.all():
                assert not sdf[v, r].any() and np.array_equal(sdm[v, r], 1.0 + edge[v, r]), (what, v, r, "dead plane")
            else:
                for ext in (-1.0, 1.0):
                    at = ref_sdf[v, r] == ext
                    assert (sdf[v, r][at] == np.float32(ext)).all(), (what, v, r, ext)
                assert sdf[v, r].min() >= -1.0 and sdf[v, r].max() <= 1.0


# ---- 1. the two entries ----------------------------------------------------------------------------------------------------------------
def check_case(lib, dev, labels, regions, what):
    labels = np.asarray(labels)
    n, R = labels.shape[0], len(regions)
    t = dev_t(labels, dev)
    bits, counts, edt, outs = run_raw(lib, t, regions)
    want_bits, want_counts = ref_masks(labels, regions)
    got_bits = bits.cpu().numpy()
    for k, name in enumerate(("inside", "outside", "edge", "boundary")):
        assert np.array_equal(got_bits[k], want_bits[k]), (what, name)
    assert np.array_equal(counts.cpu().numpy(), want_counts), (what, counts.tolist(), want_counts.tolist())
    assert not (want_bits[3] & ~want_bits[2]).any()                        # boundary is a subset of edge
    shape5 = (n, R) + labels.shape[1:]
    sdf, sdm, edge = (o.cpu().numpy().reshape(shape5) for o in outs)
    compare_targets(labels, regions, sdf, sdm, edge, what)
    _, _, _, again = run_raw(lib, t, regions)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, again)), (what, "two calls are bit-equal")
    return want_bits, want_counts, sdf, sdm, edge


def check_named(lib, dev, name):
    labels, regions = named_case(name)
    bits, counts, sdf, sdm, edge = check_case(lib, dev, labels, regions, name)
    if name == "fixture":
        wt_edge, wt_bnd = (bits[2, 0] >> 1) & 1, (bits[3, 0] >> 1) & 1
        assert int(wt_edge.sum()) == 568 and int(wt_bnd.sum()) == 554 and int((wt_edge & ~wt_bnd).sum()) == 14
        assert float(sdm.min()) == 0.0 and float(sdm.max()) == 2.75
        assert all(S.asserts_hold(sdf[0, r].astype(np.float64)) for r in range(3))
    if name == "two_voxel_slab":
        assert not S.asserts_hold(sdf[0, 0].astype(np.float64)) and sdf[0, 0].min() == 0.0 and sdf[0, 0].max() == 1.0
    if name == "far_corner":
        assert sdf[0, 0, 39, 39, 40] == 1.0 and sdf[0, 0, 0, 0, 0] == 0.0
    if name == "eight_regions":
        assert (counts[0] > 0).all()
    if name == "long_row":
        assert max(labels.shape) > L.EDT_MAX_LINE and sdf[0, 1].max() == 1.0


def check_shape(lib, dev, shape):
    """widths on either side of a wave's 64 lanes; 4 | N takes packets, the others single voxels in the planes after the first"""
    check_case(lib, dev, random_labels(shape, sum(shape))[None], BRATS, f"random {shape}")


def check_dtypes(lib, dev):
    """uint8, int16 and int64 labels give the same bits; -1 and 300 belong to no region (300 must not alias 300 - 256 = 44 -> here 1)"""
    base = random_labels((5, 6, 33), 77, np.int64)
    tab = dev_t(np.zeros(256, np.uint8), dev)
    tab[1], tab[2], tab[3], tab[44] = 3, 2, 7, 1
    want = None
    for dt in (np.uint8, np.int16, np.int64):
        v = base.astype(dt)
        bits, counts = ops_raw.sdm_masks(lib, dev_t(v[None], dev), tab, 3)
        if want is None:
            want = (bits, counts)
        assert torch.equal(bits, want[0]) and torch.equal(counts, want[1]), dt
    for dt in (np.int16, np.int64):
        v = base.astype(dt)
        v[0, 0, :5], v[4, 5, -3:], v[2, 3, 10:14] = -1, 300, (-32768 if dt == np.int16 else -2 ** 40)
        clean = np.where((v < 0) | (v > 255), 0, v).astype(np.uint8)
        a = ops_raw.sdm_masks(lib, dev_t(v[None], dev), tab, 3)
        b = ops_raw.sdm_masks(lib, dev_t(clean[None], dev), tab, 3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), dt
        check_case(lib, dev, v[None], BRATS, f"labels {np.dtype(dt).name} with -1 and 300")


def check_offset_pointers(lib, dev):
    """labels, transforms and outputs that start one element into their buffers: nothing is 16-byte aligned, the voxel route runs, and
    the results equal those of the aligned call bit for bit"""
    labels = random_labels((4, 6, 16), 5, np.int16)[None]                 # 384 voxels: a multiple of 4
    t = dev_t(labels, dev)
    bits, counts, edt, outs = run_raw(lib, t, BRATS)
    shifted = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)[1:].view(t.shape)
    shifted.copy_(t)
    b2, c2 = ops_raw.sdm_masks(lib, shifted, M._table(BRATS, t.device), 3)
    assert torch.equal(b2, bits) and torch.equal(c2, counts)
    e2 = torch.zeros(edt.numel() + 1, dtype=edt.dtype, device=dev)[1:].view(edt.shape)
    e2.copy_(edt)
    o2 = [torch.zeros(o.numel() + 1, dtype=o.dtype, device=dev)[1:].view(o.shape) for o in outs]
    assert all(o.data_ptr() % 16 == 4 for o in o2) or str(dev) == "cpu"
    ops_raw.sdm_compose(lib, bits, counts, e2, [(0, r, 2 * r, 2 * r + 1, r) for r in range(3)], *o2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs, o2))
    # each output on its own, and the edge without any transform
    for k in range(3):
        one = [None, None, None]
        one[k] = torch.empty_like(outs[k])
        ops_raw.sdm_compose(lib, bits, counts, None if k == 2 else edt, [(0, r, 2 * r, 2 * r + 1, r) for r in range(3)], *one)
        assert torch.equal(one[k].view(torch.int32), outs[k].view(torch.int32)), k
    # items in another order, to other planes of a larger output
    big = torch.full((5,) + tuple(outs[0].shape[1:]), -3.0, dtype=torch.float32, device=dev)
    ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 2, 4, 5, 0), (0, 0, 0, 1, 4)], sdf=big)
    assert torch.equal(big[0], outs[0][2]) and torch.equal(big[4], outs[0][0]) and bool((big[1:4] == -3.0).all())


# ---- 2. the host module -------------------------------------------------------------------------------------------------------------------
def check_host_groups(dev, n):
    """n volumes x 3 regions: 3, 6 and 15 pairs - the last split at 8 pairs per distance transform"""
    labels = np.stack([random_labels((6, 9, 21), 30 + i, np.int64) for i in range(n)])
    labels[0, 0, 0, :3] = -1
    t = dev_t(labels, dev)
    T.sdm_edge_targets(t)                                                   # the library is loaded, the region table is on the device
    with no_sync(dev):
        edge, sdm = T.sdm_edge_targets(t)
        sdf = T.signed_distance(t)
    assert edge.shape == sdm.shape == sdf.shape == (n, 3, 6, 9, 21) and edge.dtype == sdm.dtype == torch.float32 and edge.device == t.device
    compare_targets(labels, BRATS, sdf.cpu().numpy(), sdm.cpu().numpy(), edge.cpu().numpy(), f"{n} volumes")
    if n == 1:
        e3, s3 = T.sdm_edge_targets(t[0])                                 # (D, H, W) labels
        assert torch.equal(e3, edge) and torch.equal(s3, sdm)
        e8, s8 = T.sdm_edge_targets(labels[0].astype(np.uint8) * (labels[0] > 0))     # a numpy array is uploaded
        assert torch.equal(e8.cpu(), edge.cpu()) and torch.equal(s8.cpu(), sdm.cpu())


def check_many_regions(dev):
    """ten regions: two tables"""
    regions = EIGHT + ((2, 4), (3,))
    labels = random_labels((5, 6, 17), 4)[None]
    edge, sdm = T.sdm_edge_targets(dev_t(labels, dev), regions)
    sdf = T.signed_distance(dev_t(labels, dev), regions)
    assert tuple(edge.shape) == (1, 10, 5, 6, 17)
    compare_targets(labels, regions, sdf.cpu().numpy(), sdm.cpu().numpy(), edge.cpu().numpy(), "ten regions")


def check_reference_names(dev):
    """convert_labels, get_edge_points, edge_3d, compute_sdf: the mask-taking forms equal the label route and the restatement"""
    labels = fixture_labels()
    t = dev_t(labels, dev)
    seg = T.convert_labels(t)
    assert tuple(seg.shape) == (1, 3) + labels.shape and seg.dtype == torch.float32
    assert np.array_equal(seg.cpu().numpy(), S.convert_labels(labels).astype(np.float32))
    edge, sdm = T.sdm_edge_targets(t)
    sdf = T.signed_distance(t)
    T.edge_3d(seg)
    with no_sync(dev):
        e = T.edge_3d(seg)
        f = T.compute_sdf(seg, out_shape=seg.shape)
        p = T.get_edge_points(seg[0, 1])
    assert torch.equal(e, edge) and torch.equal(f, sdf) and torch.equal(p, edge[0, 1])
    assert torch.equal(1 - T.compute_sdf(seg.cpu().numpy()).double() + e.double(), 1 - sdf.double() + edge.double())
    assert np.array_equal(e.cpu().numpy(), S.edge_3d(S.convert_labels(labels)).astype(np.float32))
    assert_within_one_ulp(f.cpu().numpy(), S.compute_sdf(S.convert_labels(labels)), "compute_sdf on masks")
    assert_within_one_ulp(sdm.cpu().numpy(), 1 - S.compute_sdf(S.convert_labels(labels)) + S.edge_3d(S.convert_labels(labels)), "seg_sdm")
    for call in (lambda: T.get_edge_points(seg[0, 0, 0]), lambda: T.edge_3d(seg[0]), lambda: T.compute_sdf(seg[:, :, 0]),
                 lambda: T.sdm_edge_targets(t[0]), lambda: T.signed_distance(t[0])):
        with pytest.raises(ValueError):
            call()
    for call in (lambda: T.compute_sdf(seg, out_shape=(1, 3, 9, 10, 23)), lambda: T.edge_3d(seg[0, 0]), lambda: T.sdm_edge_targets(t[None, None]),
                 lambda: T.sdm_edge_targets(t, ()), lambda: T.sdm_edge_targets(t, ((256,),)),
                 lambda: T.sdm_edge_targets(t.float()), lambda: T.signed_distance(t.double())):        # float labels are refused
        with pytest.raises(RuntimeError):
            call()
    # labels outside 0 .. 255 are in no region on both routes: 300 must not become 44, -1 not 255
    wide = labels.astype(np.int64)
    wide[4, 4, 8:10], wide[0, 0, 0] = 300, -1
    wide[1, 1, 2:4] = 256 + 3
    got = T.convert_labels(dev_t(wide, dev))
    assert np.array_equal(got.cpu().numpy(), S.convert_labels(wide).astype(np.float32))
    assert torch.equal(T.edge_3d(got), T.sdm_edge_targets(dev_t(wide, dev))[0])


def check_loader(dev, augment):
    """next_with_targets(): the targets of an augmented batch are the targets of the label it returns; next() is what it was"""
    resident = [{"data": dev_t(it["data"], dev), "seg": dev_t(it["seg"], dev), "properties": it["properties"]}
                for it in PR.patch_standin_dataset()]                       # cases in device memory, as CaseDataset keeps them

    def loader(**kw):
        return PatchLoader(resident, PR.PATCH_SIZE, batch_size=2, device=dev, augment=augment, seed=3, **kw)
    with pytest.raises(RuntimeError, match="targets"):
        loader(targets="sdm")
    with pytest.raises(RuntimeError, match="targets"):
        loader().next_with_targets()
    np.random.seed(1)
    want_image, want_label = loader().next()
    np.random.seed(1)
    loader(targets="sdm_edge").next_with_targets()                          # warm: library, table, allocator
    np.random.seed(1)
    ld = loader(targets="sdm_edge")
    with no_sync(dev):
        image, label, edge, sdm = ld.next_with_targets()
    assert torch.equal(image, want_image) and torch.equal(label, want_label)
    e2, s2 = T.sdm_edge_targets(label)
    assert torch.equal(edge, e2) and torch.equal(sdm, s2) and tuple(edge.shape) == (2, 3) + tuple(PR.PATCH_SIZE)
    ref_edge, _, ref_sdm = S.targets(label.cpu().numpy(), BRATS)
    assert np.array_equal(edge.cpu().numpy(), ref_edge.astype(np.float32))
    assert_within_one_ulp(sdm.cpu().numpy(), ref_sdm, "loader sdm")
    one = PatchLoader(PR.patch_standin_dataset(), PR.PATCH_SIZE, batch_size=2, device=dev, targets="sdm_edge", regions=((2,),))
    assert tuple(one.next_with_targets()[3].shape) == (2, 1) + tuple(PR.PATCH_SIZE)


def check_tool_and_dataset(dev, tmp_path):
    """tools/make_sdm_targets.py writes <case>_seg_sdm.npy, (1, 3, X, Y, Z) float32, from .npz and from _seg.npy; CaseDataset(sdm_dir=...)
    appends its [0] to the seg"""
    spec = importlib.util.spec_from_file_location("make_sdm_targets_tool", os.path.join(ROOT, "tools", "make_sdm_targets.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    data, out = tmp_path / "data", tmp_path / "sdm"
    data.mkdir()
    paths = []
    items = PR.patch_standin_dataset()[:3]
    for i, item in enumerate(items):
        stem = os.path.join(str(data), item["properties"]["name"])
        if i == 1:
            np.save(stem + "_seg.npy", item["seg"])                        # the unpacked form alone
        np.savez_compressed(stem + ".npz", data=item["data"], seg=item["seg"] if i != 1 else np.zeros_like(item["seg"]))
        with open(stem + ".pkl", "wb") as f:
            pickle.dump(item["properties"], f)
        paths.append(stem + ".npz")
    written = tool.main(["--data", str(data), "--out", str(out), "--device", str(dev)])
    assert sorted(os.path.basename(w) for w in written) == [f"case_{i}_seg_sdm.npy" for i in range(3)]
    for i, item in enumerate(items):
        a = np.load(out / f"case_{i}_seg_sdm.npy")
        assert a.dtype == np.float32 and a.shape == (1, 3) + item["seg"].shape[1:]
        assert_within_one_ulp(a[0], S.targets(item["seg"], BRATS)[2][0], f"case_{i} file")
    wide = tool.main(["--data", str(data), "--out", str(tmp_path / "wide"), "--float64", "--device", str(dev)])
    b = np.load(wide[0])
    assert b.dtype == np.float64 and np.array_equal(b, np.load(out / "case_0_seg_sdm.npy").astype(np.float64))
    plain = CaseDataset(paths, device=dev)
    ds = CaseDataset(paths, device=dev, sdm_dir=str(out))
    for i in (0, 2):
        seg, want = ds[i]["seg"], plain[i]["seg"]
        assert seg.dtype == torch.float32 and tuple(seg.shape) == (4,) + tuple(want.shape[1:]) and tuple(want.shape[:1]) == (1,)
        assert torch.equal(seg[:1], want.float())
        assert np.array_equal(seg[1:].cpu().numpy(), np.load(out / f"case_{i}_seg_sdm.npy")[0])
    batch = PatchLoader(ds, PR.PATCH_SIZE, batch_size=2, device=dev).next_batch()
    assert tuple(batch["seg"].shape) == (2, 4) + tuple(PR.PATCH_SIZE)


# ---- 3. refusals (nothing is launched) and exports --------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    labels = dev_t(random_labels((4, 5, 6), 1)[None], dev)
    tab = M._table(BRATS, labels.device)
    bits, counts, edt, outs = run_raw(lib, labels, BRATS)
    items = [(0, r, 2 * r, 2 * r + 1, r) for r in range(3)]
    keep = [o.clone() for o in outs]
    bad = [
        lambda: ops_raw.sdm_masks(lib, labels[0], tab, 3),                                           # no volume dimension
        lambda: ops_raw.sdm_masks(lib, labels.int(), tab, 3),                                         # dtype
        lambda: ops_raw.sdm_masks(lib, labels.float(), tab, 3),
        lambda: ops_raw.sdm_masks(lib, labels[..., ::2], tab, 3),                                     # not contiguous
        lambda: ops_raw.sdm_masks(lib, labels.repeat(17, 1, 1, 1), tab, 3),                           # 17 volumes
        lambda: ops_raw.sdm_masks(lib, labels[:0], tab, 3),
        lambda: ops_raw.sdm_masks(lib, labels, tab, 0),
        lambda: ops_raw.sdm_masks(lib, labels, tab, 9),
        lambda: ops_raw.sdm_masks(lib, labels, tab[:255], 3),
        lambda: ops_raw.sdm_masks(lib, labels, tab.long(), 3),
        lambda: ops_raw.sdm_masks(lib, torch.zeros(1, 1, 1, 2049, dtype=torch.uint8, device=dev), tab, 3),      # a side beyond 2048
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, items),                                   # no output
        lambda: ops_raw.sdm_compose(lib, bits[:3], counts, edt, items, *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts[:, :7], edt, items, *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts.int(), edt, items, *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, None, items, *outs),                           # sdf without a transform
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt.float(), items, *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt[:, :3], items, *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [], *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, items * 6, *outs),                        # 18 items
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(1, 0, 0, 1, 0)], *outs),                # volume index
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 8, 0, 1, 0)], *outs),                # bit index
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 0, 6, 1, 0)], *outs),                # plane index
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 0, 0, -1, 0)], *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 0, 0, 1, 3)], *outs),                # output plane index
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 0, 0, 1, 0), (0, 1, 2, 3, 0)], *outs),     # one plane twice
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, [(0, 0, 0, 1)], *outs),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, items, outs[0].double()),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, items, outs[0][:, :3]),
        lambda: ops_raw.sdm_compose(lib, bits, counts, edt, items, outs[0], outs[1][:2]),             # two Q
    ]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f"refusal {i} did not raise")
    # the C entries themselves, without launching
    dll = lib.dll
    assert dll.segm_sdm_masks(None) == -1 and dll.segm_sdm_compose(None) == -1
    assert dll.segm_sdm_masks(L.SdmMasksArgs()) == -1 and dll.segm_sdm_compose(L.SdmComposeArgs()) == -1
    fresh_bits, fresh_counts = torch.full_like(bits, 0x55), torch.full_like(counts, -9)

    def masks_args():
        a = L.SdmMasksArgs()
        a.depth, a.height, a.width, a.n, a.n_regions, a.label_dtype = 4, 5, 6, 1, 3, L.SDM_LABEL_U8
        a.labels, a.table, a.counts = labels.data_ptr(), tab.data_ptr(), fresh_counts.data_ptr()
        a.inside, a.outside, a.edge, a.boundary = (fresh_bits[k].data_ptr() for k in range(4))
        return a
    for field, value, status in (("depth", 0, -2), ("height", -1, -2), ("width", L.EDT_LONG_MAX_LINE + 1, -2), ("n", 0, -2), ("n", 17, -2),
                                 ("n_regions", 0, -2), ("n_regions", 9, -2), ("label_dtype", 3, -4), ("label_dtype", -1, -4),
                                 ("labels", None, -1), ("table", None, -1), ("inside", None, -1), ("outside", None, -1), ("edge", None, -1),
                                 ("boundary", None, -1), ("counts", None, -1), ("counts", fresh_counts.data_ptr() + 4, -2)):
        a = masks_args()
        setattr(a, field, value)
        assert dll.segm_sdm_masks(a) == status, (field, value)
    a = masks_args()                                                                                  # 2048 x 2048 x 257 voxels > 2^30
    a.depth, a.height, a.width = 2048, 2048, 257
    assert dll.segm_sdm_masks(a) == -2
    a = masks_args()                                                                                  # int64 labels at an odd address
    a.label_dtype, a.labels = L.SDM_LABEL_I64, labels.data_ptr() + 4
    assert dll.segm_sdm_masks(a) == -2
    assert bool((fresh_bits == 0x55).all()) and bool((fresh_counts == -9).all())                      # nothing was written
    ws = torch.zeros(L.SDM_COMPOSE_WORKSPACE_BYTES // 4 + 1, dtype=torch.int32, device=dev)

    def compose_args():
        a = L.SdmComposeArgs()
        a.voxels, a.n_items, a.n_volumes, a.n_planes, a.n_out_planes = 120, 3, 1, 6, 3
        for i, (v, b, pp, npl, o) in enumerate(items):
            a.volume[i], a.bit[i], a.pos_plane[i], a.neg_plane[i], a.out_plane[i] = v, b, pp, npl, o
        a.edt, a.inside, a.edge, a.boundary, a.counts = edt.data_ptr(), bits[0].data_ptr(), bits[2].data_ptr(), bits[3].data_ptr(), counts.data_ptr()
        a.sdf, a.sdm, a.edge_out = (o.data_ptr() for o in outs)
        a.workspace, a.workspace_bytes = ws.data_ptr(), L.SDM_COMPOSE_WORKSPACE_BYTES
        return a
    for field, value, status in (("voxels", 0, -2), ("voxels", L.METRICS_MAX_VOXELS + 1, -2), ("n_items", 0, -2), ("n_items", 17, -2),
                                 ("n_volumes", 0, -2), ("n_planes", 0, -2), ("n_planes", 5, -2), ("n_out_planes", 2, -2),
                                 ("edt", None, -1), ("inside", None, -1), ("edge", None, -1), ("boundary", None, -1), ("counts", None, -1),
                                 ("edt", edt.data_ptr() + 2, -2), ("sdf", outs[0].data_ptr() + 2, -2), ("counts", counts.data_ptr() + 4, -2),
                                 ("workspace", None, -6), ("workspace_bytes", L.SDM_COMPOSE_WORKSPACE_BYTES - 1, -6),
                                 ("workspace", ws.data_ptr() + 2, -6)):
        a = compose_args()
        setattr(a, field, value)
        assert dll.segm_sdm_compose(a) == status, (field, value)
    for field, value in (("volume", 1), ("volume", -1), ("bit", 8), ("bit", -1), ("pos_plane", 6), ("neg_plane", -1), ("out_plane", 3),
                         ("out_plane", 1)):
        a = compose_args()
        getattr(a, field)[0] = value
        assert dll.segm_sdm_compose(a) == -2, (field, value)
    a = compose_args()
    a.sdf = a.sdm = a.edge_out = None
    assert dll.segm_sdm_compose(a) == -1                                                              # no output at all
    assert all(torch.equal(o.view(torch.int32), k.view(torch.int32)) for o, k in zip(outs, keep))     # nothing was written
    a = compose_args()                                                                                # the edge alone needs no transform
    a.sdf = a.sdm = a.edt = a.workspace = None                                                        # ... and no workspace
    a.n_planes, a.workspace_bytes = 0, 0
    assert dll.segm_sdm_compose(a) == 0
    assert dll.segm_sdm_compose(compose_args()) == 0 and dll.segm_sdm_masks(masks_args()) == 0
    assert torch.equal(fresh_bits, bits) and torch.equal(fresh_counts, counts)
    assert all(torch.equal(o.view(torch.int32), k.view(torch.int32)) for o, k in zip(outs, keep))


def check_exports(lib):
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()))
    for name in NEW_EXPORTS:
        assert name in declared and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10
    assert ctypes.sizeof(L.SdmMasksArgs) == 6 * 4 + 8 * 8
    assert ctypes.sizeof(L.SdmComposeArgs) == 8 + 4 * 4 + 5 * 64 + 8 * 8 + 3 * 8
    assert L.SDM_COMPOSE_WORKSPACE_BYTES == 2 * L.METRICS_MAX_PLANES * 4
