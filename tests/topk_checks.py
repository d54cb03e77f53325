"""The checks of the top-k cross entropy (csrc/topk_ce.hip through segmamba_amd.ops_raw, train_ops and losses) that the CPU emulation
(tests/test_emu_topk.py) and the GPU (tests/test_gpu_topk.py) share: `lib` is the loaded library, `dev` where the tensors live.
References: tests/topk_ref.py (float64) and the recorded tests/golden/topk_ce.npz.  TEST INFRASTRUCTURE ONLY.

Bounds.  Map: 1e-5 + 1e-6 l per voxel.  For |x| <= 10: x - max rounds to 1.2e-6 (half an ulp of 20), exp2 and log2 are within 2 ulp, at
most 15 additions of terms <= 1 each round to 6e-8 relative of a sum whose log is taken - together 4.3e-6 absolute, plus the rounding
of the result, 6e-8 l; the bound leaves a factor of 2.  Gradients: 1e-6 x max |gradient| in fp32, 2e-3 in fp16, 1e-2 in bf16, the bounds
of test_cross_entropy_matches_torch (the output is rounded to the dtype: 2^-11 and 2^-8 relative).  Select: the threshold bit-equal,
the counts exact, sum_gt within n 2^-52 relative of math.fsum (n fp64 additions of non-negative terms).  Recorded losses: 1e-5
relative (fp32 arithmetic per voxel, fp64 sum)."""
import math
import os

import numpy as np
import torch

from segmamba_amd import lib as L, losses, ops_raw, train_ops
from tests import topk_ref as R

NEW_EXPORTS = ("segm_cross_entropy_map", "segm_cross_entropy_map_bwd", "segm_topk_select", "segm_topk_select_workspace_bytes")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_ce.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
GRAD_TOL = {torch.float32: 1e-6, torch.float16: 2e-3, torch.bfloat16: 1e-2}
SELECT_SIZES = (1, 63, 64, 65, 255, 257, 4097, 70001)
PATTERNS = ("absnorm", "equal", "two", "chain", "edge", "zeros90", "inf", "nan")

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        for i in range(len(R.CASES)):
            assert float(_golden[f"logits_sum_{i}"]) == float(R.case_inputs(i)[0].astype(np.float64).sum()), "the inputs drifted"
    return _golden


def rounded(logits, dtype, dev):
    """-> (the logits as a `dtype` tensor on dev, the same values as a float64 array)"""
    t = torch.from_numpy(logits).to(dtype)
    return t.to(dev), t.double().numpy()


def ign_of(ignore):
    return -100 if ignore is None else ignore


def decode(result):
    """the 32 bytes of topk_select -> (threshold float32 scalar, n_gt, n_eq, sum_gt)"""
    raw = result.cpu().numpy()
    return raw.view(np.float32)[0], int(raw[1]), int(raw[2]), float(raw.view(np.float64)[3])


# ---- 1. the map ---------------------------------------------------------------------------------------------------------------------
def check_map(lib, dev):
    for i, (shape, C, k, ignore) in enumerate(R.CASES):
        logits, labels = R.case_inputs(i)
        y = torch.from_numpy(labels).to(dev)
        for dtype in DTYPES:
            x, x64 = rounded(logits, dtype, dev)
            got = ops_raw.cross_entropy_map(lib, x, y, ign_of(ignore))
            assert got.dtype == torch.float32 and tuple(got.shape) == shape
            want = R.loss_map(x64, labels, ignore)
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            assert (err <= 1e-5 + 1e-6 * want).all(), (i, dtype, float(err.max()))
            if ignore is not None:
                assert (got.cpu().numpy()[labels == ignore] == 0).all() and (labels == ignore).sum() > 0
            again = ops_raw.cross_entropy_map(lib, x, y, ign_of(ignore))
            assert torch.equal(got, again), "two calls differ"


def check_map_wrong_labels(lib, dev):
    """a label outside [0, C) that is not ignored gives NaN at that voxel and nowhere else; the ignored ones give 0"""
    logits, labels = R.case_inputs(0)
    labels = labels.copy()
    flat = labels.reshape(-1)
    flat[3], flat[100], flat[7] = 4, -1, -100
    got = ops_raw.cross_entropy_map(lib, torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev), -100).cpu().numpy().reshape(-1)
    assert np.isnan(got[3]) and np.isnan(got[100]) and got[7] == 0 and np.isnan(got).sum() == 2
    want = R.loss_map(logits, labels, -100).reshape(-1)
    ok = ~np.isnan(want)
    assert np.abs(got[ok] - want[ok]).max() <= 2e-5


# ---- 2. the selection, fed directly ------------------------------------------------------------------------------------------------------
def pattern(name, n, rs):
    base = np.abs(rs.standard_normal(n)).astype(np.float32)
    if name == "absnorm":
        return base
    if name == "equal":
        return np.full(n, 0.75, dtype=np.float32)
    if name == "two":
        return rs.choice(np.array([0.25, 1.5], dtype=np.float32), n)
    if name == "chain":                    # neighbours under np.nextafter: only the last digit pass separates them
        return (np.uint32(0x3f800400) + rs.randint(0, 512, n).astype(np.uint32)).view(np.float32)
    if name == "edge":                     # both sides of a 12-bit bin edge (0x3f7fffff | 0x3f800000)
        return (np.uint32(0x3f800000 - 32) + rs.randint(0, 64, n).astype(np.uint32)).view(np.float32)
    if name == "zeros90":
        return np.where(rs.rand(n) < 0.9, np.float32(0), base).astype(np.float32)
    v = base.copy()
    v[rs.randint(0, n)] = np.inf if name == "inf" else np.nan
    return v


def check_select_one(lib, dev, values, kk, what):
    t = torch.from_numpy(values).to(dev)
    res = ops_raw.topk_select(lib, t, kk)
    thr, n_gt, n_eq, sum_gt = decode(res)
    w_thr, w_gt, w_eq, w_sum = R.select(values, kk)
    assert np.float32(thr).view(np.uint32) == np.float32(w_thr).view(np.uint32), (what, thr, w_thr)
    assert (n_gt, n_eq) == (w_gt, w_eq), (what, n_gt, n_eq, w_gt, w_eq)
    if math.isfinite(w_sum):
        assert abs(sum_gt - w_sum) <= values.size * 2.0 ** -52 * abs(w_sum), (what, sum_gt, w_sum)
    else:
        assert sum_gt == w_sum or (math.isnan(sum_gt) and math.isnan(w_sum)), (what, sum_gt, w_sum)
    return res


def check_select(lib, dev, name, sizes=SELECT_SIZES):
    """one value pattern at every size and every valid kk of {1, 2, n // 10, n - 1, n}"""
    rs = np.random.RandomState(5 + PATTERNS.index(name))
    for n in sizes:
        values = pattern(name, n, rs)
        for kk in sorted({kk for kk in (1, 2, n // 10, n - 1, n) if 1 <= kk <= n}):
            check_select_one(lib, dev, values, kk, (name, n, kk))


def check_select_twice(lib, dev):
    """two calls bit-equal; a view that is not 16-byte aligned (no packets) gives the aligned copy's bits"""
    values = pattern("zeros90", 4097, np.random.RandomState(5))
    a = check_select_one(lib, dev, values, 409, "twice")
    b = check_select_one(lib, dev, values, 409, "twice")
    assert torch.equal(a, b), "two calls differ"
    off = torch.from_numpy(np.concatenate([np.zeros(1, np.float32), values])).to(dev)[1:]          # not 16-byte aligned: no packets
    assert off.is_contiguous() and torch.equal(ops_raw.topk_select(lib, off, 409), a)


# ---- 3. the backward ----------------------------------------------------------------------------------------------------------------------
def check_backward(lib, dev):
    rs = np.random.RandomState(9)
    for i in (0, 1, 2):
        shape, C, k, ignore = R.CASES[i]
        logits, labels = R.case_inputs(i)
        y = torch.from_numpy(labels).to(dev)
        n = labels.size
        kk = R.kk_of(n, k)
        coef = rs.standard_normal(shape).astype(np.float32)
        scale = np.float32(0.37)
        for dtype in DTYPES:
            x, x64 = rounded(logits, dtype, dev)
            D = R.softmax_minus_onehot(x64, labels, ignore)
            lmap = R.loss_map(x64, labels, ignore).astype(np.float32)              # the map the kernel is given: no ambiguity
            tmap = torch.from_numpy(lmap).to(dev)
            sel = ops_raw.topk_select(lib, tmap.view(-1), kk)
            w = R.topk_weight(lmap, kk)
            tcoef, tscale = torch.from_numpy(coef).to(dev), torch.tensor([scale], device=dev)
            combos = {"none": ({}, 1.0), "coef": (dict(coef=tcoef), coef.astype(np.float64)), "scale": (dict(scale=tscale), float(scale)),
                      "topk": (dict(loss_map=tmap, select=sel, kk=kk), w),
                      "all": (dict(coef=tcoef, scale=tscale, loss_map=tmap, select=sel, kk=kk), coef.astype(np.float64) * float(scale) * w)}
            for name, (kw, g) in combos.items():
                got = ops_raw.cross_entropy_map_bwd(lib, x, y, ign_of(ignore), **kw)
                assert got.dtype == dtype and got.shape == x.shape
                want = D * (g if np.isscalar(g) else np.expand_dims(g, 1))
                err = np.abs(got.double().cpu().numpy() - want).max()
                assert err <= GRAD_TOL[dtype] * np.abs(want).max(), (i, dtype, name, err, np.abs(want).max())
                if ignore is not None:
                    assert (got.double().cpu().numpy()[np.broadcast_to(np.expand_dims(labels == ignore, 1), want.shape)] == 0).all()
                assert torch.equal(got, ops_raw.cross_entropy_map_bwd(lib, x, y, ign_of(ignore), **kw)), "two calls differ"


def check_backward_ties_and_wrong_labels(lib, dev):
    """all logits 0: every loss is log(C), every voxel is tied with the threshold and gets (kk - 0) / (n kk) = 1 / n"""
    shape, C = (2, 5, 6, 7), 4
    n = int(np.prod(shape))
    kk = n // 10
    x = torch.zeros((shape[0], C) + shape[1:], device=dev)
    labels = np.random.RandomState(3).randint(0, C, shape).astype(np.int64)
    y = torch.from_numpy(labels).to(dev)
    lmap = ops_raw.cross_entropy_map(lib, x, y)
    sel = ops_raw.topk_select(lib, lmap.view(-1), kk)
    thr, n_gt, n_eq, sum_gt = decode(sel)
    assert (n_gt, n_eq, sum_gt) == (0, n, 0.0) and abs(float(thr) - math.log(C)) <= 1e-6
    got = ops_raw.cross_entropy_map_bwd(lib, x, y, loss_map=lmap, select=sel, kk=kk).double().cpu().numpy()
    want = R.softmax_minus_onehot(np.zeros(x.shape), labels) / n
    assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    # a wrong label: NaN at its voxel (all classes), also where the top-k weight is 0; nowhere else
    logits, labels = R.case_inputs(0)
    labels = labels.copy()
    labels.reshape(-1)[11] = 9
    xx, yy = torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev)
    for kw in ({}, dict(coef=torch.zeros(labels.shape, device=dev))):
        g = ops_raw.cross_entropy_map_bwd(lib, xx, yy, **kw).cpu().numpy()
        bad = np.isnan(g).reshape(2, 4, -1)
        assert bad[0, :, 11].all() and bad.sum() == 4


# ---- 4. refusals, exports ---------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    logits, labels = R.case_inputs(0)
    x, y = torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev)
    out = torch.empty(labels.shape, dtype=torch.float32, device=dev)
    d = torch.empty_like(x)

    def args(**kw):
        a = L.CrossEntropyMapArgs()
        a.batch, a.classes, a.dtype, a.spatial, a.ignore_index = 2, 4, L.dtype_code(x), 210, -100
        a.logits, a.labels, a.loss_map, a.dlogits = x.data_ptr(), y.data_ptr(), out.data_ptr(), d.data_ptr()
        for k_, v in kw.items():
            setattr(a, k_, v)
        return a
    E_NULL, E_SHAPE, E_DTYPE, E_WS = -1, -2, -4, -6
    dll = lib.dll
    assert dll.segm_cross_entropy_map(None) == E_NULL and dll.segm_cross_entropy_map_bwd(None) == E_NULL and dll.segm_topk_select(None) == E_NULL
    assert dll.segm_cross_entropy_map(args(logits=None)) == E_NULL
    assert dll.segm_cross_entropy_map(args(labels=None)) == E_NULL
    assert dll.segm_cross_entropy_map(args(loss_map=None)) == E_NULL
    assert dll.segm_cross_entropy_map(args(classes=17)) == E_SHAPE
    assert dll.segm_cross_entropy_map(args(classes=0)) == E_SHAPE
    assert dll.segm_cross_entropy_map(args(batch=0)) == E_SHAPE
    assert dll.segm_cross_entropy_map(args(spatial=1 << 31)) == E_SHAPE
    assert dll.segm_cross_entropy_map(args(dtype=7)) == E_DTYPE
    assert dll.segm_cross_entropy_map_bwd(args(loss_map=None, dlogits=None)) == E_NULL
    assert dll.segm_cross_entropy_map_bwd(args()) == E_NULL                              # a loss_map without a select
    sel = torch.zeros(4, dtype=torch.int64, device=dev)
    assert dll.segm_cross_entropy_map_bwd(args(select=sel.data_ptr(), kk=0)) == E_SHAPE
    assert dll.segm_cross_entropy_map_bwd(args(select=sel.data_ptr(), kk=421)) == E_SHAPE
    assert dll.segm_cross_entropy_map_bwd(args(dtype=9, loss_map=None)) == E_DTYPE
    assert dll.segm_topk_select_workspace_bytes(0) == 0 and dll.segm_topk_select_workspace_bytes(1 << 31) == 0
    nbytes = dll.segm_topk_select_workspace_bytes(420)
    assert nbytes > 0
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)

    def sargs(**kw):
        a = L.TopkSelectArgs()
        a.values, a.n, a.kk, a.result = out.data_ptr(), 420, 42, sel.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        for k_, v in kw.items():
            setattr(a, k_, v)
        return a
    assert dll.segm_topk_select(sargs(values=None)) == E_NULL and dll.segm_topk_select(sargs(result=None)) == E_NULL
    for bad in (dict(n=0), dict(n=1 << 31), dict(kk=0), dict(kk=421)):
        assert dll.segm_topk_select(sargs(**bad)) == E_SHAPE, bad
    assert dll.segm_topk_select(sargs(workspace=None)) == E_WS
    assert dll.segm_topk_select(sargs(workspace_bytes=nbytes - 1)) == E_WS
    assert dll.segm_topk_select(sargs(workspace=ws.data_ptr() + 4)) == E_WS
    # the wrappers
    import pytest
    with pytest.raises(RuntimeError):
        ops_raw.cross_entropy_map(lib, x, y.int())
    with pytest.raises(RuntimeError):
        ops_raw.topk_select(lib, out.view(-1), 0)
    with pytest.raises(RuntimeError):
        ops_raw.topk_select(lib, out.view(-1).double(), 1)
    with pytest.raises(RuntimeError):
        ops_raw.cross_entropy_map_bwd(lib, x, y, loss_map=out)
    with pytest.raises(RuntimeError):
        ops_raw.cross_entropy_map_bwd(lib, x, y, coef=out.view(-1))


def check_exports(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segmamba_hip.h")).read()
    assert lib.missing == [] and lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name


# ---- 5. the classes on the library ----------------------------------------------------------------------------------------------------------
def _run(fn, logits, target, dtype, dev):
    x = torch.from_numpy(logits).to(dtype).to(dev).requires_grad_(True)
    loss = fn(x, target.to(dev))
    loss.backward()
    return float(loss.detach()), x.grad.double().cpu().numpy()


def check_classes_recorded(dev, dtypes=DTYPES):
    """TopKLoss and DC_and_topk_loss(weight_dice=0) against the recording: loss 1e-5 relative in fp32, gradient at the dtype's bound.
    For the 16-bit dtypes the reference is the restatement on the rounded logits (the recording is of the fp32 logits), at every voxel
    whose float64 loss is further than 1e-4 from the threshold."""
    g = golden()
    for i, (shape, C, k, ignore) in enumerate(R.CASES):
        logits, labels = R.case_inputs(i)
        target = torch.from_numpy(labels).float().unsqueeze(1)
        for dtype in dtypes:
            keep = 1.0
            if dtype == torch.float32:
                w_loss, w_grad = float(g[f"loss_{i}"]), g[f"grad_{i}"].astype(np.float64)
            else:
                # the rounded logits may bring a loss close to the threshold: such a voxel's selection is not compared
                x64 = torch.from_numpy(logits).to(dtype).double().numpy()
                w_loss, w_grad = R.topk_loss(x64, labels, k, ignore)
                m = R.loss_map(x64, labels, ignore)
                near = np.abs(m - R.select(m, R.kk_of(m.size, k))[0]) <= 1e-4
                assert near.sum() <= 4 + (0 if ignore is None else (labels == ignore).sum())
                keep = np.expand_dims(~near | (False if ignore is None else labels == ignore), 1)
            fns = (losses.TopKLoss(k=k, ignore_index=ign_of(ignore)),
                   losses.DC_and_topk_loss({}, dict(k=k), weight_ce=1, weight_dice=0, ignore_label=ignore))
            for fn in fns:
                loss, grad = _run(fn, logits, target, dtype, dev)
                assert abs(loss - w_loss) <= 1e-5 * abs(w_loss), (i, dtype, loss, w_loss)
                assert (np.abs(grad - w_grad) * keep).max() <= GRAD_TOL[dtype] * np.abs(w_grad).max(), (i, dtype, np.abs(grad - w_grad).max())
            # (B, *spatial) integer targets take the same path
            loss2, grad2 = _run(fns[0], logits, torch.from_numpy(labels), dtype, dev)
            assert loss2 == loss and np.array_equal(grad2, grad)


def check_reductions(dev):
    """cross_entropy(reduction="none" / "sum") and their gradients against ATen in float64; "mean" unchanged"""
    import torch.nn.functional as F
    for i in (0, 1):
        shape, C, k, ignore = R.CASES[i]
        logits, labels = R.case_inputs(i)
        y = torch.from_numpy(labels)
        x64 = torch.from_numpy(logits).double().requires_grad_(True)
        up = torch.from_numpy(np.random.RandomState(4).standard_normal(shape))
        want_map = F.cross_entropy(x64, y, ignore_index=ign_of(ignore), reduction="none")
        (want_map * up).sum().backward()
        x = torch.from_numpy(logits).to(dev).requires_grad_(True)
        got = train_ops.cross_entropy(x, y.to(dev), ign_of(ignore), reduction="none")
        (got * up.float().to(dev)).sum().backward()
        assert got.dtype == torch.float32 and tuple(got.shape) == shape
        assert (np.abs(got.detach().cpu().double().numpy() - want_map.detach().numpy()) <= 1e-5 + 1e-6 * want_map.detach().numpy()).all()
        assert (x.grad.cpu().double() - x64.grad).abs().max() <= 1e-6 * x64.grad.abs().max()
        x64.grad = None
        want_map = F.cross_entropy(x64, y, ignore_index=ign_of(ignore), reduction="none")
        (3.0 * want_map.sum()).backward()
        x2 = torch.from_numpy(logits).to(dev).requires_grad_(True)
        s = train_ops.CrossEntropyLoss(ign_of(ignore), "sum")(x2, y.to(dev))
        (3.0 * s).backward()
        assert abs(float(s.detach()) - float(want_map.detach().sum())) <= 1e-5 * float(want_map.detach().sum())
        assert (x2.grad.cpu().double() - x64.grad).abs().max() <= 1e-6 * x64.grad.abs().max()


def check_mean_route_bits(lib, dev):
    """cross_entropy(reduction="mean") is ops_raw.cross_entropy's route: the same bits, value and gradient"""
    logits, labels = R.case_inputs(1)
    y = torch.from_numpy(labels).to(dev)
    for dtype in DTYPES:
        x = torch.from_numpy(logits).to(dtype).to(dev).requires_grad_(True)
        loss = train_ops.cross_entropy(x, y, 3, reduction="mean")
        loss.backward()
        loss_sum, count, dlogits = ops_raw.cross_entropy(lib, x.detach(), y, 3)
        assert torch.equal(loss.detach(), loss_sum / count)
        assert torch.equal(x.grad, dlogits * (torch.ones((), device=dev) / count).to(dtype))
        assert torch.equal(train_ops.cross_entropy(x.detach(), y, 3), loss.detach())


def check_dice_refuses_device(dev):
    import pytest
    logits, labels = R.case_inputs(0)
    fn = losses.DC_and_topk_loss(dict(R.DICE_KWARGS), dict(k=10), weight_ce=1, weight_dice=1)
    with pytest.raises(NotImplementedError):
        fn(torch.from_numpy(logits).to(dev), torch.from_numpy(labels).float().unsqueeze(1).to(dev))


def check_multi_workgroup(dev, dtype):
    """(2, 4, 40, 40, 41), k = 10, every 7th voxel ignored, against ATen in float64 on the device: loss within 1e-5 relative, gradient at
    the dtype's bound at every voxel whose float64 loss is further than 1e-4 from the threshold (at most 32 may be left out)."""
    import torch.nn.functional as F
    shape, C, k = (2, 40, 40, 41), 4, 10
    rs = np.random.RandomState(R.SEED)
    logits = (2.0 * rs.standard_normal((shape[0], C) + shape[1:])).astype(np.float32)
    labels = rs.randint(0, C, size=shape).astype(np.int64)
    labels.reshape(-1)[::7] = C
    y = torch.from_numpy(labels).to(dev)
    x = torch.from_numpy(logits).to(dtype).to(dev).requires_grad_(True)
    loss = losses.TopKLoss(k=k, ignore_index=C)(x, y.unsqueeze(1).float())
    loss.backward()
    x64 = x.detach().double().requires_grad_(True)
    res = F.cross_entropy(x64, y, ignore_index=C, reduction="none")
    kk = R.kk_of(res.numel(), k)
    top = torch.topk(res.view(-1), kk, sorted=False)[0]
    want = top.mean()
    want.backward()
    loss, want = float(loss.detach()), float(want.detach())
    print(f"multi-workgroup {dtype}: loss {loss:.8f} want {want:.8f}")
    assert abs(loss - want) <= 1e-5 * want
    near = (res.detach() - top.min().detach()).abs() <= 1e-4
    left_out = int(near.sum())
    print(f"multi-workgroup {dtype}: {left_out} voxels within 1e-4 of the threshold")
    assert left_out <= 32
    keep = (~near).unsqueeze(1)
    err = ((x.grad.double() - x64.grad).abs() * keep).max()
    print(f"multi-workgroup {dtype}: gradient error {float(err):.3e} of {float(x64.grad.abs().max()):.3e}")
    assert float(err) <= GRAD_TOL[dtype] * float(x64.grad.abs().max())
