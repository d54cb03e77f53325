"""The checks of the region-based loss (csrc/region_loss.hip through segmamba_amd.ops_raw and losses) that the CPU emulation
(tests/test_emu_region_loss.py) and the GPU (tests/test_gpu_region_loss.py) share: `lib` is the loaded library, `dev` where the tensors
live.  References: tests/region_loss_ref.py (float64) and the recorded tests/golden/region_bce.npz.  TEST INFRASTRUCTURE ONLY.

Bounds.  Sums I, P, E: 1e-6 relative - every term is non-negative, the per-voxel fp32 error is a few 2^-24 and the sums are fp64.
G, N: exact.  Gradient of the sums in fp32: 1e-6 x max |g|.  In 16 bits the output is rounded to the dtype: half an ulp with margin,
2^-8 |g| (bf16) or 2^-11 |g| + 2^-25 (fp16, the subnormal spacing), plus the fp32 bound.  Classes: loss 1e-5 relative, gradient
1e-6 x max |g|, the bounds segm_cross_entropy is held to."""
import json
import os

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L, losses, ops_raw
from tests import region_loss_ref as R

NEW_EXPORTS = ("segm_region_loss_workspace_bytes", "segm_region_loss_fwd", "segm_region_loss_bwd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "region_bce.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# spatial shapes with V = 1, 7, 63, 64, 65, 240, 255, 257, 4097 voxels: rows of odd length take the per-voxel route, (2, 4, 8) and
# (3, 5, 16) the packets in every dtype; (17, 241) has two spatial axes, (257,) one
SHAPES = ((1, 1, 1), (1, 1, 7), (1, 9, 7), (2, 4, 8), (1, 5, 13), (3, 5, 16), (3, 5, 17), (257,), (17, 241))
MANY_CHUNKS = (16641, 8)                   # 133128 voxels: 66 workgroups per sample, more partial rows than a wave has lanes
MANY_CHUNKS_WIDE = (8, 16648)              # 133184 voxels in rows of a multiple of 8: the same on the 8-wide packets of 16-bit logits
LABEL_DTYPES = (torch.int64, torch.int16, torch.uint8, torch.float32)
PLANE_DTYPES = (torch.uint8, torch.float32, torch.bool)
IGNORE = 40                                # outside [0, 32): it is compared before the range check
SUM_RTOL, GRAD_TOL, LOSS_RTOL = 1e-6, 1e-6, 1e-5
WORST = {"sum": 0.0}                       # the worst relative error of I, P, E seen by check_sums in this process

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        _golden["cases"] = json.loads(str(_golden["cases"]))
        assert os.path.getsize(GOLDEN) < 100 * 1000
    return _golden


def rounded(logits, dtype, dev):
    """-> (the logits as a `dtype` tensor on dev, the same values as a float64 array)"""
    t = torch.from_numpy(logits).to(dtype)
    return t.to(dev), t.double().numpy()


def make_case(rs, B, Rn, sp, ignore):
    """-> logits fp32, labels int64 in [0, 32), masks, the validity m (B, *sp) or None, the planes float64"""
    logits = (2.0 * rs.standard_normal((B, Rn) + sp)).astype(np.float32)
    labels = rs.randint(0, 32, size=(B,) + sp).astype(np.int64)
    masks = [int(v) for v in rs.randint(0, 1 << 32, size=Rn, dtype=np.uint64)]
    m = None
    if ignore:
        m = np.ones((B,) + sp)
        m.reshape(-1)[::5] = 0
    return logits, labels, masks, m, R.planes_of_masks(labels, masks)


def target_of(kind, tdtype, labels, planes, m, dev):
    """-> the keyword arguments of ops_raw.region_loss_fwd / _bwd after the logits, for a label map or a plane target"""
    if kind == "labels":
        lab = labels.copy()
        if m is not None:
            lab[m == 0] = IGNORE
        return dict(target=torch.from_numpy(lab).to(tdtype).to(dev), ignore_label=None if m is None else IGNORE)
    pl = planes if m is None else np.concatenate([planes, 1.0 - m[:, None]], 1)
    return dict(target=torch.from_numpy(pl).to(tdtype).to(dev), ignore_plane=m is not None)


def assert_sums(got, want, what):
    for name, g, w in zip("IPGEN", got, want):
        g = g.cpu().numpy()
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name)
        if name in "GN":
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            err = np.abs(g - w)
            rel = float((err / np.maximum(np.abs(w), 1e-300)).max()) if err.any() else 0.0
            WORST["sum"] = max(WORST["sum"], rel)
            assert (err <= SUM_RTOL * np.abs(w)).all(), (what, name, rel)


# ---- 1. the sums, fed directly --------------------------------------------------------------------------------------------------------
def check_sums_one(lib, dev, rs, B, Rn, sp, kind, tdtype, ignore, dtype):
    logits, labels, masks, m, planes = make_case(rs, B, Rn, sp, ignore)
    x, x64 = rounded(logits, dtype, dev)
    kw = target_of(kind, tdtype, labels, planes, m, dev)
    got = ops_raw.region_loss_fwd(lib, x, masks=masks if kind == "labels" else None, **kw)
    assert_sums(got, R.sums(x64, planes, m), (sp, Rn, kind, tdtype, ignore, dtype))


def check_sums(lib, dev, shapes=SHAPES):
    """every shape x R in {1, 3, 8} x the seven targets x with / without ignore, the logits' dtype rotating; every dtype pair at 64
    and 65 voxels; 66 workgroups per sample on the per-voxel route, on the 4-wide and on the 8-wide packets"""
    rs = np.random.RandomState(41)
    targets = [("labels", d) for d in LABEL_DTYPES] + [("planes", d) for d in PLANE_DTYPES]
    for si, sp in enumerate(shapes):
        for Rn in (1, 3, 8):
            for ti, (kind, tdtype) in enumerate(targets):
                for ignore in (False, True):
                    check_sums_one(lib, dev, rs, 2, Rn, sp, kind, tdtype, ignore, DTYPES[(si + ti + ignore) % 3])
    for sp in ((2, 4, 8), (1, 5, 13)):
        for kind, tdtype in targets:
            for dtype in DTYPES:
                check_sums_one(lib, dev, rs, 2, 3, sp, kind, tdtype, True, dtype)
    check_sums_one(lib, dev, rs, 2, 1, MANY_CHUNKS, "labels", torch.uint8, True, torch.float32)
    check_sums_one(lib, dev, rs, 1, 2, MANY_CHUNKS[::-1], "planes", torch.uint8, False, torch.bfloat16)
    check_sums_one(lib, dev, rs, 1, 2, MANY_CHUNKS_WIDE, "labels", torch.int64, True, torch.bfloat16)
    check_sums_one(lib, dev, rs, 2, 3, MANY_CHUNKS_WIDE, "planes", torch.float32, True, torch.float16)
    print(f"region sums: worst relative error of I, P, E {WORST['sum']:.3e}")


# ---- 2. layouts, repeatability -----------------------------------------------------------------------------------------------------------
def views(logits, dtype, dev):
    """name -> a view of the logits' values that lies differently in memory"""
    t = torch.from_numpy(logits).to(dtype)
    B, Rn = t.shape[:2]
    sp = tuple(t.shape[2:])
    out = {"dense": t.to(dev)}
    flat = torch.zeros(t.numel() + 1, dtype=dtype)
    flat[1:] = t.reshape(-1)
    out["offset1"] = flat.to(dev)[1:].view(t.shape)
    wide = torch.zeros((B, Rn + 1) + sp, dtype=dtype)
    wide[:, :Rn] = t
    out["channels3of4"] = wide.to(dev)[:, :Rn]
    two = torch.zeros((2 * B, Rn) + sp, dtype=dtype)
    two[::2] = t
    out["batch_strided"] = two.to(dev)[::2]
    pad = torch.zeros((B, Rn) + sp[:-1] + (2 * sp[-1],), dtype=dtype)
    pad[..., :sp[-1]] = t
    out["row_strided"] = pad.to(dev)[..., :sp[-1]]
    tall = torch.zeros((B, Rn) + sp[:-2] + (sp[-2] + 1, sp[-1]), dtype=dtype)
    tall[..., :sp[-2], :] = t
    out["plane_strided"] = tall.to(dev)[..., :sp[-2], :]
    for name, v in out.items():
        assert torch.equal(v.cpu(), t) and v.is_contiguous() == (name in ("dense", "offset1")), name
    return out


def grad_bound(want, dtype):
    mx = np.abs(want).max()
    if dtype == torch.float32:
        return GRAD_TOL * mx
    if dtype == torch.bfloat16:
        return 2.0 ** -8 * np.abs(want) + GRAD_TOL * mx
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -25 + GRAD_TOL * mx


def check_layouts(lib, dev):
    """a storage offset of one element, a 3-of-4 channel slice, a batch-strided view, rows and planes with padding: forward and
    backward within the bounds of the dense tensor (no bit-equality is claimed between differently aligned views)"""
    rs = np.random.RandomState(43)
    for sp in ((4, 6, 8), (3, 5, 7)):
        logits, labels, masks, m, planes = make_case(rs, 2, 3, sp, True)
        coefs = [rs.standard_normal((2, 3)).astype(np.float32) for _ in range(3)]
        tc = [torch.from_numpy(c).to(dev) for c in coefs]
        for dtype in DTYPES:
            x64 = torch.from_numpy(logits).to(dtype).double().numpy()
            want, wgrad = R.sums(x64, planes, m), R.sums_grad(x64, planes, m, *coefs)
            for kind, tdtype in (("labels", torch.int64), ("planes", torch.uint8)):
                kw = target_of(kind, tdtype, labels, planes, m, dev)
                mk = masks if kind == "labels" else None
                for name, v in views(logits, dtype, dev).items():
                    assert_sums(ops_raw.region_loss_fwd(lib, v, masks=mk, **kw), want, (name, sp, dtype, kind))
                    d = ops_raw.region_loss_bwd(lib, v, kw["target"], *tc, masks=mk, **{k: a for k, a in kw.items() if k != "target"})
                    assert d.is_contiguous() and d.dtype == dtype and d.shape == v.shape
                    err = np.abs(d.double().cpu().numpy() - wgrad)
                    assert (err <= grad_bound(wgrad, dtype)).all(), (name, sp, dtype, kind, float(err.max()))


def check_repeat(lib, dev):
    """two calls on the same tensors are bit-equal, forward and backward, on the packet route and on the per-voxel route"""
    rs = np.random.RandomState(44)
    for sp in ((9, 16, 16), (17, 241)):
        logits, labels, masks, m, planes = make_case(rs, 2, 3, sp, True)
        tc = [torch.from_numpy(rs.standard_normal((2, 3)).astype(np.float32)).to(dev) for _ in range(3)]
        for dtype in (torch.float32, torch.bfloat16):
            x, _ = rounded(logits, dtype, dev)
            kw = target_of("labels", torch.int64, labels, planes, m, dev)
            a, b = ops_raw.region_loss_fwd(lib, x, masks=masks, **kw), ops_raw.region_loss_fwd(lib, x, masks=masks, **kw)
            for u, v in zip(a, b):
                assert torch.equal(u, v), "two forward calls differ"
            da = ops_raw.region_loss_bwd(lib, x, kw["target"], *tc, masks=masks, ignore_label=IGNORE)
            db = ops_raw.region_loss_bwd(lib, x, kw["target"], *tc, masks=masks, ignore_label=IGNORE)
            assert torch.equal(da, db), "two backward calls differ"


# ---- 3. the backward ------------------------------------------------------------------------------------------------------------------------
def check_backward(lib, dev):
    """each of gI, gP, gE alone and combined, three dtypes, label and plane targets; exactly 0 at the ignored voxels"""
    rs = np.random.RandomState(45)
    for sp in ((2, 4, 8), (3, 5, 17), (257,)):
        logits, labels, masks, m, planes = make_case(rs, 2, 3, sp, True)
        g = [rs.standard_normal((2, 3)).astype(np.float32) for _ in range(3)]
        zero = np.zeros((2, 3), np.float32)
        combos = {"gI": (g[0], zero, zero), "gP": (zero, g[1], zero), "gE": (zero, zero, g[2]), "all": tuple(g)}
        for dtype in DTYPES:
            x, x64 = rounded(logits, dtype, dev)
            for kind, tdtype in (("labels", torch.int16), ("planes", torch.float32)):
                kw = target_of(kind, tdtype, labels, planes, m, dev)
                rest = {k: a for k, a in kw.items() if k != "target"}
                for name, c in combos.items():
                    tc = [torch.from_numpy(a).to(dev) for a in c]
                    got = ops_raw.region_loss_bwd(lib, x, kw["target"], *tc, masks=masks if kind == "labels" else None, **rest)
                    assert got.dtype == dtype and got.shape == x.shape
                    got = got.double().cpu().numpy()
                    want = R.sums_grad(x64, planes, m, *c)
                    err = np.abs(got - want)
                    assert (err <= grad_bound(want, dtype)).all(), (sp, dtype, kind, name, float(err.max()), float(np.abs(want).max()))
                    off = np.broadcast_to(np.expand_dims(m == 0, 1), got.shape)
                    assert off.any() and (got[off] == 0).all()


# ---- 4. wrong labels ------------------------------------------------------------------------------------------------------------------------
def check_wrong_labels(lib, dev):
    """a label of 32, of -3, a float label of 1.5: NaN in exactly that sample's I, P and E, and in that voxel's gradient; an ignored
    label of 255 or -1 does not"""
    rs = np.random.RandomState(46)
    logits, labels, masks, _, planes = make_case(rs, 2, 3, (3, 5, 8), False)
    x = torch.from_numpy(logits).to(dev)
    ones = [torch.ones(2, 3, device=dev) for _ in range(3)]
    for value, tdtype, sample in ((32, torch.int64, 0), (-3, torch.int16, 1), (1.5, torch.float32, 0), (32, torch.uint8, 1),
                                  (float("nan"), torch.float32, 1)):
        lab = torch.from_numpy(labels.copy()).to(tdtype)
        lab[sample].view(-1)[17] = value
        I, P, G, E, N = (t.cpu().numpy() for t in ops_raw.region_loss_fwd(lib, x, lab.to(dev), masks=masks, ignore_label=255))
        for s in (I, P, E):
            assert np.isnan(s[sample]).all() and np.isfinite(s[1 - sample]).all(), (value, tdtype)
        assert np.isfinite(G).all() and (N == 120).all()
        d = ops_raw.region_loss_bwd(lib, x, lab.to(dev), *ones, masks=masks, ignore_label=255).cpu().numpy().reshape(2, 3, -1)
        assert np.isnan(d[sample, :, 17]).all() and np.isnan(d).sum() == 3, (value, tdtype)
    for value, tdtype in ((255, torch.uint8), (255, torch.int64), (-1, torch.int64), (-1, torch.int16), (-1.0, torch.float32)):
        lab = torch.from_numpy(labels.copy()).to(tdtype)
        lab[0].view(-1)[17] = value
        got = ops_raw.region_loss_fwd(lib, x, lab.to(dev), masks=masks, ignore_label=int(value))
        m = np.ones((2, 3, 5, 8))
        m[0].reshape(-1)[17] = 0
        assert_sums(got, R.sums(logits, planes, m), ("ignored", value, tdtype))
        d = ops_raw.region_loss_bwd(lib, x, lab.to(dev), *ones, masks=masks, ignore_label=int(value)).cpu().numpy().reshape(2, 3, -1)
        assert np.isfinite(d).all() and (d[0, :, 17] == 0).all()


# ---- 5. the classes on the library ----------------------------------------------------------------------------------------------------------
def run(fn, logits, target, dtype, dev):
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32)).to(dtype).to(dev).requires_grad_(True)
    loss = fn(x, target.to(dev))
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == dtype
    return float(loss.detach()), x.grad.double().cpu().numpy()


def dice_kwargs(c):
    return dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"], ddp=False)


def class_of(c, **kw):
    return losses.DC_and_BCE_loss({}, dice_kwargs(c), weight_ce=c["weight_ce"], weight_dice=c["weight_dice"],
                                  use_ignore_label=c["use_ignore_label"],
                                  dice_class=losses.SoftDiceLoss if c["kind"] == "soft" else losses.MemoryEfficientSoftDiceLoss, **kw)


def golden_target(g, c):
    if c["use_ignore_label"]:
        return torch.from_numpy(np.concatenate([g["target"], g["ignore"][:, None]], 1))
    return torch.from_numpy(g["target_soft"] if c["soft_target"] else g["target"])


def check_classes_recorded(dev):
    """the 13 recorded configurations (the soft target among them): loss 1e-5 relative, gradient 1e-6 x max |g|"""
    g = golden()
    assert len(g["cases"]) == 13
    for i, c in enumerate(g["cases"]):
        loss, grad = run(class_of(c), g["logits"], golden_target(g, c), torch.float32, dev)
        assert abs(loss - float(g["loss"][i])) <= LOSS_RTOL * abs(float(g["loss"][i])), (c, loss, float(g["loss"][i]))
        assert np.abs(grad - g["grad"][i]).max() <= GRAD_TOL * np.abs(g["grad"][i]).max(), (c, np.abs(grad - g["grad"][i]).max())


def check_label_mode_equals_plane_mode(dev):
    """DC_and_BCE_loss(regions=BRATS_REGIONS) on the label map against the plane mode on region_targets(labels), with and without
    ignored voxels, (B, *sp) int64 and (B, 1, *sp) float labels: loss 1e-6 relative, gradient 1e-6 x max"""
    g = golden()
    labels = torch.from_numpy(g["labels"])
    assert torch.equal(losses.region_targets(labels).to(torch.uint8), torch.from_numpy(g["target"]))
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    for dtype in DTYPES:
        w_loss, w_grad = run(losses.DC_and_BCE_loss({}, kw), g["logits"], losses.region_targets(labels), dtype, dev)
        for tgt in (labels, labels.unsqueeze(1).float(), labels.to(torch.uint8), labels.to(torch.int16)):
            loss, grad = run(losses.DC_and_BCE_loss({}, kw, regions=losses.BRATS_REGIONS), g["logits"], tgt, dtype, dev)
            assert abs(loss - w_loss) <= 1e-6 * abs(w_loss) and np.abs(grad - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max()
        ign = torch.from_numpy(g["ignore"]).bool()
        planes = torch.cat([losses.region_targets(labels), ign.unsqueeze(1).float()], 1)
        w_loss, w_grad = run(losses.DC_and_BCE_loss({}, kw, use_ignore_label=True), g["logits"], planes, dtype, dev)
        lab = labels.clone()
        lab[ign] = 9
        loss, grad = run(losses.DC_and_BCE_loss({}, kw, regions=losses.BRATS_REGIONS, ignore_label=9), g["logits"], lab, dtype, dev)
        assert abs(loss - w_loss) <= 1e-6 * abs(w_loss) and np.abs(grad - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max()
        assert (grad[np.broadcast_to(ign.unsqueeze(1).numpy(), grad.shape)] == 0).all()


def check_classes_edge_cases(dev):
    """a region that never occurs (its Dice is smooth / (P + smooth)); the all-ignored batch: the BCE term is 0, the loss finite"""
    g = golden()
    labels = g["labels"]
    regions = ((1, 3), (1, 2, 3), (7,))
    for kind, cls in (("soft", losses.SoftDiceLoss), ("mem", losses.MemoryEfficientSoftDiceLoss)):
        for smooth in (1e-5, 0.0):
            kw = dict(batch_dice=False, do_bg=True, smooth=smooth, ddp=False)
            loss, grad = run(losses.DC_and_BCE_loss({}, kw, dice_class=cls, regions=regions), g["logits"], torch.from_numpy(labels),
                             torch.float32, dev)
            w_loss, w_grad = R.value_and_grad(R.dc_and_bce, g["logits"], R.region_planes(labels, regions), None, kind, False, True, smooth)
            assert np.isfinite(loss) and abs(loss - w_loss) <= LOSS_RTOL * abs(w_loss), (kind, smooth, loss, w_loss)
            assert np.abs(grad - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max()
    all_ignored = torch.full(labels.shape, 9, dtype=torch.int64)
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    loss, grad = run(losses.DC_and_BCE_loss({}, kw, weight_dice=0, regions=losses.BRATS_REGIONS, ignore_label=9), g["logits"],
                     all_ignored, torch.float32, dev)
    assert loss == 0.0 and not grad.any()
    loss, grad = run(losses.DC_and_BCE_loss({}, kw, regions=losses.BRATS_REGIONS, ignore_label=9), g["logits"], all_ignored,
                     torch.float32, dev)
    assert np.isfinite(loss) and not grad.any()
    planes = torch.cat([losses.region_targets(torch.from_numpy(labels)), torch.ones((2, 1) + labels.shape[1:])], 1)
    loss, grad = run(losses.DC_and_BCE_loss({}, kw, use_ignore_label=True), g["logits"], planes, torch.float32, dev)
    assert np.isfinite(loss) and not grad.any()


def check_strided_logits_through_the_class(dev):
    """a channel slice of a wider output goes to the kernel as it lies; a tensor without unit stride along x is copied first"""
    g = golden()
    labels = torch.from_numpy(g["labels"])
    fn = losses.DC_and_BCE_loss({}, dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False), regions=losses.BRATS_REGIONS)
    w_loss, w_grad = run(fn, g["logits"], labels, torch.float32, dev)
    wide = torch.zeros(2, 4, 5, 6, 7)
    wide[:, :3] = torch.from_numpy(g["logits"])
    for make in (lambda w: w[:, :3], lambda w: w.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)[:, :3]):
        w = wide.clone().to(dev).requires_grad_(True)
        loss = fn(make(w), labels.to(dev))
        loss.backward()
        assert abs(float(loss.detach()) - w_loss) <= 1e-6 * abs(w_loss)
        assert np.abs(w.grad[:, :3].double().cpu().numpy() - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max() and not w.grad[:, 3].any()


# ---- 6. refusals, exports -------------------------------------------------------------------------------------------------------------------
def check_refusals_host(dev):
    """what the constructor and forward of DC_and_BCE_loss refuse, wherever the tensors lie"""
    g = golden()
    x = torch.from_numpy(g["logits"]).to(dev)
    labels = torch.from_numpy(g["labels"]).to(dev)
    planes = losses.region_targets(labels)
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    BCE = losses.DC_and_BCE_loss
    for bad in (dict(weight=torch.ones(3)), dict(pos_weight=torch.ones(3)), dict(reduction="sum"), dict(reduction="none"),
                dict(size_average=True), dict(reduce=False)):
        with pytest.raises(NotImplementedError):
            BCE(bad, kw)
    with pytest.raises(NotImplementedError):
        BCE({}, kw, dice_class=torch.nn.Identity)
    with pytest.raises(ValueError):
        BCE({}, kw, regions=losses.BRATS_REGIONS, use_ignore_label=True)
    with pytest.raises(ValueError):
        BCE({}, kw, ignore_label=4)
    with pytest.raises(ValueError):
        BCE({}, kw, regions=((1, 32),))
    with pytest.raises(ValueError):
        BCE({}, kw, regions=losses.BRATS_REGIONS)(x, planes)                      # regions together with a plane target
    with pytest.raises(ValueError):
        BCE({}, kw, regions=losses.BRATS_REGIONS[:2])(x, labels)                  # two regions, three channels
    for tgt in (labels[:, :4], planes[:, :2], torch.cat([planes, planes], 1), planes[..., :6], labels.unsqueeze(1)):
        with pytest.raises(ValueError):
            BCE({}, kw)(x, tgt)
    with pytest.raises(ValueError):
        BCE({}, kw, use_ignore_label=True)(x, planes)                              # R planes where R + 1 are announced
    with pytest.raises(ValueError):
        BCE({}, kw)(torch.zeros(2, 9, 5, 6, 7, device=dev), torch.zeros(2, 9, 5, 6, 7, device=dev))


def check_refusals(lib, dev, monkeypatch):
    check_refusals_host(dev)
    g = golden()
    x = torch.from_numpy(g["logits"]).to(dev)
    labels = torch.from_numpy(g["labels"]).to(dev)
    planes = losses.region_targets(labels)
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    BCE = losses.DC_and_BCE_loss
    with pytest.raises(NotImplementedError):
        BCE({}, kw).dc(x, labels.unsqueeze(1).float())                              # the Dice class itself keeps refusing device tensors
    # graph capture: refused before any launch; nothing is captured here
    launched = []
    with monkeypatch.context() as mp:
        mp.setattr(ops_raw, "region_loss_fwd", lambda *a, **k: launched.append(1))
        mp.setattr(torch.cuda, "is_initialized", lambda: True)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            BCE({}, kw, regions=losses.BRATS_REGIONS)(x, labels)
    assert not launched
    # ... and the backward of a forward that ran outside the capture
    xg = x.clone().requires_grad_(True)
    loss = BCE({}, kw, regions=losses.BRATS_REGIONS)(xg, labels)
    with monkeypatch.context() as mp:
        mp.setattr(ops_raw, "region_loss_bwd", lambda *a, **k: launched.append(1))
        mp.setattr(torch.cuda, "is_initialized", lambda: True)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            loss.backward()
    assert not launched and xg.grad is None
    # the C entries
    sums = torch.empty(4 * 2 * 3 + 2, dtype=torch.float64, device=dev)
    d = torch.empty_like(x)
    coef = torch.zeros(2, 3, device=dev)
    dll = lib.dll
    nbytes = dll.segm_region_loss_workspace_bytes(2, 3, 210)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)

    def args(**over):
        a = L.RegionLossArgs()
        a.batch, a.regions, a.dtype, a.target_kind = 2, 3, L.dtype_code(x), L.REGION_LABELS[torch.int64]
        a.depth, a.height, a.width = 5, 6, 7
        a.stride_b, a.stride_r, a.stride_z, a.stride_y, a.stride_x = 630, 210, 42, 7, 1
        for r, mk in enumerate((0b1010, 0b1110, 0b1000)):
            a.masks[r] = mk
        a.logits, a.target, a.sums, a.dlogits = x.data_ptr(), labels.data_ptr(), sums.data_ptr(), d.data_ptr()
        a.g_i = a.g_p = a.g_e = coef.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        for k_, v in over.items():
            setattr(a, k_, v)
        return a
    E_NULL, E_SHAPE, E_DTYPE, E_WS = -1, -2, -4, -6
    assert dll.segm_region_loss_fwd(args()) == 0 and dll.segm_region_loss_bwd(args()) == 0        # the arguments themselves are good
    for fn in (dll.segm_region_loss_fwd, dll.segm_region_loss_bwd):
        assert fn(None) == E_NULL
        for bad in (dict(regions=0), dict(regions=9), dict(stride_x=2), dict(stride_x=0), dict(batch=0), dict(width=0),
                    dict(depth=1 << 15, height=1 << 15, width=4), dict(stride_y=-7), dict(ignore_plane=1)):
            assert fn(args(**bad)) == E_SHAPE, bad
        assert fn(args(dtype=7)) == E_DTYPE and fn(args(target_kind=6)) == E_DTYPE and fn(args(target_kind=-1)) == E_DTYPE
        assert fn(args(logits=None)) == E_NULL and fn(args(target=None)) == E_NULL
    assert dll.segm_region_loss_fwd(args(sums=None)) == E_NULL
    assert dll.segm_region_loss_fwd(args(workspace=None)) == E_WS
    assert dll.segm_region_loss_fwd(args(workspace_bytes=nbytes - 1)) == E_WS
    assert dll.segm_region_loss_fwd(args(workspace=ws.data_ptr() + 4)) == E_WS
    assert dll.segm_region_loss_bwd(args(dlogits=None)) == E_NULL and dll.segm_region_loss_bwd(args(g_p=None)) == E_NULL
    for bad in ((0, 3, 210), (2, 0, 210), (2, 9, 210), (2, 3, 0), (2, 3, 1 << 31)):
        assert dll.segm_region_loss_workspace_bytes(*bad) == 0, bad
    # the wrappers
    masks = [0b1010, 0b1110, 0b1000]
    for call in (lambda: ops_raw.region_loss_fwd(lib, x, labels.int(), masks=masks),
                 lambda: ops_raw.region_loss_fwd(lib, x, labels, masks=masks[:2]),
                 lambda: ops_raw.region_loss_fwd(lib, x, labels),
                 lambda: ops_raw.region_loss_fwd(lib, x, planes, ignore_label=3),
                 lambda: ops_raw.region_loss_fwd(lib, x, planes, ignore_plane=True),
                 lambda: ops_raw.region_loss_fwd(lib, x.double(), planes),
                 lambda: ops_raw.region_loss_fwd(lib, x.transpose(-1, -2), planes.transpose(-1, -2)),
                 lambda: ops_raw.region_loss_fwd(lib, x, planes, workspace=ws[::2]),
                 lambda: ops_raw.region_loss_fwd(lib, x, planes, workspace=ws[:2]),
                 lambda: ops_raw.region_loss_bwd(lib, x, planes, coef, coef, coef[:1]),
                 lambda: ops_raw.region_loss_bwd(lib, x, planes, coef, coef.double(), coef)):
        with pytest.raises(RuntimeError):
            call()


def check_exports(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segmamba_hip.h")).read()
    assert lib.missing == [] and lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert "compound_losses.py:84-100" in hdr and "dice.py:72-113" in hdr


# ---- 7. GPU only: many workgroups per sample against ATen in float64 on the device --------------------------------------------------------
def check_multi_workgroup(dev, dtype):
    """(2, 3, 40, 40, 41), 33 workgroups per sample, every 7th voxel ignored, both target modes against the ATen formulation in float64
    on the device: loss 1e-5 relative, gradient at the dtype's bound"""
    import torch.nn.functional as F
    rs = np.random.RandomState(47)
    logits = (2.0 * rs.standard_normal((2, 3, 40, 40, 41))).astype(np.float32)
    labels = rs.randint(0, 4, size=(2, 40, 40, 41)).astype(np.int64)
    labels.reshape(-1)[::7] = 4
    y = torch.from_numpy(labels).to(dev)
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    x = torch.from_numpy(logits).to(dtype).to(dev).requires_grad_(True)
    loss = losses.DC_and_BCE_loss({}, kw, regions=losses.BRATS_REGIONS, ignore_label=4)(x, y)
    loss.backward()
    x64 = x.detach().double().requires_grad_(True)
    t = losses.region_targets(y).double()
    m = (y != 4).unsqueeze(1).double()
    p = torch.sigmoid(x64)
    inter, pred, gt = (p * t * m).sum((0, 2, 3, 4)), (p * m).sum((0, 2, 3, 4)), (t * m).sum((0, 2, 3, 4))
    dice = -((2 * inter + 1e-5) / torch.clip(gt + pred + 1e-5, 1e-8)).mean()
    want = (F.binary_cross_entropy_with_logits(x64, t, reduction="none") * m).sum() / torch.clip(m.sum(), min=1e-8) + dice
    want.backward()
    got, w = float(loss.detach()), float(want.detach())
    wg = x64.grad.cpu().numpy()
    err = np.abs(x.grad.double().cpu().numpy() - wg)
    print(f"multi-workgroup {dtype}: loss {got:.8f} want {w:.8f}; gradient error {float(err.max()):.3e} of {float(np.abs(wg).max()):.3e}")
    assert abs(got - w) <= LOSS_RTOL * abs(w)
    assert (err <= grad_bound(wg, dtype)).all()
    assert (x.grad[(y == 4).unsqueeze(1).expand_as(x.grad)] == 0).all()
    planes = torch.cat([t.float(), (y == 4).unsqueeze(1).float()], 1)
    x2 = x.detach().clone().requires_grad_(True)
    loss2 = losses.DC_and_BCE_loss({}, kw, use_ignore_label=True)(x2, planes)
    loss2.backward()
    assert abs(float(loss2.detach()) - w) <= LOSS_RTOL * abs(w)
    assert (np.abs(x2.grad.double().cpu().numpy() - wg) <= grad_bound(wg, dtype)).all()
