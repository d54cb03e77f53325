"""The checks of softmax Dice + cross entropy on the device (csrc/dice_ce.hip through segmamba_amd.ops_raw and losses) that the CPU
emulation (tests/test_emu_dice_ce.py) and the GPU (tests/test_gpu_dice_ce.py) share: `lib` is the loaded library, `dev` where the
tensors live.  References: tests/loss_ref.py (float64) and the recorded tests/golden/dice_ce.npz and topk_ce.npz.  TEST INFRASTRUCTURE
ONLY.

Bounds.  Sums I, P: 1e-6 relative, the region loss's bound - every term is non-negative, the per-voxel fp32 error is a few 2^-24 and
the sums are fp64.  CE: 1e-5 relative, segm_cross_entropy's bound.  G, N: exact.  Gradient of the sums in fp32: 1e-6 x max |g|.  In 16
bits the output is rounded to the dtype: half an ulp with margin, 2^-8 |g| (bf16) or 2^-11 |g| + 2^-25 (fp16, the subnormal spacing),
plus the fp32 bound.  Classes: loss 1e-5 relative, gradient 1e-6 x max |g|."""
import json
import os

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L, losses, ops_raw
from tests import loss_ref as R
from tests import topk_ref

NEW_EXPORTS = ("segm_softmax_dice_workspace_bytes", "segm_softmax_dice_fwd", "segm_softmax_dice_bwd")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dice_ce.npz")
GOLDEN_TOPK = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "topk_ce.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# spatial shapes with V = 1, 7, 63, 64, 65, 240, 255, 257, 4097 voxels: rows of odd length take the per-voxel route, (2, 4, 8) and
# (3, 5, 16) the packets in every dtype; (17, 241) has two spatial axes, (257,) one
SHAPES = ((1, 1, 1), (1, 1, 7), (1, 9, 7), (2, 4, 8), (1, 5, 13), (3, 5, 16), (3, 5, 17), (257,), (17, 241))
MANY_CHUNKS = (16641, 8)                   # 133128 voxels: 66 workgroups per sample, more partial rows than a wave has lanes
MANY_CHUNKS_WIDE = (8, 16648)              # 133184 voxels in rows of a multiple of 8: the same on the 8-wide packets of 16-bit logits
# 8 | 9: the last class count with a packet instantiation and the first that takes the per-voxel route on aligned rows too
CLASSES = (1, 2, 4, 8, 9, 16)
LABEL_DTYPES = (torch.int64, torch.int16, torch.uint8, torch.float32)
IGNORE = 40                                # outside [0, 16): it is compared before the range check
SUM_RTOL, CE_RTOL, GRAD_TOL, LOSS_RTOL = 1e-6, 1e-5, 1e-6, 1e-5
WORST = {"IP": 0.0, "CE": 0.0}             # the worst relative errors seen by assert_sums in this process

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        _golden["cases"] = json.loads(str(_golden["cases"]))
    return _golden


def rounded(logits, dtype, dev):
    """-> (the logits as a `dtype` tensor on dev, the same values as a float64 tensor)"""
    t = torch.from_numpy(logits).to(dtype)
    return t.to(dev), t.double()


def make_case(rs, B, C, sp, ignore, mask):
    """-> logits fp32, labels int64 in [0, C) with IGNORE at every 5th voxel if `ignore`, the mask (B, *sp) uint8 or None.  With
    C >= 2 class C - 1 never occurs in the last sample."""
    logits = (2.0 * rs.standard_normal((B, C) + sp)).astype(np.float32)
    labels = rs.randint(0, C, size=(B,) + sp).astype(np.int64)
    if C >= 2:
        labels[-1][labels[-1] == C - 1] = 0
    if ignore:
        labels.reshape(-1)[::5] = IGNORE
    m = (rs.rand(*((B,) + sp)) < 0.7).astype(np.uint8) if mask else None
    return logits, labels, m


def assert_sums(got, want, what, C=None, never=None):
    for name, g, w in zip(("I", "P", "G", "CE", "N"), got, want):
        g, w = g.cpu().numpy(), w.numpy()
        assert g.dtype == np.float64 and g.shape == w.shape, (what, name)
        if name in ("G", "N"):
            assert np.array_equal(g, w), (what, name, g, w)
        else:
            err = np.abs(g - w)
            rel = float((err / np.maximum(np.abs(w), 1e-300)).max()) if err.any() else 0.0
            key = "CE" if name == "CE" else "IP"
            WORST[key] = max(WORST[key], rel)
            assert (err <= (CE_RTOL if name == "CE" else SUM_RTOL) * np.abs(w)).all(), (what, name, rel)
    if never is not None:
        b, c = never
        assert float(got[0][b, c]) == 0.0 and float(got[2][b, c]) == 0.0, (what, "a class that never occurs")


def sums_grad(x64, labels, m, ignore, gi, gp, gce):
    """autograd in float64 on the restatement: d (sum gi I + sum gp P + sum gce CE) / d x"""
    x = x64.clone().requires_grad_(True)
    I, P, _, CE, _ = R.sums(x, labels, m, ignore)
    ((I * torch.from_numpy(gi).double()).sum() + (P * torch.from_numpy(gp).double()).sum()
     + (CE * torch.from_numpy(gce).double()).sum()).backward()
    return x.grad.numpy()


def grad_bound(want, dtype):
    mx = np.abs(want).max()
    if dtype == torch.float32:
        return GRAD_TOL * mx
    if dtype == torch.bfloat16:
        return 2.0 ** -8 * np.abs(want) + GRAD_TOL * mx
    return 2.0 ** -11 * np.abs(want) + 2.0 ** -25 + GRAD_TOL * mx


def dev_mask(m, dev):
    return None if m is None else torch.from_numpy(m).to(dev)


# ---- 1. the sums, fed directly --------------------------------------------------------------------------------------------------------
def check_sums_one(lib, dev, rs, B, C, sp, ldtype, ignore, mask, dtype):
    logits, labels, m = make_case(rs, B, C, sp, ignore, mask)
    x, x64 = rounded(logits, dtype, dev)
    ign = IGNORE if ignore else None
    got = ops_raw.softmax_dice_fwd(lib, x, torch.from_numpy(labels).to(ldtype).to(dev), dev_mask(m, dev), ign)
    assert_sums(got, R.sums(x64, labels, m, ign), (sp, C, ldtype, ignore, mask, dtype), C, (B - 1, C - 1) if C >= 2 else None)


def check_sums(lib, dev, shapes=SHAPES):
    """every shape x C in {1, 2, 4, 8, 9, 16} x four label dtypes x with / without ignore, the mask and the logits' dtype rotating;
    every (label dtype, logits dtype, mask) at 64 and 65 voxels; 66 workgroups per sample on the per-voxel route, on the 4-wide and
    on the 8-wide packets"""
    rs = np.random.RandomState(61)
    for si, sp in enumerate(shapes):
        for ci, C in enumerate(CLASSES):
            for ti, ldtype in enumerate(LABEL_DTYPES):
                for ignore in (False, True):
                    check_sums_one(lib, dev, rs, 2, C, sp, ldtype, ignore, (si + ci + ti + ignore) % 2 == 0, DTYPES[(si + ci + ti + ignore) % 3])
    for sp in ((2, 4, 8), (1, 5, 13)):
        for ldtype in LABEL_DTYPES:
            for dtype in DTYPES:
                for mask in (False, True):
                    check_sums_one(lib, dev, rs, 2, 4, sp, ldtype, True, mask, dtype)
    check_sums_one(lib, dev, rs, 2, 2, MANY_CHUNKS[::-1], torch.uint8, True, False, torch.float32)        # rows of odd length: per voxel
    check_sums_one(lib, dev, rs, 1, 9, MANY_CHUNKS, torch.int16, False, True, torch.bfloat16)            # 9 classes: per voxel
    check_sums_one(lib, dev, rs, 2, 4, MANY_CHUNKS, torch.int64, True, True, torch.float32)              # the 4-wide packets
    check_sums_one(lib, dev, rs, 1, 4, MANY_CHUNKS_WIDE, torch.int64, True, False, torch.bfloat16)       # the 8-wide packets
    check_sums_one(lib, dev, rs, 2, 8, MANY_CHUNKS_WIDE, torch.float32, False, True, torch.float16)
    print(f"softmax dice sums: worst relative error of I, P {WORST['IP']:.3e}, of CE {WORST['CE']:.3e}")


# ---- 2. layouts, repeatability -----------------------------------------------------------------------------------------------------------
def views(logits, dtype, dev):
    """name -> a view of the logits' values that lies differently in memory"""
    t = torch.from_numpy(logits).to(dtype)
    B, C = t.shape[:2]
    sp = tuple(t.shape[2:])
    out = {"dense": t.to(dev)}
    flat = torch.zeros(t.numel() + 1, dtype=dtype)
    flat[1:] = t.reshape(-1)
    out["offset1"] = flat.to(dev)[1:].view(t.shape)
    wide = torch.zeros((B, C + 1) + sp, dtype=dtype)
    wide[:, :C] = t
    out["channels4of5"] = wide.to(dev)[:, :C]
    two = torch.zeros((2 * B, C) + sp, dtype=dtype)
    two[::2] = t
    out["batch_strided"] = two.to(dev)[::2]
    pad = torch.zeros((B, C) + sp[:-1] + (2 * sp[-1],), dtype=dtype)
    pad[..., :sp[-1]] = t
    out["row_strided"] = pad.to(dev)[..., :sp[-1]]
    tall = torch.zeros((B, C) + sp[:-2] + (sp[-2] + 1, sp[-1]), dtype=dtype)
    tall[..., :sp[-2], :] = t
    out["plane_strided"] = tall.to(dev)[..., :sp[-2], :]
    for name, v in out.items():
        assert torch.equal(v.cpu(), t) and v.is_contiguous() == (name in ("dense", "offset1")), name
    return out


def check_layouts(lib, dev):
    """a storage offset of one element, a 4-of-5 channel slice, a batch-strided view, rows and planes with padding: forward and
    backward held to the restatement (no bit-equality is claimed between differently aligned views)"""
    rs = np.random.RandomState(63)
    for sp in ((4, 6, 8), (3, 5, 7)):
        logits, labels, m = make_case(rs, 2, 4, sp, True, True)
        gi, gp = (rs.standard_normal((2, 4)).astype(np.float32) for _ in range(2))
        gce = rs.standard_normal(2).astype(np.float32)
        tc = [torch.from_numpy(c).to(dev) for c in (gi, gp, gce)]
        y, mk = torch.from_numpy(labels).to(dev), dev_mask(m, dev)
        for dtype in DTYPES:
            x64 = torch.from_numpy(logits).to(dtype).double()
            want, wgrad = R.sums(x64, labels, m, IGNORE), sums_grad(x64, labels, m, IGNORE, gi, gp, gce)
            for name, v in views(logits, dtype, dev).items():
                assert_sums(ops_raw.softmax_dice_fwd(lib, v, y, mk, IGNORE), want, (name, sp, dtype))
                d = ops_raw.softmax_dice_bwd(lib, v, y, *tc, mask=mk, ignore_label=IGNORE)
                assert d.is_contiguous() and d.dtype == dtype and d.shape == v.shape
                err = np.abs(d.double().cpu().numpy() - wgrad)
                assert (err <= grad_bound(wgrad, dtype)).all(), (name, sp, dtype, float(err.max()))


def check_repeat(lib, dev):
    """two calls on the same tensors are bit-equal, forward and backward, on the packet route and on the per-voxel route"""
    rs = np.random.RandomState(64)
    for sp in ((9, 16, 16), (17, 241)):
        logits, labels, m = make_case(rs, 2, 4, sp, True, True)
        tc = [torch.from_numpy(rs.standard_normal(s).astype(np.float32)).to(dev) for s in ((2, 4), (2, 4), (2,))]
        y, mk = torch.from_numpy(labels).to(dev), dev_mask(m, dev)
        for dtype in (torch.float32, torch.bfloat16):
            x, _ = rounded(logits, dtype, dev)
            a, b = ops_raw.softmax_dice_fwd(lib, x, y, mk, IGNORE), ops_raw.softmax_dice_fwd(lib, x, y, mk, IGNORE)
            for u, v in zip(a, b):
                assert torch.equal(u, v), "two forward calls differ"
            da = ops_raw.softmax_dice_bwd(lib, x, y, *tc, mask=mk, ignore_label=IGNORE)
            db = ops_raw.softmax_dice_bwd(lib, x, y, *tc, mask=mk, ignore_label=IGNORE)
            assert torch.equal(da, db), "two backward calls differ"


# ---- 3. the backward ------------------------------------------------------------------------------------------------------------------------
def check_backward(lib, dev):
    """each of gI, gP, gCE alone and combined, three dtypes, the packet instantiations and the per-voxel route (odd rows, 9 classes);
    exactly 0 at the ignored and at the masked voxels"""
    rs = np.random.RandomState(65)
    for sp, C in (((2, 4, 8), 4), ((2, 4, 8), 8), ((2, 4, 8), 9), ((3, 5, 17), 4), ((257,), 16)):
        logits, labels, m = make_case(rs, 2, C, sp, True, True)
        g = [rs.standard_normal((2, C)).astype(np.float32), rs.standard_normal((2, C)).astype(np.float32),
             rs.standard_normal(2).astype(np.float32)]
        z = [np.zeros_like(a) for a in g]
        combos = {"gI": (g[0], z[1], z[2]), "gP": (z[0], g[1], z[2]), "gCE": (z[0], z[1], g[2]), "all": tuple(g)}
        y, mk = torch.from_numpy(labels).to(torch.int16).to(dev), dev_mask(m, dev)
        off = np.broadcast_to(np.expand_dims((labels == IGNORE) | (m == 0), 1), logits.shape)
        assert off.any() and not off.all()
        for dtype in DTYPES:
            x, x64 = rounded(logits, dtype, dev)
            for name, c in combos.items():
                tc = [torch.from_numpy(a).to(dev) for a in c]
                got = ops_raw.softmax_dice_bwd(lib, x, y, *tc, mask=mk, ignore_label=IGNORE)
                assert got.dtype == dtype and got.shape == x.shape
                got = got.double().cpu().numpy()
                want = sums_grad(x64, labels, m, IGNORE, *c)
                err = np.abs(got - want)
                assert (err <= grad_bound(want, dtype)).all(), (sp, C, dtype, name, float(err.max()), float(np.abs(want).max()))
                assert (got[off] == 0).all()


# ---- 4. wrong labels ------------------------------------------------------------------------------------------------------------------------
def check_wrong_labels(lib, dev):
    """a label of C, of -3, a float label of 1.5 or NaN: NaN in exactly that sample's I, P and CE, and in that voxel's gradient; an
    ignored label of 255 or -1 does not; a wrong label under a zero of the mask does not either"""
    rs = np.random.RandomState(66)
    C = 4
    logits, labels, _ = make_case(rs, 2, C, (3, 5, 8), False, False)
    x = torch.from_numpy(logits).to(dev)
    ones = [torch.ones(2, C, device=dev), torch.ones(2, C, device=dev), torch.ones(2, device=dev)]
    for value, tdtype, sample in ((C, torch.int64, 0), (-3, torch.int16, 1), (1.5, torch.float32, 0), (C, torch.uint8, 1),
                                  (float("nan"), torch.float32, 1)):
        lab = torch.from_numpy(labels.copy()).to(tdtype)
        lab[sample].view(-1)[17] = value
        I, P, G, CE, N = (t.cpu().numpy() for t in ops_raw.softmax_dice_fwd(lib, x, lab.to(dev), None, 255))
        assert np.isnan(I[sample]).all() and np.isnan(P[sample]).all() and np.isnan(CE[sample]), (value, tdtype)
        assert np.isfinite(I[1 - sample]).all() and np.isfinite(P[1 - sample]).all() and np.isfinite(CE[1 - sample]), (value, tdtype)
        assert np.isfinite(G).all() and (N == 120).all()
        d = ops_raw.softmax_dice_bwd(lib, x, lab.to(dev), *ones, ignore_label=255).cpu().numpy().reshape(2, C, -1)
        assert np.isnan(d[sample, :, 17]).all() and np.isnan(d).sum() == C, (value, tdtype)
        # the same wrong label where the mask is 0 does not count
        mk = torch.ones(lab.shape, dtype=torch.uint8)
        mk[sample].view(-1)[17] = 0
        got = ops_raw.softmax_dice_fwd(lib, x, lab.to(dev), mk.to(dev), 255)
        assert_sums(got, R.sums(torch.from_numpy(logits).double(), labels, mk.numpy(), 255), ("masked wrong label", value, tdtype))
    for value, tdtype in ((255, torch.uint8), (255, torch.int64), (-1, torch.int64), (-1, torch.int16), (-1.0, torch.float32)):
        lab = torch.from_numpy(labels.copy()).to(tdtype)
        lab[0].view(-1)[17] = value
        got = ops_raw.softmax_dice_fwd(lib, x, lab.to(dev), None, int(value))
        m = np.ones((2, 3, 5, 8), dtype=np.uint8)
        m[0].reshape(-1)[17] = 0
        assert_sums(got, R.sums(torch.from_numpy(logits).double(), labels, m), ("ignored", value, tdtype))
        d = ops_raw.softmax_dice_bwd(lib, x, lab.to(dev), *ones, ignore_label=int(value)).cpu().numpy().reshape(2, C, -1)
        assert np.isfinite(d).all() and (d[0, :, 17] == 0).all()


# ---- 5. the classes on the library, device_sums=True ------------------------------------------------------------------------------------
def run(fn, logits, target, dtype, dev, **kw):
    x = torch.from_numpy(np.asarray(logits, dtype=np.float32)).to(dtype).to(dev).requires_grad_(True)
    loss = fn(x, target.to(dev), **{k: v.to(dev) for k, v in kw.items()})
    loss.backward()
    assert loss.dtype == torch.float32 and x.grad.dtype == dtype
    return float(loss.detach()), x.grad.double().cpu().numpy()


def class_of(c, **kw):
    dk = dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"], ddp=False)
    if c.get("clip_tp") is not None:
        dk["clip_tp"] = c["clip_tp"]
    return losses.DC_and_CE_loss(dk, {}, weight_ce=c.get("weight_ce", 1), weight_dice=c.get("weight_dice", 1),
                                 ignore_label=c.get("ignore_label"),
                                 dice_class=losses.SoftDiceLoss if c["kind"] == "soft" else losses.MemoryEfficientSoftDiceLoss, **kw)


def close(loss, grad, w_loss, w_grad, what):
    assert abs(loss - w_loss) <= LOSS_RTOL * abs(w_loss), (what, loss, w_loss)
    assert np.abs(grad - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max(), (what, float(np.abs(grad - w_grad).max()))


def check_classes_recorded(dev):
    """the 14 recorded configurations of DC_and_CE_loss: loss 1e-5 relative, gradient 1e-6 x max |g|"""
    g = golden()
    assert len(g["cases"]) == 14
    for i, c in enumerate(g["cases"]):
        tgt = torch.from_numpy(g["target_ignore"] if c["ignore_label"] is not None else g["target"])
        loss, grad = run(class_of(c, device_sums=True), g["logits"], tgt, torch.float32, dev)
        close(loss, grad, float(g["loss"][i]), g["grad"][i].astype(np.float64), c)


def check_topk_recorded(dev):
    """DC_and_topk_loss(weight_dice=1, device_sums=True), wholly on the device, against topk_ce.npz's recordings with a Dice term:
    loss 1e-5 relative, gradient 1e-6 x max |g| (the fp32 bounds of tests/topk_checks.py)"""
    with np.load(GOLDEN_TOPK) as z:
        for i in topk_ref.DICE_CASES:
            shape, C, k, ignore = topk_ref.CASES[i]
            logits, labels = topk_ref.case_inputs(i)
            fn = losses.DC_and_topk_loss(dict(topk_ref.DICE_KWARGS), dict(k=k), weight_ce=1, weight_dice=1, ignore_label=ignore,
                                         device_sums=True)
            loss, grad = run(fn, logits, torch.from_numpy(labels).float().unsqueeze(1), torch.float32, dev)
            close(loss, grad, float(z[f"dc_loss_{i}"]), z[f"dc_grad_{i}"].astype(np.float64), ("topk", i))


def check_dice_classes_and_masks(dev):
    """both Dice classes on their own with device_sums=True: a loss_mask in bool, uint8 and float, labels (B, 1, ...) float and
    (B, ...) int64, a class that never occurs, against tests/loss_ref.py"""
    rng = np.random.default_rng(11)
    x = (2 * rng.standard_normal((2, 5, 4, 6, 9))).astype(np.float32)
    y = rng.integers(0, 5, (2, 4, 6, 9))
    y[1][y[1] == 3] = 0                                     # class 3 never occurs in sample 1
    m = rng.random(y.shape) < 0.6
    for kind, cls in (("soft", losses.SoftDiceLoss), ("mem", losses.MemoryEfficientSoftDiceLoss)):
        for batch_dice, do_bg, smooth in ((False, True, 1e-5), (True, False, 1.0), (False, False, 0.0)):
            mod = cls(apply_nonlin=losses.softmax_helper_dim1, batch_dice=batch_dice, do_bg=do_bg, smooth=smooth, ddp=False, device_sums=True)
            v, gr = R.value_and_grad(R.dice, x, y, kind, batch_dice, do_bg, smooth)
            for tgt in (torch.as_tensor(y.astype(np.float32))[:, None], torch.as_tensor(y)):
                close(*run(mod, x, tgt, torch.float32, dev), v, gr, (kind, batch_dice, do_bg, smooth))
            vm, gm = R.value_and_grad(R.dice, x, y, kind, batch_dice, do_bg, smooth, mask=m)
            for dt in (torch.bool, torch.uint8, torch.float32):
                close(*run(mod, x, torch.as_tensor(y), torch.float32, dev, loss_mask=torch.as_tensor(m)[:, None].to(dt)), vm, gm, (kind, dt))


def check_classes_edge_cases(dev):
    """the all-ignored batch: the CE term is 0 and the loss finite; DeepSupervisionWrapper over two scales; bf16 logits"""
    g = golden()
    tgt = torch.full((2, 1, 5, 6, 7), 4.0)
    loss, grad = run(losses.DC_and_CE_loss({"ddp": False}, {}, weight_dice=0, ignore_label=4, device_sums=True), g["logits"], tgt,
                     torch.float32, dev)
    assert loss == 0.0 and not grad.any()
    both = losses.DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, ignore_label=4,
                                 dice_class=losses.MemoryEfficientSoftDiceLoss, device_sums=True)
    loss, grad = run(both, g["logits"], tgt, torch.float32, dev)
    assert np.isfinite(loss) and not grad.any()
    # two scales
    fn = losses.DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, ignore_label=4, device_sums=True)
    mod = losses.DeepSupervisionWrapper(fn, weight_factors=(1.0, 0.5))
    xs = [torch.from_numpy(g["logits"]).to(dev).requires_grad_(True), torch.from_numpy(g["logits"][..., ::2].copy()).to(dev).requires_grad_(True)]
    ys = [torch.from_numpy(g["target_ignore"]).to(dev), torch.from_numpy(g["target_ignore"][..., ::2].copy()).to(dev)]
    total = mod(xs, ys)
    total.backward()
    want, wgrads = 0.0, []
    for w, a, b in zip((1.0, 0.5), (g["logits"], g["logits"][..., ::2]), (g["target_ignore"], g["target_ignore"][..., ::2])):
        v, gr = R.value_and_grad(R.dc_and_ce, a, b[:, 0].astype(np.int64), "soft", True, False, 1e-5, ignore=4)
        want += w * v
        wgrads.append(w * gr)
    assert total.dtype == torch.float32 and abs(float(total.detach()) - want) <= LOSS_RTOL * abs(want)
    for xg, wg in zip(xs, wgrads):
        assert np.abs(xg.grad.double().cpu().numpy() - wg).max() <= GRAD_TOL * np.abs(wg).max()
    # 16-bit logits through the class: the gradient comes back in the logits' dtype
    for dtype in (torch.bfloat16, torch.float16):
        x64 = torch.from_numpy(g["logits"]).to(dtype).double().numpy()
        v, gr = R.value_and_grad(R.dc_and_ce, x64, g["target_ignore"][:, 0].astype(np.int64), "soft", True, False, 1e-5, ignore=4)
        loss, grad = run(fn, g["logits"], torch.from_numpy(g["target_ignore"]), dtype, dev)
        assert abs(loss - v) <= LOSS_RTOL * abs(v) and (np.abs(grad - gr) <= grad_bound(gr, dtype)).all()


def check_strided_logits_through_the_class(dev):
    """a channel slice of a wider output goes to the kernel as it lies; a tensor without unit stride along x is copied first"""
    g = golden()
    tgt = torch.from_numpy(g["target"])
    fn = losses.DC_and_CE_loss(dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False), {}, device_sums=True)
    w_loss, w_grad = run(fn, g["logits"], tgt, torch.float32, dev)
    wide = torch.zeros(2, 5, 5, 6, 7)
    wide[:, :4] = torch.from_numpy(g["logits"])
    for make in (lambda w: w[:, :4], lambda w: w.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)[:, :4]):
        w = wide.clone().to(dev).requires_grad_(True)
        loss = fn(make(w), tgt.to(dev))
        loss.backward()
        assert abs(float(loss.detach()) - w_loss) <= 1e-6 * abs(w_loss)
        assert np.abs(w.grad[:, :4].double().cpu().numpy() - w_grad).max() <= GRAD_TOL * np.abs(w_grad).max() and not w.grad[:, 4].any()


# ---- 6. refusals, exports -------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev, monkeypatch):
    g = golden()
    x = torch.from_numpy(g["logits"]).to(dev)
    tgt = torch.from_numpy(g["target"]).to(dev)
    labels = tgt[:, 0].long().contiguous()
    kw = dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False)
    sm = losses.softmax_helper_dim1
    # the default keeps every refusal on the library's tensors; dice_ce_sums itself keeps refusing
    for mod in (losses.SoftDiceLoss(sm, ddp=False), losses.MemoryEfficientSoftDiceLoss(sm, ddp=False), losses.DC_and_CE_loss(kw, {}),
                losses.DC_and_CE_loss(kw, {}, device_sums=False), losses.DC_and_topk_loss(kw, {}),
                losses.SoftDiceLoss(torch.sigmoid, ddp=False, device_sums=True), losses.MemoryEfficientSoftDiceLoss(None, ddp=False, device_sums=True)):
        with pytest.raises(NotImplementedError):
            mod(x, tgt)
    with pytest.raises(NotImplementedError):
        losses.dice_ce_sums(x, tgt)
    with pytest.raises(NotImplementedError, match="one-hot"):
        losses.DC_and_CE_loss(kw, {}, device_sums=True)(x, torch.zeros_like(x))
    with pytest.raises(ValueError):
        losses.softmax_dice_sums(x, labels[:, :4])
    with pytest.raises(NotImplementedError):
        losses.softmax_dice_sums(torch.zeros(2, 17, 3, 4, 5, device=dev), torch.zeros(2, 3, 4, 5, device=dev))
    # graph capture: refused before any launch; nothing is captured here
    launched = []
    with monkeypatch.context() as mp:
        mp.setattr(ops_raw, "softmax_dice_fwd", lambda *a, **k: launched.append(1))
        mp.setattr(torch.cuda, "is_initialized", lambda: True)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            losses.DC_and_CE_loss(kw, {}, device_sums=True)(x, tgt)
        with pytest.raises(RuntimeError, match="capture"):
            losses.softmax_dice_sums(x, tgt)
        mp.setattr(ops_raw, "cross_entropy_map", lambda *a, **k: launched.append(1))
        with pytest.raises(RuntimeError, match="capture"):
            losses.DC_and_topk_loss(kw, {}, device_sums=True)(x, tgt)               # before its top-k kernels
    assert not launched
    # ... and the backward of a forward that ran outside the capture
    xg = x.clone().requires_grad_(True)
    loss = losses.DC_and_CE_loss(kw, {}, device_sums=True)(xg, tgt)
    with monkeypatch.context() as mp:
        mp.setattr(ops_raw, "softmax_dice_bwd", lambda *a, **k: launched.append(1))
        mp.setattr(torch.cuda, "is_initialized", lambda: True)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="capture"):
            loss.backward()
    assert not launched and xg.grad is None
    # the C entries
    sums = torch.empty(3 * 2 * 4 + 2 * 2, dtype=torch.float64, device=dev)
    d = torch.empty_like(x)
    coef = torch.zeros(2, 4, device=dev)
    dll = lib.dll
    nbytes = dll.segm_softmax_dice_workspace_bytes(2, 4, 210)
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device=dev)

    def args(**over):
        a = L.SoftmaxDiceArgs()
        a.batch, a.classes, a.dtype, a.label_kind = 2, 4, L.dtype_code(x), L.REGION_LABELS[torch.int64]
        a.depth, a.height, a.width = 5, 6, 7
        a.stride_b, a.stride_c, a.stride_z, a.stride_y, a.stride_x = 840, 210, 42, 7, 1
        a.logits, a.labels, a.sums, a.dlogits = x.data_ptr(), labels.data_ptr(), sums.data_ptr(), d.data_ptr()
        a.g_i = a.g_p = a.g_ce = coef.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
        for k_, v in over.items():
            setattr(a, k_, v)
        return a
    E_NULL, E_SHAPE, E_DTYPE, E_WS = -1, -2, -4, -6
    assert dll.segm_softmax_dice_fwd(args()) == 0 and dll.segm_softmax_dice_bwd(args()) == 0      # the arguments themselves are good
    for fn in (dll.segm_softmax_dice_fwd, dll.segm_softmax_dice_bwd):
        assert fn(None) == E_NULL
        for bad in (dict(classes=0), dict(classes=17), dict(stride_x=2), dict(stride_x=0), dict(batch=0), dict(width=0),
                    dict(depth=1 << 15, height=1 << 15, width=2), dict(stride_y=-7)):
            assert fn(args(**bad)) == E_SHAPE, bad
        assert fn(args(dtype=7)) == E_DTYPE and fn(args(label_kind=4)) == E_DTYPE and fn(args(label_kind=-1)) == E_DTYPE
        assert fn(args(logits=None)) == E_NULL and fn(args(labels=None)) == E_NULL
    assert dll.segm_softmax_dice_fwd(args(sums=None)) == E_NULL
    assert dll.segm_softmax_dice_fwd(args(workspace=None)) == E_WS
    assert dll.segm_softmax_dice_fwd(args(workspace_bytes=nbytes - 1)) == E_WS
    assert dll.segm_softmax_dice_fwd(args(workspace=ws.data_ptr() + 4)) == E_WS
    assert dll.segm_softmax_dice_bwd(args(dlogits=None)) == E_NULL and dll.segm_softmax_dice_bwd(args(g_p=None)) == E_NULL
    assert dll.segm_softmax_dice_bwd(args(g_ce=None)) == E_NULL
    for bad in ((0, 4, 210), (2, 0, 210), (2, 17, 210), (2, 4, 0), (2, 4, 1 << 31)):
        assert dll.segm_softmax_dice_workspace_bytes(*bad) == 0, bad
    # the wrappers
    mk = torch.ones(labels.shape, dtype=torch.uint8, device=dev)
    for call in (lambda: ops_raw.softmax_dice_fwd(lib, x, labels.int()),
                 lambda: ops_raw.softmax_dice_fwd(lib, x, labels[:, :4]),
                 lambda: ops_raw.softmax_dice_fwd(lib, x, labels, mk.bool()),
                 lambda: ops_raw.softmax_dice_fwd(lib, x, labels, mk[:, :4]),
                 lambda: ops_raw.softmax_dice_fwd(lib, x.double(), labels),
                 lambda: ops_raw.softmax_dice_fwd(lib, x.transpose(-1, -2), labels.transpose(-1, -2)),
                 lambda: ops_raw.softmax_dice_fwd(lib, x, labels, workspace=ws[::2]),
                 lambda: ops_raw.softmax_dice_fwd(lib, x, labels, workspace=ws[:2]),
                 lambda: ops_raw.softmax_dice_bwd(lib, x, labels, coef, coef, coef[:1, 0]),
                 lambda: ops_raw.softmax_dice_bwd(lib, x, labels, coef, coef.double(), coef[0, :2].contiguous())):
        with pytest.raises(RuntimeError):
            call()


def check_exports(lib):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "segmamba_hip.h")).read()
    assert lib.missing == [] and lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert "dice.py:9-116" in hdr and "compound_losses.py:8-57" in hdr


# ---- 7. GPU only: many workgroups per sample against ATen in float64 on the device --------------------------------------------------------
def check_multi_workgroup(dev, dtype):
    """(2, 4, 40, 40, 41), 33 stretches per sample, every 7th voxel ignored, against the ATen formulation in float64 on the device:
    the sums at the bounds of check_sums, the gradient of sum gI I + sum gP P + sum gCE CE at the dtype's bound, and
    DC_and_CE_loss(device_sums=True) at 1e-5 relative"""
    rs = np.random.RandomState(67)
    logits = (2.0 * rs.standard_normal((2, 4, 40, 40, 41))).astype(np.float32)
    labels = rs.randint(0, 4, size=(2, 40, 40, 41)).astype(np.int64)
    labels.reshape(-1)[::7] = 4
    y = torch.from_numpy(labels).to(dev)
    gi, gp = (torch.from_numpy(rs.standard_normal((2, 4))).to(dev) for _ in range(2))
    gce = torch.from_numpy(rs.standard_normal(2)).to(dev)
    x = torch.from_numpy(logits).to(dtype).to(dev).requires_grad_(True)
    got = losses.softmax_dice_sums(x, y, None, 4)
    ((got[0] * gi).sum() + (got[1] * gp).sum() + (got[3] * gce).sum()).backward()
    x64 = x.detach().double().requires_grad_(True)
    m = (y != 4).unsqueeze(1)
    onehot = (torch.nn.functional.one_hot(y.clamp(max=3), 4).permute(0, 4, 1, 2, 3).bool() & m).double()
    p = torch.softmax(x64, 1)
    ce = -(torch.log_softmax(x64, 1) * onehot).sum((1, 2, 3, 4))
    want = ((p * onehot).sum((2, 3, 4)), (p * m).sum((2, 3, 4)), onehot.sum((2, 3, 4)), ce, m.sum((1, 2, 3, 4)).double())
    ((want[0] * gi).sum() + (want[1] * gp).sum() + (want[3] * gce).sum()).backward()
    assert_sums([t.detach() for t in got], [t.detach().cpu() for t in want], ("multi-workgroup", dtype))
    wg = x64.grad.cpu().numpy()
    err = np.abs(x.grad.double().cpu().numpy() - wg)
    print(f"multi-workgroup {dtype}: gradient error {float(err.max()):.3e} of {float(np.abs(wg).max()):.3e}; "
          f"worst relative error of I, P {WORST['IP']:.3e}, of CE {WORST['CE']:.3e}")
    assert (err <= grad_bound(wg, dtype)).all()
    assert (x.grad[(y == 4).unsqueeze(1).expand_as(x.grad)] == 0).all()
    # the class
    x2 = x.detach().clone().requires_grad_(True)
    loss = losses.DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, ignore_label=4, device_sums=True)(x2, y)
    loss.backward()
    x64b = x.detach().double().requires_grad_(True)
    p = torch.softmax(x64b, 1)
    inter, pred, gt = (p * onehot).sum((0, 2, 3, 4)), (p * m).sum((0, 2, 3, 4)), onehot.sum((0, 2, 3, 4))
    ce = -(torch.log_softmax(x64b, 1) * onehot).sum() / m.sum()
    wl = ce - ((2 * inter + 1e-5) / torch.clip(2 * inter + (pred - inter) + (gt - inter) + 1e-5, 1e-8))[1:].mean()
    wl.backward()
    assert abs(float(loss.detach()) - float(wl.detach())) <= LOSS_RTOL * abs(float(wl.detach()))
    wg = x64b.grad.cpu().numpy()
    assert (np.abs(x2.grad.double().cpu().numpy() - wg) <= grad_bound(wg, dtype)).all()
