"""Checks shared by tests/test_emu_intensity.py (kernel sources on the CPU emulator) and tests/test_gpu_intensity.py (the HIP library):
every function takes the loaded library and the device its tensors live on.  Reference: tests/intensity_ref.py (numpy float64).

NOISE, SCALE and a plane with no op on (the mirror's copy) are held bit-equal to the ATen expressions of `SplineAugmenter`.  CONTRAST
and GAMMA are held per channel to |got - want| <= k * 2^-24 * max|want| against the float64 restatement, with k from the error of
the parent's own ATen route on the same inputs (below).  Statistics: mean and sd within 1e-12 relative of numpy's float64 results,
min and max exact."""
import contextlib
import os

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd.augment import DeviceAugmenter, FusedAugmenter, SplineAugmenter, select_augmenter
from segmamba_amd.dataloading import PatchLoader
from segmamba_amd.trainer import SyntheticBraTS
from tests import intensity_ref as IR
from tests import preprocess_ref as R
from tests.preprocess_checks import dev_t

NEW_EXPORTS = ("segm_intensity_workspace_bytes", "segm_intensity_stats", "segm_intensity_apply")
ROW = L.INTENSITY_STATS_DOUBLES
EPS24 = 2.0 ** -24

# The worst |y_aten - y_ref| / (2^-24 max|y_ref|) per channel of the parent's ATen route - the contrast lines of
# `SplineAugmenter.__call__` and `SplineAugmenter._gamma`, on CPU tensors in fp32 - against tests/intensity_ref.py on the inputs of
# `pointwise_cases()` (measured by `aten_ratios()`, which tests/test_emu_intensity.py runs again and prints).  k is twice that ratio
# and no less than 4: the kernels multiply by a reciprocal and contract products where ATen divides and rounds each step; their
# statistics are fp64 where ATen's are fp32 reductions, so those cannot be the worse part.
ATEN_RATIO_CONTRAST = 1.76
ATEN_RATIO_GAMMA = 4.07
K_CONTRAST = max(4.0, 2.0 * ATEN_RATIO_CONTRAST)
K_GAMMA = max(4.0, 2.0 * ATEN_RATIO_GAMMA)

GAMMAS = [(g, inv) for inv in (False, True) for g in (0.7, 1.0, 1.5)]                 # one per plane of a (2, 3) batch
CONTRASTS = [(m, f) for f in (0.75, 1.25) for m in (1.0, 0.8, 1.2)]
POINTWISE_SHAPES = ((2, 3, 12, 14, 16), (2, 3, 5, 7, 9))                              # the packet route, the single-voxel route


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def volumes(shape, seed, zscore=False):
    rng = np.random.RandomState(seed)
    if zscore:
        return rng.standard_normal(shape).astype(np.float32)
    return (rng.standard_normal(shape) * (1.0 + 50.0 * rng.random_sample(shape[:2] + (1, 1, 1))) + 3.0).astype(np.float32)


def pointwise_cases():
    """(name, x (2, 3, D, H, W)) - what CONTRAST and GAMMA are judged on, by the kernels and by the ATen route alike"""
    out = []
    for i, shape in enumerate(POINTWISE_SHAPES):
        out.append((f"wide {shape[2:]}", volumes(shape, 200 + i)))
        out.append((f"z-scored {shape[2:]}", volumes(shape, 210 + i, zscore=True)))
    return out


def ratio(got, want):
    """worst |got - want| / (2^-24 max|want|) of one channel"""
    return float(np.abs(got.astype(np.float64) - want).max() / (EPS24 * np.abs(want).max()))


def aten_contrast(v, m, f):
    """one plane through the brightness and contrast lines of SplineAugmenter.__call__ (augment.py:342-348), fp32 on the host"""
    x = torch.from_numpy(v.copy())[None]
    x *= torch.full((1, 1, 1, 1), float(m), dtype=torch.float32)
    red = (1, 2, 3)
    mn, lo, hi = x.mean(red, keepdim=True), x.amin(red, keepdim=True), x.amax(red, keepdim=True)
    return torch.minimum(torch.maximum((x - mn) * torch.full((1, 1, 1, 1), float(f), dtype=torch.float32) + mn, lo), hi)[0].numpy()


def aten_gamma(v, g, invert):
    aug = SplineAugmenter.__new__(SplineAugmenter)
    x = torch.from_numpy(v.copy())[None]
    return SplineAugmenter._gamma(aug, x, SplineAugmenter._vec(aug, [g], x), invert)[0].numpy()


def aten_ratios():
    """-> (worst ratio of the ATen contrast, of the ATen gamma) over `pointwise_cases()`"""
    worst_c = worst_g = 0.0
    for name, x in pointwise_cases():
        for v, ((m, f), (g, inv)) in enumerate(zip(CONTRASTS, GAMMAS)):
            plane = x[v // 3, v % 3]
            worst_c = max(worst_c, ratio(aten_contrast(plane, m, f), IR.contrast_ref(plane, m, f)))
            worst_g = max(worst_g, ratio(aten_gamma(plane, g, inv), IR.gamma_ref(plane, g, inv)))
    return worst_c, worst_g


def check_aten_ratios():
    """the constants above are what the ATen route gives here, to the two digits they are written with; on another host's ATen build
    the route must still lie within the k it defines"""
    c, g = aten_ratios()
    print(f"ATen route against the float64 restatement: contrast {c:.3f} (recorded {ATEN_RATIO_CONTRAST}), gamma {g:.3f} "
          f"(recorded {ATEN_RATIO_GAMMA}); k = {K_CONTRAST}, {K_GAMMA}")
    assert c <= K_CONTRAST and g <= K_GAMMA


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


# ---- 1. statistics ----------------------------------------------------------------------------------------------------------------------
STAT_SHAPES = [(1, 1, 1), (1, 1, 7), (3, 3, 7), (4, 4, 4), (5, 13, 1), (3, 5, 17), (1, 1, 257), (12, 14, 16), (17, 241, 1), (40, 40, 41)]
assert [int(np.prod(s)) for s in STAT_SHAPES] == [1, 7, 63, 64, 65, 255, 257, 2688, 4097, 65600]


def stats_within(rows, host, ops, name):
    """rows (planes, 8) against numpy on the planes of host (N, C, D, H, W) that are on"""
    rows = _np(rows)
    C = host.shape[1]
    for v, op in enumerate(ops):
        if op is None:
            continue
        plane = host[v // C, v % C]
        if op[0] == "contrast":
            plane = plane * np.float32(op[1])
        elif op[2]:
            plane = -plane
        want = IR.stats_ref(plane)
        got = rows[v]
        assert got[0] == want[0] and got[3] == want[3] and got[4] == want[4], (name, v, got, want)
        for q in (1, 2):
            assert abs(got[q] - want[q]) <= 1e-12 * abs(want[q]), (name, v, q, got[q], want[q])
        assert (got[5:] == 0).all()


def check_stats(lib, dev):
    """V in {1, 7, 63, 64, 65, 255, 257, 2688, 4097, 65600}: widths that are and are not multiples of 4, several workgroups per plane,
    a plane with mean 3e4 and sd 1, two calls bit-equal"""
    for i, shape in enumerate(STAT_SHAPES):
        x = volumes((1, 2) + shape, 100 + i)
        if shape == (12, 14, 16):
            x[0, 1] = (np.random.RandomState(7).standard_normal(shape) + 3.0e4).astype(np.float32)      # the pivot's case
        ops = [("contrast", 1.0, 1.0), ("gamma", 1.0, True)]
        t = dev_t(x, dev)
        rows = ops_raw.intensity_stats(lib, t, ops)
        stats_within(rows, x, ops, shape)
        assert torch.equal(rows, ops_raw.intensity_stats(lib, t, ops)), "two calls must be bit-equal"
    big = volumes((1, 1, 40, 40, 41), 120, zscore=True) + np.float32(3.0e4)                     # mean 3e4, sd 1, 65 workgroups
    stats_within(ops_raw.intensity_stats(lib, dev_t(big, dev), [("contrast", 1.0, 1.0)]), big, [("contrast", 1.0, 1.0)], "pivot, 65 workgroups")


def check_stats_layouts(lib, dev):
    """a storage offset of one element, a 3-of-4 channel slice, padded rows and padded planes, the pre-scale; 1 plane, 64 planes, a mix
    of planes on and off"""
    big = volumes((2, 4, 7, 10, 20), 130)
    tb = dev_t(big, dev)
    views = {"channel slice": lambda a: a[:, :3], "padded rows": lambda a: a[:, :, :, :, 4:20], "padded planes": lambda a: a[:, :, 1:6, 2:9],
             "odd width": lambda a: a[:, 1:, :, :, 3:12], "packets, padded": lambda a: a[:, :, :, 1:9, 8:16]}
    for name, view in views.items():
        host, t = np.ascontiguousarray(view(big)), view(tb)
        assert not t.is_contiguous() and t.stride(-1) == 1
        planes = host.shape[0] * host.shape[1]
        ops = [("contrast", 1.0 + 0.125 * (v % 3), 1.0) if v % 2 else ("gamma", 1.0, v % 4 == 0) for v in range(planes)]
        stats_within(ops_raw.intensity_stats(lib, t, ops), host, ops, name)
    flat = dev_t(np.concatenate([np.zeros(1, np.float32), volumes((1, 2, 4, 6, 8), 131).reshape(-1)]), dev)
    off = flat[1:].view(1, 2, 4, 6, 8)                                    # packets impossible: the base is 4 bytes past 16
    assert off.storage_offset() == 1
    ops = [("contrast", 1.0, 1.0), ("gamma", 1.0, False)]
    stats_within(ops_raw.intensity_stats(lib, off, ops), _np(off), ops, "storage offset")
    one = volumes((1, 1, 4, 6, 8), 132)
    stats_within(ops_raw.intensity_stats(lib, dev_t(one, dev), [("gamma", 1.0, False)]), one, [("gamma", 1.0, False)], "1 plane")
    many = volumes((8, 8, 3, 5, 8), 133)
    ops = [("gamma", 1.0, v % 3 == 0) if v % 5 else ("contrast", 0.75, 1.0) for v in range(64)]
    stats_within(ops_raw.intensity_stats(lib, dev_t(many, dev), ops), many, ops, "64 planes")
    mixed = [op if v % 4 != 1 else (None if v % 8 == 1 else ("scale", 2.0)) for v, op in enumerate(ops)]
    marked = ops_raw.intensity_stats(lib, dev_t(many, dev), mixed)
    stats_within(marked, many, [op if op is not None and op[0] != "scale" else None for op in mixed], "planes on and off")


# ---- 2. NOISE, SCALE, COPY: the bits of ATen -------------------------------------------------------------------------------------------
def check_single_rounding_ops(lib, dev):
    """x += randn * s, x *= m and a copy, bit for bit on both routes, in place and out of place, planes that are off untouched"""
    for i, shape in enumerate(((2, 3, 4, 6, 8), (2, 3, 5, 7, 9), (1, 2, 3, 5, 16))):
        x = volumes(shape, 140 + i)
        B, C = shape[:2]
        rng = np.random.RandomState(150 + i)
        fields = rng.standard_normal(shape).astype(np.float32)
        s = rng.uniform(0.0, 0.1, B).astype(np.float32)
        m = rng.uniform(0.75, 1.25, (B, C)).astype(np.float32)
        t, tf = dev_t(x, dev), dev_t(fields, dev)
        # the ATen expressions of SplineAugmenter.__call__, on the host (one rounding per product, one per sum: the same on every device)
        want_noise, want_scale = torch.from_numpy(x.copy()), torch.from_numpy(x.copy())
        for b in range(B):
            want_noise[b] += torch.from_numpy(fields[b]) * float(s[b])
            want_scale[b] *= torch.from_numpy(m[b]).view(-1, 1, 1, 1)
        noise_ops = [("noise", float(s[v // C]), tf[v // C, v % C]) for v in range(B * C)]
        scale_ops = [("scale", float(m[v // C, v % C])) for v in range(B * C)]
        for ops, want in ((noise_ops, want_noise), (scale_ops, want_scale)):
            mixed = [op if v != 1 else None for v, op in enumerate(ops)]
            got_out = ops_raw.intensity_apply(lib, t, mixed, out_of_place=True)
            work = t.clone()
            assert ops_raw.intensity_apply(lib, work, mixed) is work
            assert torch.equal(t, dev_t(x, dev)), "the input of an out-of-place call is not written"
            for got in (_np(got_out), _np(work)):
                for v in range(B * C):
                    expect = want.numpy()[v // C, v % C] if v != 1 else x[v // C, v % C]
                    assert np.array_equal(_bits(got[v // C, v % C]), _bits(expect)), (shape, ops[0][0], v)
        copy = ops_raw.intensity_apply(lib, t, [None] * (B * C), out_of_place=True)
        assert copy.data_ptr() != t.data_ptr() and np.array_equal(_bits(_np(copy)), _bits(x))
    # the two routes on the same values: a view whose base is 4 bytes past a packet takes single voxels
    x = volumes((1, 2, 4, 6, 8), 160)
    flat = dev_t(np.concatenate([np.zeros(1, np.float32), x.reshape(-1)]), dev)
    off, t = flat[1:].view(1, 2, 4, 6, 8), dev_t(x, dev)
    field = dev_t(volumes((4, 6, 8), 161, zscore=True), dev)
    ops = [("noise", 0.07, field), ("scale", 1.1)]
    assert torch.equal(ops_raw.intensity_apply(lib, off, ops, out_of_place=True), ops_raw.intensity_apply(lib, t, ops, out_of_place=True))


# ---- 3. CONTRAST and GAMMA against the float64 restatement -----------------------------------------------------------------------------
def run_contrast(lib, t, ops, **kw):
    return ops_raw.intensity_apply(lib, t, ops, ops_raw.intensity_stats(lib, t, ops), **kw)


def run_gamma(lib, t, ops, **kw):
    stats = ops_raw.intensity_stats(lib, t, ops)
    return ops_raw.intensity_apply(lib, t, ops, stats, ops_raw.intensity_stats(lib, t, ops, 1, stats), **kw)


def check_contrast_gamma(lib, dev):
    worst_c = worst_g = 0.0
    for name, x in pointwise_cases():
        t = dev_t(x, dev)
        c_ops = [("contrast", m, f) for m, f in CONTRASTS]
        g_ops = [("gamma", g, inv) for g, inv in GAMMAS]
        got_c = run_contrast(lib, t, c_ops, out_of_place=True)
        got_g = run_gamma(lib, t, g_ops, out_of_place=True)
        assert torch.equal(got_c, run_contrast(lib, t.clone(), c_ops)) and torch.equal(got_g, run_gamma(lib, t.clone(), g_ops)), \
            "in place and out of place, and two calls, are bit-equal"
        got_c, got_g = _np(got_c), _np(got_g)
        for v in range(6):
            plane = x[v // 3, v % 3]
            rc = ratio(got_c[v // 3, v % 3], IR.contrast_ref(plane, *CONTRASTS[v]))
            rg = ratio(got_g[v // 3, v % 3], IR.gamma_ref(plane, *GAMMAS[v]))
            print(f"{name} plane {v}: contrast {CONTRASTS[v]} ratio {rc:.3f} (k {K_CONTRAST}), gamma {GAMMAS[v]} ratio {rg:.3f} (k {K_GAMMA})")
            worst_c, worst_g = max(worst_c, rc), max(worst_g, rg)
            assert rc <= K_CONTRAST, (name, v, rc)
            assert rg <= K_GAMMA, (name, v, rg)
    print(f"worst ratio: contrast {worst_c:.3f} of {K_CONTRAST}, gamma {worst_g:.3f} of {K_GAMMA}")


def check_exact_cases(lib, dev):
    """a constant channel comes back bit-equal under GAMMA and CONTRAST; a channel that CONTRAST clips touches lo and hi exactly"""
    for shape in ((1, 3, 4, 6, 8), (1, 3, 5, 7, 9)):
        x = np.empty(shape, np.float32)
        x[0, 0], x[0, 1], x[0, 2] = np.float32(3.3), np.float32(-0.7), np.float32(1.0e-3)
        t = dev_t(x, dev)
        for ops, run in (([("gamma", 0.7, False), ("gamma", 1.5, True), ("gamma", 1.0, True)], run_gamma),
                         ([("contrast", 1.0, 0.75), ("contrast", 1.0, 1.25), ("contrast", 1.0, 1.25)], run_contrast)):
            assert np.array_equal(_bits(_np(run(lib, t, ops, out_of_place=True))), _bits(x)), (shape, ops[0][0])
        y = volumes(shape, 170)
        got = _np(run_contrast(lib, dev_t(y, dev), [("contrast", 1.0, 1.25)] * 3, out_of_place=True))
        for c in range(3):
            assert got[0, c].min() == y[0, c].min() and got[0, c].max() == y[0, c].max(), (shape, c)
            assert (got[0, c] == y[0, c].max()).sum() >= 1 and (got[0, c] == y[0, c].min()).sum() >= 1


# ---- 4. mirror ---------------------------------------------------------------------------------------------------------------------------
def check_mirror(lib, dev):
    """every subset of the three axes, through a plane with no op on and through GAMMA: bit-equal to torch.flip of the unmirrored output;
    W = 8 and 16 reverse packets, W = 9 takes single voxels"""
    for i, spatial in enumerate(((5, 7, 9), (4, 6, 8), (3, 2, 16))):
        x = volumes((2, 4) + spatial, 180 + i)
        t = dev_t(x, dev)
        masks = list(range(8))                                            # plane v is flipped by the subset v
        g_ops = [("gamma", GAMMAS[v % 6][0], GAMMAS[v % 6][1]) for v in range(8)]
        stats = ops_raw.intensity_stats(lib, t, g_ops)
        stats2 = ops_raw.intensity_stats(lib, t, g_ops, 1, stats)
        plain = ops_raw.intensity_apply(lib, t, g_ops, stats, stats2, out_of_place=True)
        flipped = ops_raw.intensity_apply(lib, t, g_ops, stats, stats2, mirror=masks, out_of_place=True)
        copied = ops_raw.intensity_apply(lib, t, [None] * 8, mirror=masks, out_of_place=True)
        for v, mask in enumerate(masks):
            axes = [ax for ax in range(3) if mask >> ax & 1]
            b, c = divmod(v, 4)
            for got, base in ((flipped, plain), (copied, t)):
                want = base[b, c].flip(axes) if axes else base[b, c]
                assert torch.equal(got[b, c], want), (spatial, mask)
                assert np.array_equal(_bits(_np(got[b, c])), _bits(_np(want)))


# ---- 5. the chain without the host ------------------------------------------------------------------------------------------------------
EVERYTHING = ("rotation", "scale", "noise", "blur", "blur_channel", "brightness", "contrast", "lowres", "lowres_channel",
              "gamma_inverted", "gamma", "mirror")


def check_chain(lib, dev):
    """brightness + contrast and both gammas back to back, every statistic read from the device rows; then one whole FusedAugmenter
    call with every coin on.  On the GPU under set_sync_debug_mode("error"): a copy to the host or a wait raises."""
    x = volumes((2, 3, 12, 14, 16), 190)
    t = dev_t(x, dev)
    c_ops = [("contrast", m, f) for m, f in CONTRASTS]
    inv_ops = [("gamma", g, True) for g, _ in GAMMAS]
    g_ops = [("gamma", g, False) for g, _ in reversed(GAMMAS)]
    aug = ForcedFused(dev, seed=21, force=EVERYTHING)
    tx, ty = batch(dev)
    with no_sync(dev):
        a = run_contrast(lib, t, c_ops, out_of_place=True)
        b = run_gamma(lib, a.clone(), inv_ops)                            # in place on a tensor of its own
        c = run_gamma(lib, b, g_ops, mirror=[5] * 6, out_of_place=True)
        gx, gy = aug(tx, ty)
    a, b, c = _np(a), _np(b), _np(c)
    for v in range(6):                                                    # every op judged from the fp32 input it was given
        i = (v // 3, v % 3)
        assert ratio(a[i], IR.contrast_ref(x[i], *CONTRASTS[v])) <= K_CONTRAST, v
        assert ratio(b[i], IR.gamma_ref(a[i], inv_ops[v][1], True)) <= K_GAMMA, v
        assert ratio(c[i], IR.gamma_ref(b[i], g_ops[v][1], False)[::-1, :, ::-1]) <= K_GAMMA, v
    assert gx.shape == tx.shape and gx.dtype == tx.dtype and gy.shape == ty.shape and gy.dtype == ty.dtype
    assert torch.isfinite(gx).all()


# ---- 6. FusedAugmenter -------------------------------------------------------------------------------------------------------------------
class Forced(SplineAugmenter):
    """the coins of the named transforms always fall on, every other coin off; the stream of draws stays what it is"""

    def __init__(self, *a, force=(), **kw):
        super().__init__(*a, **kw)
        self.force = tuple(force)

    def _coin(self, name, p, *shape):
        super()._coin(name, p, *shape)
        return np.full(shape, name in self.force, dtype=bool)


class ForcedFused(FusedAugmenter):
    def __init__(self, *a, force=(), **kw):
        super().__init__(*a, **kw)
        self.force = tuple(force)

    def _coin(self, name, p, *shape):
        super()._coin(name, p, *shape)
        return np.full(shape, name in self.force, dtype=bool)


def batch(dev, seed=220, shape=(2, 3, 12, 14, 16)):
    x = volumes(shape, seed)
    rng = np.random.RandomState(seed + 1)
    seg = rng.randint(0, 4, (shape[0],) + shape[2:]).astype(np.int64)
    return dev_t(x, dev), dev_t(seg, dev)


def channels_within(got, want_fn, k, name):
    """got (B, C, ...) device tensor; want_fn(b, c) -> float64 plane"""
    got = _np(got)
    for b in range(got.shape[0]):
        for c in range(got.shape[1]):
            r = ratio(got[b, c], want_fn(b, c))
            print(f"{name} sample {b} channel {c}: ratio {r:.3f} of {k}")
            assert r <= k, (name, b, c, r)


def check_augmenter_single_transforms(lib, dev):
    """each new transform forced on alone, with SplineAugmenter's seed: labels bit-equal; images bit-equal for noise, brightness and
    mirror, within the bounds of the restatement for contrast and the gammas"""
    tx, ty = batch(dev)
    x = _np(tx)
    B, C = x.shape[:2]
    x0, y0 = tx.clone(), ty.clone()
    for name in ("noise", "brightness", "contrast", "gamma_inverted", "gamma", "mirror"):
        plan = Forced(dev, seed=31, force=(name,)).draw(B, C, x.shape[2:])
        sx, sy = Forced(dev, seed=31, force=(name,))(tx, ty)
        fx, fy = ForcedFused(dev, seed=31, force=(name,))(tx, ty)
        assert torch.equal(fy, sy) and fy.dtype == sy.dtype, name
        assert fx.shape == sx.shape and fx.dtype == sx.dtype and fx.is_contiguous()
        assert not torch.equal(fx, tx), name
        if name in ("noise", "brightness", "mirror"):
            assert np.array_equal(_bits(_np(fx)), _bits(_np(sx))), name
        elif name == "contrast":
            channels_within(fx, lambda b, c: IR.contrast_ref(x[b, c], 1.0, plan["contrast"][b, c]), K_CONTRAST, name)
        else:
            key = "gamma_inv" if name == "gamma_inverted" else "gamma"
            channels_within(fx, lambda b, c: IR.gamma_ref(x[b, c], plan[key][b, c], name == "gamma_inverted"), K_GAMMA, name)
        assert torch.equal(tx, x0) and torch.equal(ty, y0), "the input is not modified"


def spline_stages(aug, lib, image, label):
    """SplineAugmenter.__call__ step by step -> the plan and the tensor after each step (the walk is checked against the call itself)"""
    B, C = image.shape[:2]
    plan = aug.draw(B, C, tuple(image.shape[2:]))
    st = {}
    x, y = aug._spatial(lib, image, label, plan) if aug.spatial else (image, label)
    x, y = x.clone(), y.clone()
    st["spatial"] = x.clone()
    for b in np.nonzero(plan["noise_on"])[0]:
        x[b] += torch.randn(x.shape[1:], device=x.device, generator=aug.g, dtype=x.dtype) * float(plan["noise_scale"][b])
    st["noise"] = x.clone()
    x = aug._blur(lib, x, plan).clone()
    st["blur"] = x.clone()
    for b in np.nonzero(plan["bright_on"])[0]:
        x[b] *= aug._vec(plan["bright"][b], x)
    for b in np.nonzero(plan["contrast_on"])[0]:
        v, red = x[b], (1, 2, 3)
        mn, lo, hi = v.mean(red, keepdim=True), v.amin(red, keepdim=True), v.amax(red, keepdim=True)
        x[b] = torch.minimum(torch.maximum((v - mn) * aug._vec(plan["contrast"][b], x) + mn, lo), hi)
    st["contrast"] = x.clone()
    x, _ = aug._low_res(lib, x, plan, True)
    st["lowres"] = x.clone()
    for key, invert in (("gamma_inv", True), ("gamma", False)):
        for b in np.nonzero(plan[key + "_on"])[0]:
            x[b] = aug._gamma(x[b], aug._vec(plan[key][b], x), invert)
        st[key] = x.clone()
    for b in range(B):
        axes = [ax for j, ax in enumerate(aug.mirror_axes) if plan["mirror"][b, j]]
        if axes:
            x[b] = x[b].flip([1 + ax for ax in axes])
            y[b] = y[b].flip(axes)
    st["mirror"], st["label"] = x, y
    return plan, st


def check_augmenter_everything(lib, dev):
    """all twelve coins on: labels bit-equal to SplineAugmenter's (int64 and int16), and each group of new ops judged from
    SplineAugmenter's own intermediate - noise bit-equal, brightness + contrast, inverted gamma and gamma + mirror within their bounds"""
    tx, ty = batch(dev, 230)
    x0, y0 = tx.clone(), ty.clone()
    B, C = tx.shape[:2]
    sx, sy = Forced(dev, seed=41, force=EVERYTHING)(tx, ty)
    plan, st = spline_stages(Forced(dev, seed=41, force=EVERYTHING), lib, tx, ty)
    assert torch.equal(st["mirror"], sx) and torch.equal(st["label"], sy), "the walk is SplineAugmenter's call"
    fused = ForcedFused(dev, seed=41, force=EVERYTHING)
    fx, fy = fused(tx, ty)
    assert torch.equal(fy, sy) and fx.shape == sx.shape and fx.dtype == sx.dtype and torch.isfinite(fx).all()
    _, fy16 = ForcedFused(dev, seed=41, force=EVERYTHING)(tx, ty.to(torch.int16))
    assert fy16.dtype == torch.int16 and torch.equal(fy16, sy.to(torch.int16))
    assert torch.equal(tx, x0) and torch.equal(ty, y0), "the input is not modified"
    again = ForcedFused(dev, seed=41, force=EVERYTHING)(tx, ty)
    assert torch.equal(again[0], fx) and torch.equal(again[1], fy), "the same seed twice"
    # the groups, each from the parent's intermediate
    walker = ForcedFused(dev, seed=41, force=EVERYTHING)
    assert all(np.array_equal(a, b) for a, b in zip(walker.draw(B, C, tuple(tx.shape[2:])).values(), plan.values()))
    got, _ = walker._pass(lib, st["spatial"], walker._noise_ops(st["spatial"], plan), False)
    assert got.data_ptr() != st["spatial"].data_ptr() and np.array_equal(_bits(_np(got)), _bits(_np(st["noise"]))), "noise"
    blur = _np(st["blur"])
    got, _ = walker._pass(lib, st["blur"], walker._contrast_ops(B, C, plan), False)
    channels_within(got, lambda b, c: IR.contrast_ref(blur[b, c], plan["bright"][b, c], plan["contrast"][b, c]), K_CONTRAST, "brightness + contrast")
    low = _np(st["lowres"])
    got, _ = walker._pass(lib, st["lowres"], walker._gamma_ops(B, C, plan, "gamma_inv", True), False)
    channels_within(got, lambda b, c: IR.gamma_ref(low[b, c], plan["gamma_inv"][b, c], True), K_GAMMA, "inverted gamma")
    inv = _np(st["gamma_inv"])
    masks = walker._mirror_masks(B, plan)
    assert all(m == 7 for m in masks)
    got, _ = walker._pass(lib, st["gamma_inv"], walker._gamma_ops(B, C, plan, "gamma", False), True, masks)
    assert got.data_ptr() != st["gamma_inv"].data_ptr()
    channels_within(got, lambda b, c: IR.gamma_ref(inv[b, c], plan["gamma"][b, c], False)[::-1, ::-1, ::-1], K_GAMMA, "gamma + mirror")


def check_augmenter_behaviour(lib, dev):
    """same seed -> bit-equal output over several draws; all coins off returns the inputs; 9 samples of 9 channels go through in
    groups; host tensors raise"""
    tx, ty = batch(dev, 240)
    x0, y0 = tx.clone(), ty.clone()
    runs = []
    for _ in range(2):
        aug = FusedAugmenter(dev, seed=7)
        runs.append([aug(tx, ty) for _ in range(6)])
    changed = False
    for (a, la), (b, lb) in zip(*runs):
        assert torch.equal(a, b) and torch.equal(la, lb)
        assert a.shape == tx.shape and a.dtype == tx.dtype and la.shape == ty.shape and la.dtype == ty.dtype and torch.isfinite(a).all()
        changed = changed or not torch.equal(a, tx)
    assert changed and torch.equal(tx, x0) and torch.equal(ty, y0)
    spline = SplineAugmenter(dev, seed=7)
    for a, la in runs[0]:                                                 # the parent's plan, noise and labels for the seed
        sa, sla = spline(tx, ty)
        assert torch.equal(la, sla)
    gx, gy = ForcedFused(dev, seed=1)(tx, ty)
    assert gx is tx and gy is ty, "every coin off: the inputs come back"
    rng = np.random.RandomState(5)
    wide = dev_t(rng.standard_normal((9, 9, 4, 5, 6)).astype(np.float32), dev)
    lab = dev_t(rng.randint(0, 4, (9, 4, 5, 6)).astype(np.int64), dev)
    force = ("noise", "brightness", "mirror")
    sx, sy = Forced(dev, seed=3, force=force)(wide, lab)
    fx, fy = ForcedFused(dev, seed=3, force=force)(wide, lab)
    assert torch.equal(fy, sy) and np.array_equal(_bits(_np(fx)), _bits(_np(sx))), "81 planes in groups"
    w = _np(wide)
    plan = Forced(dev, seed=4, force=("brightness", "contrast")).draw(9, 9, (4, 5, 6))
    fx, _ = ForcedFused(dev, seed=4, force=("brightness", "contrast"))(wide, lab)
    channels_within(fx, lambda b, c: IR.contrast_ref(w[b, c], plan["bright"][b, c], plan["contrast"][b, c]), K_CONTRAST, "81 planes, contrast")
    plan = Forced(dev, seed=4, force=("gamma_inverted",)).draw(9, 9, (4, 5, 6))
    fx, _ = ForcedFused(dev, seed=4, force=("gamma_inverted",))(wide, lab)
    channels_within(fx, lambda b, c: IR.gamma_ref(w[b, c], plan["gamma_inv"][b, c], True), K_GAMMA, "81 planes, inverted gamma")


def check_needs_the_library():
    with pytest.raises(RuntimeError, match="HIP library"):
        FusedAugmenter("cpu")(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.long))


# ---- 7. feeders ---------------------------------------------------------------------------------------------------------------------------
def check_feeders(dev):
    assert select_augmenter("fused") is FusedAugmenter and select_augmenter("spline") is SplineAugmenter
    assert select_augmenter(True) is DeviceAugmenter and issubclass(FusedAugmenter, SplineAugmenter)

    def loader(augment):
        return PatchLoader(R.patch_standin_dataset(), R.PATCH_SIZE, batch_size=2, device=dev, augment=augment, seed=3)
    assert type(loader("fused").augmenter) is FusedAugmenter and type(loader("spline").augmenter) is SplineAugmenter
    assert type(loader(True).augmenter) is DeviceAugmenter and loader(False).augmenter is None
    np.random.seed(1)
    a, la = loader("spline").next()
    np.random.seed(1)
    fused = loader("fused")
    b, lb = fused.next()
    assert a.shape == b.shape and a.dtype == b.dtype and la.shape == lb.shape and la.dtype == lb.dtype and b.device == a.device
    assert torch.equal(la, lb) and torch.isfinite(b).all()
    for _ in range(3):
        b, lb = fused.next()
        assert b.shape == a.shape and lb.dtype == la.dtype
    data = SyntheticBraTS(1, 8, torch.device(dev), seed=42, augment="fused")
    assert type(data.augmenter) is FusedAugmenter
    image, label = data.next()
    assert tuple(image.shape) == (1, 4, 8, 8, 8) and image.dtype == torch.float32 and label.dtype == torch.int64


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    """every refusal of the wrappers and of the C entries; a refused call launches nothing: the data and the rows stay what they were"""
    x = dev_t(volumes((2, 2, 4, 6, 8), 250), dev)
    keep = x.clone()
    field = dev_t(volumes((4, 6, 8), 251, zscore=True), dev)
    g_ops = [("gamma", 0.7, False)] * 4
    stats = ops_raw.intensity_stats(lib, x, g_ops)
    stats2 = ops_raw.intensity_stats(lib, x, g_ops, 1, stats)
    for call in (lambda: ops_raw.intensity_stats(lib, x[0], g_ops),                                       # wrong rank
                 lambda: ops_raw.intensity_stats(lib, x.double(), g_ops),                                 # wrong dtype
                 lambda: ops_raw.intensity_stats(lib, x[..., ::2], g_ops),                                # non-unit x stride
                 lambda: ops_raw.intensity_stats(lib, x.repeat(9, 2, 1, 1, 1)[:13, :5], g_ops * 17),      # 65 planes
                 lambda: ops_raw.intensity_stats(lib, x[:0], []),                                         # 0 planes
                 lambda: ops_raw.intensity_stats(lib, x, g_ops[:3]),
                 lambda: ops_raw.intensity_stats(lib, x, g_ops, 2),
                 lambda: ops_raw.intensity_stats(lib, x, g_ops, 1),                                       # stage 1 without the rows
                 lambda: ops_raw.intensity_stats(lib, x, g_ops, 1, stats.float()),
                 lambda: ops_raw.intensity_stats(lib, x, g_ops, 1, stats[:3]),
                 lambda: ops_raw.intensity_stats(lib, x, [("sharpen", 1.0)] * 4),                         # an unknown op
                 lambda: ops_raw.intensity_stats(lib, x, [("gamma", 0.7)] * 4),
                 lambda: ops_raw.intensity_stats(lib, x, [("gamma", float("nan"), False)] * 4),
                 lambda: ops_raw.intensity_apply(lib, x, g_ops),                                          # gamma without rows
                 lambda: ops_raw.intensity_apply(lib, x, g_ops, stats),
                 lambda: ops_raw.intensity_apply(lib, x, [("contrast", 1.0, 1.25)] * 4),
                 lambda: ops_raw.intensity_apply(lib, x, [None] * 4, mirror=[1, 0, 0, 0]),                # a mirror in place
                 lambda: ops_raw.intensity_apply(lib, x, [None] * 4, mirror=[8, 0, 0, 0], out_of_place=True),
                 lambda: ops_raw.intensity_apply(lib, x, [None] * 4, mirror=[1, 0, 0], out_of_place=True),
                 lambda: ops_raw.intensity_apply(lib, x, [("noise", 0.1, field[:2])] * 4),
                 lambda: ops_raw.intensity_apply(lib, x, [("noise", 0.1, field.double())] * 4),
                 lambda: ops_raw.intensity_apply(lib, x, [("noise", 0.1, field[..., ::2])] * 4),
                 lambda: ops_raw.intensity_apply(lib, x, [("noise", 0.1, None)] * 4),
                 lambda: ops_raw.intensity_apply(lib, x[..., ::2], [("scale", 1.1)] * 4)):
        with pytest.raises(RuntimeError):
            call()
    # the C entries
    dll = lib.dll
    assert dll.segm_intensity_stats(None) == -1 and dll.segm_intensity_apply(None) == -1
    assert dll.segm_intensity_workspace_bytes(4, 4 * 6 * 8) == 4 * 1 * 5 * 8
    assert dll.segm_intensity_workspace_bytes(2, 40 * 40 * 41) == 2 * 65 * 5 * 8
    for bad in ((0, 100), (65, 100), (4, 0), (4, 1 << 31)):
        assert dll.segm_intensity_workspace_bytes(*bad) == 0, bad
    ws = torch.empty(4 * 5, dtype=torch.float64, device=x.device)
    out = torch.empty_like(x)
    marked = torch.full((4, ROW), -5.0, dtype=torch.float64, device=x.device)

    def args(**kw):
        a = L.IntensityArgs()
        a.samples, a.channels, a.depth, a.height, a.width = 2, 2, 4, 6, 8
        a.stride_n, a.stride_c, a.stride_z, a.stride_y = x.stride()[:4]
        a.stride_x = 1
        a.op[:4], a.a[:4] = [L.INTENSITY_GAMMA] * 4, [0.7] * 4
        a.data, a.stats, a.stats2 = x.data_ptr(), marked.data_ptr(), stats2.data_ptr()
        a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws.numel() * 8, L.stream_handle(x)
        for k, v in kw.items():
            if k in ("op", "mirror"):
                getattr(a, k)[:len(v)] = v
            else:
                setattr(a, k, v)
        return a
    shape_cases = ({"samples": 0}, {"channels": 0}, {"samples": 13, "channels": 5}, {"depth": 0}, {"width": 0}, {"stride_x": 2},
                   {"stride_x": 0}, {"stride_y": 7}, {"stride_n": -1}, {"depth": 2048, "height": 1024, "width": 1024}, {"stage": 2})
    for kw in shape_cases:
        assert dll.segm_intensity_stats(args(**kw)) == -2, kw
        if "stage" not in kw:
            assert dll.segm_intensity_apply(args(stats=stats.data_ptr(), **kw)) == -2, kw
    assert dll.segm_intensity_stats(args(op=[L.INTENSITY_GAMMA, 5])) == -4 and dll.segm_intensity_apply(args(op=[9])) == -4
    assert dll.segm_intensity_stats(args(data=None)) == -1 and dll.segm_intensity_stats(args(stats=None)) == -1
    assert dll.segm_intensity_stats(args(stage=1, stats2=None)) == -1
    for kw in ({"workspace": None}, {"workspace_bytes": ws.numel() * 8 - 8}, {"workspace": ws.data_ptr() + 4}):
        assert dll.segm_intensity_stats(args(**kw)) == -6, kw
    assert dll.segm_intensity_apply(args(data=None)) == -1 and dll.segm_intensity_apply(args(stats=None)) == -1
    assert dll.segm_intensity_apply(args(stats=stats.data_ptr(), stats2=None)) == -1
    assert dll.segm_intensity_apply(args(op=[L.INTENSITY_NOISE] * 4)) == -1                               # no noise plane
    assert dll.segm_intensity_apply(args(op=[0] * 4, mirror=[1])) == -2                                   # a mirror in place
    assert dll.segm_intensity_apply(args(op=[0] * 4, mirror=[1], out=x.data_ptr())) == -2
    assert dll.segm_intensity_apply(args(op=[0] * 4, mirror=[8], out=out.data_ptr(), out_stride_n=x.stride(0), out_stride_c=x.stride(1),
                                         out_stride_z=x.stride(2), out_stride_y=x.stride(3))) == -2
    assert dll.segm_intensity_apply(args(op=[0] * 4, out=out.data_ptr(), out_stride_y=7)) == -2
    assert torch.equal(x, keep) and bool((marked == -5.0).all()), "a refused call launches nothing"
    # what is not refused: no plane takes part -> nothing to do
    assert dll.segm_intensity_stats(args(op=[0, L.INTENSITY_SCALE, L.INTENSITY_NOISE, 0], workspace=None, stats=None)) == 0
    assert dll.segm_intensity_apply(args(op=[0] * 4)) == 0 and torch.equal(x, keep)
    assert dll.segm_intensity_stats(args()) == 0 and torch.equal(marked, stats)


# ---- 9. exports ---------------------------------------------------------------------------------------------------------------------------
def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    assert os.path.exists(os.path.join(root, "segmamba_amd", "csrc", "intensity.hip"))
    for name in ("intensity_stats", "intensity_apply"):
        assert callable(getattr(ops_raw, name))
