"""Checks shared by tests/test_emu_augment.py (kernel sources on the CPU emulator) and tests/test_gpu_augment.py (the HIP library):
every function takes the loaded library and the device its tensors live on.  Reference: tests/augment_ref.py, the numpy float64
restatements that tests/test_augment_ref_cpu.py pins to scipy.

Spline values are held to |got - want| <= 2^-23 |want| + 2^-40 max|x| (one rounding to fp32 plus fp64 reordering), at every voxel
whose source coordinate is not within 1e-9 of a face; labels are equal at every voxel where no label's weight is within 1e-9 of 0.5;
for the matrices used here neither exclusion removes a voxel, which the checks assert.  Nearest zoom is equal.  Blur is held to
3 * 2^-23 max|x|: one possibly flipped fp32 rounding per pass, and weights that are non-negative and sum to one."""
import os

import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd.augment import DeviceAugmenter, SplineAugmenter
from segmamba_amd.dataloading import PatchLoader
from segmamba_amd.trainer import SyntheticBraTS
from tests import augment_ref as AR
from tests import preprocess_ref as R
from tests.preprocess_checks import dev_t

NEW_EXPORTS = ("segm_spline_coefs", "segm_spline_coefs_workspace_bytes", "segm_affine_spline3", "segm_affine_labels",
               "segm_zoom_nearest", "segm_gauss_blur")
MATRICES = [((0.3, -0.2, 0.45), 0.85), ((-0.52, 0.52, 0.1), 1.35), ((0.0, 0.0, 0.0), 0.7)]
THIN_MATRICES = [((0.05, -0.04, 0.03), 0.7)]
MIN_INSIDE = 0.2


def _np(t):
    return t.cpu().numpy()


def _volumes(shape, seed):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal(shape) * (1.0 + 50.0 * rng.random_sample(shape[:2] + (1, 1, 1))) + 3.0).astype(np.float32)


_REF = {}


def warp_reference(x, matrix, key):
    """the float64 reference of one volume under one matrix, computed once per key"""
    if key not in _REF:
        want, p = AR.affine_spline3_ref(x, matrix)
        want.setflags(write=False)
        _REF[key] = (want, p)
    return _REF[key]


def warp_within(got, x, matrix, key, name):
    """one volume against the restatement; -> (worst error / bound, share of voxels inside the volume)"""
    want, p = warp_reference(x, matrix, key)
    assert got.dtype == np.float32 and got.shape == want.shape, (name, got.shape)
    keep = ~AR.near_face(p, x.shape).reshape(x.shape)
    assert keep.all(), (name, "a source coordinate lies within 1e-9 of a face", int((~keep).sum()))
    share = float(AR.inside(p, x.shape).mean())
    bound = AR.data_bound(want, float(np.abs(x).max()))
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print(f"warp {name}: worst error / bound {worst:.3f}, inside {share:.2f}")
    assert (err <= bound).all(), (name, worst)
    return worst, share


# ---- 1. coefficients ------------------------------------------------------------------------------------------------------------------
COEF_SHAPES = [(12, 14, 16), (7, 33, 9), (5, 2, 300), (6, 1, 9), (1, 1, 1), (3, 45, 4)]


def check_coefs(lib, dev):
    """fp64 coefficients within 2^-40 max|x| of spline_filter(mode='mirror'): lines shorter than the FIR's 32 taps and the 40-term
    start value, lines longer than both, two row tiles, sides of 1; samples that are off are not written"""
    for i, shape in enumerate(COEF_SHAPES):
        x = _volumes((2, 3) + shape, 30 + i)
        got = _np(ops_raw.spline_coefs(lib, dev_t(x, dev)))
        assert got.dtype == np.float64 and got.shape == x.shape
        for n in range(2):
            for c in range(3):
                want = AR.spline_coefs_ref(x[n, c])
                err = float(np.abs(got[n, c] - want).max())
                assert err <= 2.0 ** -40 * float(np.abs(x[n, c]).max()), (shape, n, c, err)
    x = _volumes((3, 2, 6, 7, 8), 40)
    t = dev_t(x, dev)
    a, b = ops_raw.spline_coefs(lib, t, [True, False, True]), ops_raw.spline_coefs(lib, t, [True, False, True])
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]), "two calls must be bit-equal"
    assert torch.equal(a[2], ops_raw.spline_coefs(lib, t[2:3])[0])


# ---- 2. the warp ----------------------------------------------------------------------------------------------------------------------
def check_warp(lib, dev):
    """Every case keeps all its voxels (none within 1e-9 of a face).  At least 20 % of the compared voxels lie inside the volume: per
    case on the two regular shapes, and over all compared voxels together.  The thin volume (5, 2, 300) under its small rotation keeps
    9 % inside (x reaches 150 voxels from the centre, so a rotation of 0.04 moves z by up to 6 of its 5 voxels): there the check asks
    for at least 250 inside voxels, every one of them with taps mirrored across the 2-voxel side."""
    worst, n_inside, n_all = 0.0, 0, 0
    for i, (shape, cases) in enumerate((((12, 14, 16), MATRICES), ((7, 33, 9), MATRICES), ((5, 2, 300), THIN_MATRICES))):
        N, C = len(cases), 2
        x = _volumes((N, C) + shape, 50 + i)
        mats = np.stack([AR.affine_matrix(a, s, shape) for a, s in cases])
        t = dev_t(x, dev)
        got = _np(ops_raw.affine_spline3(lib, t, ops_raw.spline_coefs(lib, t), mats))
        for n in range(N):
            for c in range(C):
                w, share = warp_within(got[n, c], x[n, c], mats[n], ("warp", i, n, c), f"{shape} matrix {n} channel {c}")
                worst = max(worst, w)
                n_inside, n_all = n_inside + share * x[n, c].size, n_all + x[n, c].size
                assert share >= MIN_INSIDE if min(shape) > 2 else share * x[n, c].size >= 250, (shape, n, share)
    assert n_inside >= MIN_INSIDE * n_all, (n_inside, n_all)
    print(f"warp: worst error / bound over all cases {worst:.3f}, inside {n_inside / n_all:.2f}")


def check_warp_flags_and_views(lib, dev):
    """1 to 8 samples with mixed flags: off samples bit-equal to the input, on samples within the bound; strided channel views;
    two calls bit-equal; cval"""
    shape = (12, 14, 16)
    x = _volumes((8, 1) + shape, 60)
    all_mats = np.stack([AR.affine_matrix(*MATRICES[n % 3], shape) for n in range(8)])
    for N in range(1, 9):
        on = [(n * 5 + N) % 3 != 0 for n in range(N)]
        if N == 4:
            on = [False] * 4
        t = dev_t(x[:N], dev)
        coefs = ops_raw.spline_coefs(lib, t, on)
        got = ops_raw.affine_spline3(lib, t, coefs, all_mats[:N], on)
        assert torch.equal(got, ops_raw.affine_spline3(lib, t, ops_raw.spline_coefs(lib, t, on), all_mats[:N], on)), "two calls must be bit-equal"
        got = _np(got)
        for n in range(N):
            if on[n]:
                warp_within(got[n, 0], x[n, 0], all_mats[n], ("flags", n), f"{N} samples, sample {n}")
            else:
                assert np.array_equal(got[n].view(np.uint32), x[n].view(np.uint32)), (N, n)
    big = _volumes((3, 6, 12, 18, 40), 61)
    for j, view in enumerate((lambda a: a[:, ::2, :, 1:15, 3:19], lambda a: a[1:3, 1:5, :, 2:16, 20:36], lambda a: a[::2, :2, :, ::1, 8:24][:, :, :, 3:17])):
        host, t = np.ascontiguousarray(view(big)), view(dev_t(big, dev))
        assert not t.is_contiguous() and t.stride(-1) == 1 and host.shape[2:] == shape
        N = host.shape[0]
        on = [True] * N
        on[-1] = N == 1
        got = _np(ops_raw.affine_spline3(lib, t, ops_raw.spline_coefs(lib, t, on), all_mats[:N], on))
        for n in range(N):
            for c in range(host.shape[1]):
                if on[n]:
                    warp_within(got[n, c], host[n, c], all_mats[n], ("view", j, n, c), f"view {j} sample {n} channel {c}")
                else:
                    assert np.array_equal(got[n, c], host[n, c])
    t = dev_t(x[:1], dev)
    got = _np(ops_raw.affine_spline3(lib, t, ops_raw.spline_coefs(lib, t), all_mats[1:2], cval=-7.5))
    outside = ~AR.inside(AR.source_points(all_mats[1], AR.output_points(shape)), shape).reshape(shape)
    assert outside.any() and (got[0, 0][outside] == -7.5).all()


# ---- 3. labels ------------------------------------------------------------------------------------------------------------------------
def check_labels(lib, dev):
    for dt in (np.int16, np.int64):
        seg = AR.nested_boxes(dtype=dt)
        assert {1, 2, 4, 300} <= set(np.unique(seg).tolist())
        cases = [AR.affine_matrix(a, s, seg.shape) for a, s in MATRICES]
        dyadic = AR.affine_matrix((0.0, 0.0, 0.0), 1.0, seg.shape, shift=(0.0, 0.0, 0.5))
        mats = np.stack(cases + [dyadic, cases[0]])
        on = [True, True, True, True, False]
        batch = dev_t(np.stack([seg] * 5), dev)
        got_t = ops_raw.affine_labels(lib, batch, mats, on)
        assert got_t.dtype == batch.dtype and torch.equal(got_t, ops_raw.affine_labels(lib, batch, mats, on))
        got = _np(got_t)
        for n in range(4):
            want, weights, p = AR.affine_labels_ref(seg, mats[n])
            ties = AR.near_ties(weights)
            if n < 3:
                assert not ties.any(), (n, "a weight within 1e-9 of one half", int(ties.sum()))
                assert AR.inside(p, seg.shape).mean() >= MIN_INSIDE
            else:                                      # the half-voxel shift: weights of exactly one half, and they decide
                assert ties.any() and all(np.isin(r, (-1.0, 0.0, 0.5, 1.0)).all() for r in weights.values())
                both = (weights[1] == 0.5) & (weights[2] == 0.5)
                assert both.any() and (want.reshape(-1)[both] == 2).all(), "two labels at one half: the larger wins"
                assert (want.reshape(-1)[~AR.inside(p, seg.shape)] == 0).all() and (~AR.inside(p, seg.shape)).any()
            assert np.array_equal(got[n], want), (dt, n, int((got[n] != want).sum()))
            assert len(np.unique(want)) >= 4
        assert np.array_equal(got[4], seg), "a sample that is off is copied"


# ---- 4. order-0 zoom ------------------------------------------------------------------------------------------------------------------
NEAREST_CASES = [((16, 16, 12), (8, 12, 9)), ((10, 1, 5), (5, 1, 8)), ((12, 10, 16), (9, 5, 12)), ((5, 6, 7), (8, 6, 3)), ((1, 1, 1), (2, 3, 1))]


def check_zoom_nearest(lib, dev):
    rng = np.random.RandomState(70)
    for shape, new in NEAREST_CASES:
        x = rng.standard_normal((3,) + shape).astype(np.float32)
        got = _np(ops_raw.zoom_nearest(lib, dev_t(x, dev), new))
        for c in range(3):
            assert np.array_equal(got[c], AR.zoom_nearest_ref(x[c], new)), (shape, new, c)
    big = rng.standard_normal((4, 16, 18, 24)).astype(np.float32)
    host, t = np.ascontiguousarray(big[::2, :, 1:17, 4:20]), dev_t(big, dev)[::2, :, 1:17, 4:20]
    got = _np(ops_raw.zoom_nearest(lib, t, (8, 12, 12)))
    for c in range(2):
        assert np.array_equal(got[c], AR.zoom_nearest_ref(host[c], (8, 12, 12)))


# ---- 5. blur --------------------------------------------------------------------------------------------------------------------------
SIGMAS = (0.5, 0.62, 0.63, 0.87, 0.88, 1.0)


def check_blur(lib, dev):
    worst = 0.0
    for i, shape in enumerate(((10, 12, 14), (3, 5, 40))):
        x = _volumes((2, 4) + shape, 80 + i)
        sigma = [SIGMAS[v % 6] for v in range(8)]
        on = [v != 6 for v in range(8)]               # every sigma once, one volume off, one sigma twice
        t = dev_t(x, dev)
        got_t = ops_raw.gauss_blur(lib, t, sigma, on)
        assert torch.equal(got_t, ops_raw.gauss_blur(lib, t, sigma, on)), "two calls must be bit-equal"
        got = _np(got_t)
        for v in range(8):
            n, c = divmod(v, 4)
            if not on[v]:
                assert np.array_equal(got[n, c].view(np.uint32), x[n, c].view(np.uint32))
                continue
            want = AR.gauss_blur_ref(x[n, c], sigma[v])
            bound = 3.0 * 2.0 ** -23 * float(np.abs(x[n, c]).max())
            err = float(np.abs(got[n, c].astype(np.float64) - want.astype(np.float64)).max())
            worst = max(worst, err / bound)
            print(f"blur {shape} sigma {sigma[v]}: error / bound {err / bound:.3f}, bit-equal {np.array_equal(got[n, c], want)}")
            assert err <= bound, (shape, sigma[v], err / bound)
    view = dev_t(_volumes((2, 4, 10, 14, 20), 82), dev)[:, ::2, :, 1:13, 2:16]
    got = _np(ops_raw.gauss_blur(lib, view, [0.7, 0.9, 1.0, 0.55], [True, False, True, True]))
    host = _np(view)
    for v, s in ((0, 0.7), (2, 1.0), (3, 0.55)):
        n, c = divmod(v, 2)
        assert np.abs(got[n, c].astype(np.float64) - AR.gauss_blur_ref(host[n, c], s)).max() <= 3.0 * 2.0 ** -23 * np.abs(host[n, c]).max()
    assert np.array_equal(got[0, 1], host[0, 1])
    none = ops_raw.gauss_blur(lib, view, [0.7] * 4, [False] * 4)
    assert torch.equal(none, view)
    print(f"blur: worst error / bound {worst:.3f}")


# ---- 6. SplineAugmenter ---------------------------------------------------------------------------------------------------------------
class Forced(SplineAugmenter):
    """the coins of the named transforms always fall on, every other coin off"""

    def __init__(self, *a, force=(), **kw):
        super().__init__(*a, **kw)
        self.force = tuple(force)

    def _coin(self, name, p, *shape):
        super()._coin(name, p, *shape)                 # the stream of draws stays what it is
        return np.full(shape, name in self.force, dtype=bool)


def _batch(dev, seed=90, shape=(2, 3, 12, 14, 16)):
    x = _volumes(shape, seed)
    seg = np.stack([AR.nested_boxes(shape[2:], np.int64, high=3), np.roll(AR.nested_boxes(shape[2:], np.int64, high=3), 2, 2)])
    return x, seg, dev_t(x, dev), dev_t(seg, dev)


def check_augmenter_transforms(lib, dev):
    """spatial, blur and low resolution each forced on once and replayed from the host's own draws through the restatements"""
    x, seg, tx, ty = _batch(dev)
    B, C = x.shape[:2]
    shape = x.shape[2:]
    # spatial
    plan = Forced(dev, seed=11, force=("rotation", "scale")).draw(B, C, shape)
    aug = Forced(dev, seed=11, force=("rotation", "scale"))
    gx, gy = aug(tx, ty)
    assert gx.dtype == tx.dtype and gy.dtype == ty.dtype and gx.shape == tx.shape and gy.shape == ty.shape
    assert plan["spatial_on"].all() and not plan["blur_on"].any() and not plan["lowres_on"].any() and not plan["mirror"].any()
    gx, gy = _np(gx), _np(gy)
    for b in range(B):
        m = plan["matrices"][b]
        assert not np.allclose(m[:, :3], np.eye(3), atol=1e-2)
        for c in range(C):
            w, share = warp_within(gx[b, c], x[b, c], m, ("aug", b, c), f"augmenter sample {b} channel {c}")
        want, weights, p = AR.affine_labels_ref(seg[b], m)
        keep = ~AR.near_ties(weights).reshape(shape)
        assert keep.mean() >= 0.999 and np.array_equal(gy[b][keep], want[keep])
        assert set(np.unique(gy[b]).tolist()) <= {0, 1, 2, 3, 4}
    # blur
    plan = Forced(dev, seed=12, force=("blur", "blur_channel")).draw(B, C, shape)
    gx, gy = Forced(dev, seed=12, force=("blur", "blur_channel"))(tx, ty)
    assert torch.equal(gy, ty)
    gx = _np(gx)
    for b in range(B):
        for c in range(C):
            s = float(plan["blur_sigma"][b, c])
            assert 0.5 <= s <= 1.0
            want = AR.gauss_blur_ref(x[b, c], s)
            assert np.abs(gx[b, c].astype(np.float64) - want).max() <= 3.0 * 2.0 ** -23 * np.abs(x[b, c]).max(), (b, c, s)
    # low resolution
    plan = Forced(dev, seed=13, force=("lowres", "lowres_channel")).draw(B, C, shape)
    gx, gy = Forced(dev, seed=13, force=("lowres", "lowres_channel"))(tx, ty)
    assert torch.equal(gy, ty)
    gx = _np(gx)
    from tests import resample_ref as RR
    for b in range(B):
        for c in range(C):
            small_shape = tuple(int(v) for v in plan["lowres_shape"][b, c])
            assert small_shape == tuple(max(1, int(v)) for v in np.round(np.asarray(shape) * plan["lowres_zoom"][b, c]).astype(int))
            small = AR.zoom_nearest_ref(x[b, c], small_shape)
            want = RR.zoom_ref(small, shape, 3, clip=True)
            err = np.abs(gx[b, c].astype(np.float64) - want)
            assert (err <= RR.data_bound(want, float(np.abs(small).max()))).all(), (b, c, small_shape)


def check_augmenter_behaviour(lib, dev):
    """same seed -> bit-equal output, shapes and dtypes kept, labels still classes, the input untouched, an all-off call returns its
    input, more than 8 samples / channels go through in groups"""
    x, seg, tx, ty = _batch(dev, 91)
    x0, y0 = tx.clone(), ty.clone()
    runs = []
    for _ in range(2):
        aug = SplineAugmenter(dev, seed=7)
        runs.append([aug(tx, ty) for _ in range(6)])
    seen_change = False
    for (a, la), (b, lb) in zip(*runs):
        assert torch.equal(a, b) and torch.equal(la, lb)
        assert a.shape == tx.shape and a.dtype == tx.dtype and la.shape == ty.shape and la.dtype == ty.dtype
        assert torch.isfinite(a).all() and set(np.unique(_np(la)).tolist()) <= {0, 1, 2, 3, 4}
        seen_change = seen_change or not torch.equal(a, tx)
    assert seen_change and torch.equal(tx, x0) and torch.equal(ty, y0)
    gx, gy = Forced(dev, seed=1, mirror_axes=())(tx, ty)
    assert torch.equal(gx, tx) and torch.equal(gy, ty)
    # every transform at once, int16 labels too
    everything = ("rotation", "scale", "noise", "blur", "blur_channel", "brightness", "contrast", "lowres", "lowres_channel",
                  "gamma_inverted", "gamma", "mirror")
    gx, gy = Forced(dev, seed=2, force=everything)(tx, ty.to(torch.int16))
    assert gx.shape == tx.shape and gy.dtype == torch.int16 and torch.isfinite(gx).all() and torch.equal(tx, x0)
    # groups: 9 samples of 9 channels
    rng = np.random.RandomState(5)
    wide = dev_t(rng.standard_normal((9, 9, 4, 5, 6)).astype(np.float32), dev)
    lab = dev_t(rng.randint(0, 4, (9, 4, 5, 6)).astype(np.int64), dev)
    force = ("rotation", "blur", "blur_channel")
    plan = Forced(dev, seed=3, force=force).draw(9, 9, (4, 5, 6))
    gx, gy = Forced(dev, seed=3, force=force)(wide, lab)
    one = ops_raw.affine_spline3(lib, wide[8:9, 8:9], ops_raw.spline_coefs(lib, wide[8:9, 8:9]), plan["matrices"][8:9])
    assert torch.equal(gx[8:9, 8:9], ops_raw.gauss_blur(lib, one, [plan["blur_sigma"][8, 8]]))
    assert torch.equal(gy[8:9], ops_raw.affine_labels(lib, lab[8:9], plan["matrices"][8:9]))


def check_feeders(dev):
    """PatchLoader / SyntheticBraTS: "spline" selects SplineAugmenter and returns what True returns in shape and dtype; True still
    constructs DeviceAugmenter; False / None stay off"""
    def loader(augment):
        return PatchLoader(R.patch_standin_dataset(), R.PATCH_SIZE, batch_size=2, device=dev, augment=augment, seed=3)
    assert type(loader(True).augmenter) is DeviceAugmenter and type(loader("spline").augmenter) is SplineAugmenter
    assert loader(False).augmenter is None and loader(None).augmenter is None
    np.random.seed(1)
    a, la = loader(True).next()
    np.random.seed(1)
    spline = loader("spline")
    b, lb = spline.next()
    assert a.shape == b.shape and a.dtype == b.dtype and la.shape == lb.shape and la.dtype == lb.dtype and b.device == a.device
    assert torch.isfinite(b).all() and set(np.unique(_np(lb)).tolist()) <= {0, 1, 2, 3}
    for _ in range(3):
        b, lb = spline.next()
        assert b.shape == a.shape and lb.dtype == la.dtype
    assert type(SyntheticBraTS(1, 8, torch.device(dev), augment=True).augmenter) is DeviceAugmenter
    data = SyntheticBraTS(1, 8, torch.device(dev), seed=42, augment="spline")
    assert type(data.augmenter) is SplineAugmenter
    image, label = data.next()
    assert tuple(image.shape) == (1, 4, 8, 8, 8) and image.dtype == torch.float32 and label.dtype == torch.int64


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    rng = np.random.RandomState(9)
    x = dev_t(rng.standard_normal((2, 2, 6, 7, 8)).astype(np.float32), dev)
    seg = dev_t(rng.randint(0, 3, (2, 6, 7, 8)).astype(np.int16), dev)
    mats = np.stack([AR.affine_matrix(*MATRICES[0], (6, 7, 8))] * 2)
    coefs = ops_raw.spline_coefs(lib, x)
    nine = x[:1].repeat(1, 5, 1, 1, 1)[:, :9]
    for call in (lambda: ops_raw.spline_coefs(lib, x[0]),                                          # wrong rank
                 lambda: ops_raw.spline_coefs(lib, x.double()),                                    # wrong dtype
                 lambda: ops_raw.spline_coefs(lib, nine),                                          # more than 8 channels
                 lambda: ops_raw.spline_coefs(lib, x.repeat(5, 1, 1, 1, 1)[:9]),                   # more than 8 samples
                 lambda: ops_raw.spline_coefs(lib, x[..., ::2]),                                   # non-unit x stride
                 lambda: ops_raw.spline_coefs(lib, x, [True]),
                 lambda: ops_raw.spline_coefs(lib, torch.empty(1, 1, 1, 1, 2049, device=dev)),     # a side above 2048
                 lambda: ops_raw.affine_spline3(lib, x, coefs.float(), mats),
                 lambda: ops_raw.affine_spline3(lib, x, coefs[:1], mats),
                 lambda: ops_raw.affine_spline3(lib, x, coefs, mats[:1]),
                 lambda: ops_raw.affine_spline3(lib, x, coefs, mats * np.nan),
                 lambda: ops_raw.affine_spline3(lib, x[..., ::2], coefs[..., ::2].contiguous(), mats),
                 lambda: ops_raw.affine_spline3(lib, nine, ops_raw.spline_coefs(lib, nine[:, :8]), mats[:1]),
                 lambda: ops_raw.affine_labels(lib, seg[0], mats),
                 lambda: ops_raw.affine_labels(lib, seg.float(), mats),
                 lambda: ops_raw.affine_labels(lib, seg.to(torch.int32), mats),
                 lambda: ops_raw.affine_labels(lib, seg[..., ::2], mats),
                 lambda: ops_raw.affine_labels(lib, seg, mats[:1]),
                 lambda: ops_raw.zoom_nearest(lib, x, (3, 4, 4)),                                  # wrong rank
                 lambda: ops_raw.zoom_nearest(lib, x[0].double(), (3, 4, 4)),
                 lambda: ops_raw.zoom_nearest(lib, x[0], (2049, 4, 4)),
                 lambda: ops_raw.zoom_nearest(lib, x[0], (0, 4, 4)),
                 lambda: ops_raw.zoom_nearest(lib, x[0], (4, 4)),
                 lambda: ops_raw.zoom_nearest(lib, x[0][..., ::2], (3, 4, 4)),
                 lambda: ops_raw.zoom_nearest(lib, nine[0], (3, 4, 4)),
                 lambda: ops_raw.gauss_blur(lib, x[0], [0.7] * 2),
                 lambda: ops_raw.gauss_blur(lib, x.double(), [0.7] * 4),
                 lambda: ops_raw.gauss_blur(lib, x, [0.7] * 3),
                 lambda: ops_raw.gauss_blur(lib, x, [0.7, 0.7, 1.2, 0.7]),                         # radius 5
                 lambda: ops_raw.gauss_blur(lib, x, [0.7, 0.0, 0.7, 0.7]),
                 lambda: ops_raw.gauss_blur(lib, x[..., ::2], [0.7] * 4),
                 lambda: ops_raw.gauss_blur(lib, nine, [0.7] * 9)):
        with pytest.raises(RuntimeError):
            call()
    ops_raw.gauss_blur(lib, x, [0.7, 0.7, 1.2, 0.7], [True, True, False, True])                    # an off volume's sigma is not read
    # the C entries refuse what the wrappers would have refused, without touching the device
    dll = lib.dll
    for fn in (dll.segm_spline_coefs, dll.segm_affine_spline3, dll.segm_affine_labels, dll.segm_zoom_nearest, dll.segm_gauss_blur):
        assert fn(None) == -1
    assert dll.segm_spline_coefs(L.SplineCoefsArgs()) == -1 and dll.segm_gauss_blur(L.GaussBlurArgs()) == -1
    assert dll.segm_spline_coefs_workspace_bytes(2, 2, 6, 7, 8) == 2 * 2 * 6 * 7 * 8 * 8
    for bad in ((9, 2, 6, 7, 8), (2, 9, 6, 7, 8), (2, 2, 6, 7, 2049), (2, 2, 0, 7, 8), (0, 2, 6, 7, 8)):
        assert dll.segm_spline_coefs_workspace_bytes(*bad) == 0, bad

    def coef_args(**kw):
        a = L.SplineCoefsArgs()
        a.samples, a.channels, a.depth, a.height, a.width = 2, 2, 6, 7, 8
        a.stride_n, a.stride_c, a.stride_z, a.stride_y = x.stride()[:4]
        a.on[:2] = [1, 1]
        a.data, a.workspace, a.workspace_bytes, a.stream = x.data_ptr(), coefs.data_ptr(), coefs.numel() * 8, L.stream_handle(x)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert dll.segm_spline_coefs(coef_args()) == 0
    for kw in ({"channels": 9}, {"samples": 9}, {"width": 2049}, {"depth": 0}, {"stride_y": 7}, {"stride_n": -1}):
        assert dll.segm_spline_coefs(coef_args(**kw)) == -2, kw
    assert dll.segm_spline_coefs(coef_args(workspace_bytes=coefs.numel() * 8 - 8)) == -6 and dll.segm_spline_coefs(coef_args(workspace=None)) == -6
    assert dll.segm_spline_coefs(coef_args(depth=2048, height=2048, width=1024, workspace_bytes=1 << 62)) == -2    # 2^32 voxels
    out = torch.empty_like(x)

    def blur_args(**kw):
        a = L.GaussBlurArgs()
        a.samples, a.channels, a.depth, a.height, a.width = 2, 2, 6, 7, 8
        a.stride_n, a.stride_c, a.stride_z, a.stride_y = x.stride()[:4]
        a.sigma[:4], a.on[:4] = [0.7] * 4, [1] * 4
        a.data, a.out, a.workspace, a.workspace_bytes = x.data_ptr(), out.data_ptr(), coefs.data_ptr(), x.numel() * 4
        a.stream = L.stream_handle(x)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert dll.segm_gauss_blur(blur_args()) == 0
    for kw in ({"channels": 9}, {"height": 2049}, {"stride_y": 7}):
        assert dll.segm_gauss_blur(blur_args(**kw)) == -2, kw
    a = blur_args()
    a.sigma[1] = 1.2
    assert dll.segm_gauss_blur(a) == -2
    assert dll.segm_gauss_blur(blur_args(workspace_bytes=x.numel() * 4 - 4)) == -6 and dll.segm_gauss_blur(blur_args(workspace=None)) == -6
    b = L.AffineLabelsArgs()
    b.seg, b.out = seg.data_ptr(), out.data_ptr()
    b.samples, b.depth, b.height, b.width = 2, 6, 7, 2049
    assert dll.segm_affine_labels(b) == -2
    b.width, b.wide = 8, 2
    assert dll.segm_affine_labels(b) == -4
    c = L.ZoomNearestArgs()
    c.data, c.out = x.data_ptr(), out.data_ptr()
    c.channels, c.depth, c.height, c.width, c.out_depth, c.out_height, c.out_width = 9, 6, 7, 8, 3, 3, 3
    c.stride_c, c.stride_z, c.stride_y = 336, 56, 8
    assert dll.segm_zoom_nearest(c) == -2


def check_needs_the_library():
    """on host tensors that the library does not take the augmenter names its requirement"""
    with pytest.raises(RuntimeError, match="HIP library"):
        SplineAugmenter("cpu")(torch.zeros(1, 1, 4, 4, 4), torch.zeros(1, 4, 4, 4, dtype=torch.long))


# ---- 8. exports -----------------------------------------------------------------------------------------------------------------------
def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
