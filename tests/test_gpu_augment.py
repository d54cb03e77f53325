"""Augmentation at the reference's interpolation orders (segmamba_amd/augment.py `SplineAugmenter` on csrc/augment.hip) on the HIP
library: the checks of tests/test_emu_augment.py on the GPU, the warp at 2 x 4 x 128^3 against the float64 restatement on a random
sample of voxels, and a call under torch's synchronisation debug mode."""
import numpy as np
import pytest
import torch

from tests import augment_checks as K
from tests import augment_ref as AR
from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd.augment import SplineAugmenter

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


def test_spline_coefficients(hip):
    K.check_coefs(hip, DEV)


def test_cubic_warp(hip):
    K.check_warp(hip, DEV)


def test_cubic_warp_flags_and_views(hip):
    K.check_warp_flags_and_views(hip, DEV)


def test_labels(hip):
    K.check_labels(hip, DEV)


def test_nearest_zoom(hip):
    K.check_zoom_nearest(hip, DEV)


def test_gaussian_blur(hip):
    K.check_blur(hip, DEV)


def test_augmenter_transforms_replayed(hip):
    K.check_augmenter_transforms(hip, DEV)


def test_augmenter_behaviour(hip):
    K.check_augmenter_behaviour(hip, DEV)


def test_feeders(hip):
    K.check_feeders(DEV)


def test_refusals(hip):
    K.check_refusals(hip, DEV)


def test_needs_the_library(hip):
    K.check_needs_the_library()


def test_new_exports(hip):
    K.check_exports(hip)


def test_warp_at_training_size(hip):
    """2 x 4 x 128^3, both samples rotated and scaled: 4 096 random output voxels per channel within the bound of the float64
    restatement (its coefficients over the whole volume, its values at the sample), the labels equal on the same sample"""
    shape, B, C = (128, 128, 128), 2, 4
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, C, *shape, device=DEV, generator=g) * 30.0 + 2.0
    idx = np.indices(shape).astype(np.float64)
    r2 = sum(((idx[a] - 63.5 - 5 * a) / (50.0 - 6 * a)) ** 2 for a in range(3))
    seg0 = (r2 < 1.0).astype(np.int64) + (r2 < 0.5) + 2 * (r2 < 0.15)                     # classes 0, 1, 2, 4
    seg = np.stack([seg0, seg0[::-1].copy()])
    mats = np.stack([AR.affine_matrix((0.3, -0.2, 0.45), 0.85, shape), AR.affine_matrix((-0.52, 0.52, 0.1), 1.35, shape)])
    got = ops_raw.affine_spline3(hip, x, ops_raw.spline_coefs(hip, x), mats).cpu().numpy()
    got_seg = ops_raw.affine_labels(hip, torch.from_numpy(seg).to(DEV), mats).cpu().numpy()
    host = x.cpu().numpy()
    rng = np.random.RandomState(6)
    for b in range(B):
        pts = np.stack([rng.randint(0, n, 4096) for n in shape], 1)
        p = AR.source_points(mats[b], pts.astype(np.float64))
        assert not AR.near_face(p, shape).any()
        inside = AR.inside(p, shape)
        assert inside.mean() >= K.MIN_INSIDE, inside.mean()
        at = (pts[:, 0], pts[:, 1], pts[:, 2])
        for c in range(C):
            want = AR.spline_values(AR.spline_coefs_ref(host[b, c]), p)
            err = np.abs(got[b, c][at].astype(np.float64) - want)
            bound = AR.data_bound(want, float(np.abs(host[b, c]).max()))
            print(f"sample {b} channel {c}: worst error / bound {float((err / bound).max()):.3f}, inside {inside.mean():.2f}")
            assert (err <= bound).all(), (b, c, float((err / bound).max()))
        want_seg, weights = AR.labels_at(seg[b], p)
        keep = ~AR.near_ties(weights)
        assert keep.mean() >= 0.999 and np.array_equal(got_seg[b][at][keep], want_seg[keep])
        assert len(np.unique(want_seg)) == 4


def test_a_call_does_not_wait_for_the_device(hip):
    """one `__call__` with every transform on under torch.cuda.set_sync_debug_mode("error"): no device-to-host copy, no
    synchronisation"""
    everything = ("rotation", "scale", "noise", "blur", "blur_channel", "brightness", "contrast", "lowres", "lowres_channel",
                  "gamma_inverted", "gamma", "mirror")
    x = torch.randn(2, 3, 12, 14, 16, device=DEV)
    y = torch.randint(0, 4, (2, 12, 14, 16), device=DEV)
    aug = K.Forced(DEV, seed=4, force=everything)
    aug(x, y)                                          # warm-up: allocations, lazy initialisation
    plain = SplineAugmenter(DEV, seed=4)
    plain(x, y)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        honoured = False
        try:
            torch.ones(1, device=DEV).item()           # harmless probe: does this build raise on a synchronising call?
        except RuntimeError:
            honoured = True
        if honoured:
            gx, gy = aug(x, y)
            for _ in range(4):
                plain(x, y)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    if not honoured:
        pytest.skip("this torch build does not raise under set_sync_debug_mode('error')")
    assert gx.shape == x.shape and gy.shape == y.shape and torch.isfinite(gx).all()
