"""Device-side training augmentation: the feeder that replaces the reference's 18-process batchgenerators pipeline.

The reference augments on the host (light_training/trainer.py:154-162 starts NonDetMultiThreadedAugmenter workers running
`get_train_transforms`, light_training/augment/train_augment.py:24-66) and ships each batch over PCIe.  Here the batch is
already resident on the GPU (`SyntheticBraTS`, or a real loader's pinned upload) and the same chain runs there as a
handful of elementwise / resampling ops per step - a few hundred microseconds, no worker processes, no host round trip.

The chain, in the reference's order and with its parameters (train_augment.py:30-60).  `batchgenerators` itself is a
third-party dependency that is NOT in the reference tree (setup: pip `batchgenerators`, unpinned); what each transform does
is restated from its published implementation:

  SpatialTransform         rotation about x / y / z by U(-30 deg, 30 deg) with p 0.2, isotropic scale with p 0.2 drawn two-sided - U(0.7, 1) or U(1, 1.4)
                           with equal odds, batchgenerators' rule for a range straddling 1 -
                           about the patch centre, zero padding; image cubic spline / label linear in the reference ->
                           trilinear / nearest here (grid_sample has no 3-D cubic mode); labels outside the volume become 0
                           (RemoveLabelTransform(-1, 0), :57)
  GaussianNoise            p 0.1: x += N(0, s), s ~ U(0, 0.1)   (batchgenerators passes its "variance" as numpy's scale)
  GaussianBlur             p 0.2, each channel with p 0.5: separable gaussian, sigma ~ U(0.5, 1) per channel; the kernel is cut at
                           radius 3 (>= 3 sigma) and the border replicated, where scipy's gaussian_filter cuts at 4 sigma and
                           reflects: differences below 1e-3 of the kernel mass, at the border voxels only
  BrightnessMultiplicative p 0.15: each channel x U(0.75, 1.25)
  ContrastAugmentation     p 0.15: each channel (x - mean) f + mean, f from (0.75, 1) or (1, 1.25) with equal odds, clipped
                           to the channel's former range
  SimulateLowResolution    p 0.25, each channel with p 0.5: nearest down by U(0.5, 1), back up (cubic in the reference ->
                           trilinear here)
  Gamma (inverted image)   p 0.1;  Gamma  p 0.3: per channel, gamma from (0.7, 1) or (1, 1.5) with equal odds on the
                           range-normalised channel, mean / std retained
  Mirror                   each of the three axes with p 0.5, image and label together

Every random decision comes from one torch.Generator on the device (reproducible per rank: seed 42 + rank, trainer.py:331).
`SplineAugmenter` below runs the same chain at the reference's interpolation orders on the kernels of csrc/augment.hip.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from . import lib as L
from . import ops_raw


class DeviceAugmenter:
    def __init__(self, device, seed: int = 42, mirror_axes=(0, 1, 2), spatial: bool = True):
        self.g = torch.Generator(device=device).manual_seed(seed)
        self.device = torch.device(device)
        self.mirror_axes = tuple(mirror_axes or ())
        self.spatial = spatial

    # ---- random helpers (all on the device generator) ------------------------------------------------------------------
    def _u(self, lo, hi, *shape):
        return lo + (hi - lo) * torch.rand(*shape, device=self.device, generator=self.g)

    def _coin(self, p, *shape):
        return torch.rand(*shape, device=self.device, generator=self.g) < p

    def _two_sided(self, lo, hi, *shape):
        """batchgenerators' contrast / gamma sampling: (lo, 1) or (max(lo, 1), hi) with equal odds"""
        low = self._u(lo, 1.0, *shape)
        high = self._u(max(lo, 1.0), hi, *shape)
        return torch.where(self._coin(0.5, *shape), low, high)

    # ---- transforms -------------------------------------------------------------------------------------------------------
    def _spatial(self, x, y):
        B = x.shape[0]
        rot = self._coin(0.2, B)
        scl = self._coin(0.2, B)
        if not bool((rot | scl).any()):
            return x, y
        a = self._u(-math.pi / 6, math.pi / 6, B, 3) * rot[:, None]
        s = torch.where(scl, self._two_sided(0.7, 1.4, B), torch.ones(B, device=self.device))
        cx, sx, cy, sy, cz, sz = a[:, 0].cos(), a[:, 0].sin(), a[:, 1].cos(), a[:, 1].sin(), a[:, 2].cos(), a[:, 2].sin()
        one, zero = torch.ones_like(cx), torch.zeros_like(cx)
        Rx = torch.stack([one, zero, zero, zero, cx, -sx, zero, sx, cx], 1).view(B, 3, 3)
        Ry = torch.stack([cy, zero, sy, zero, one, zero, -sy, zero, cy], 1).view(B, 3, 3)
        Rz = torch.stack([cz, -sz, zero, sz, cz, zero, zero, zero, one], 1).view(B, 3, 3)
        M = (Rz @ Ry @ Rx) * s[:, None, None]              # output coordinate -> input coordinate (scale > 1 zooms out)
        theta = torch.cat([M, torch.zeros(B, 3, 1, device=self.device)], 2)
        grid = F.affine_grid(theta, list(x.shape), align_corners=False)
        x = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        y = F.grid_sample(y[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)[:, 0].to(y.dtype)
        return x, y

    def _blur(self, x):
        B, C = x.shape[:2]
        on = self._coin(0.2, B)[:, None] & self._coin(0.5, B, C)
        if not bool(on.any()):
            return x
        sigma = self._u(0.5, 1.0, B, C)
        r = 3                                               # 3 sigma at sigma <= 1
        t = torch.arange(-r, r + 1, device=self.device, dtype=x.dtype)
        k = torch.exp(-0.5 * (t[None, None] / sigma[:, :, None]) ** 2)
        k = k / k.sum(-1, keepdim=True)                      # (B, C, 7)
        ident = torch.zeros_like(k)
        ident[:, :, r] = 1
        k = torch.where(on[:, :, None], k, ident).reshape(B * C, 1, 2 * r + 1)
        v = x.reshape(1, B * C, *x.shape[2:])
        for dim in range(3):                                # separable: one 1-D depthwise convolution per axis
            shape = [B * C, 1, 1, 1, 1]
            shape[2 + dim] = 2 * r + 1
            pad = [0, 0, 0, 0, 0, 0]
            pad[2 * (2 - dim)] = pad[2 * (2 - dim) + 1] = r
            v = F.conv3d(F.pad(v, pad, mode="replicate"), k.reshape(shape), groups=B * C)
        return v.reshape(x.shape)

    def _low_res(self, x):
        B, C = x.shape[:2]
        on = self._coin(0.25, B)[:, None] & self._coin(0.5, B, C)
        if not bool(on.any()):
            return x
        zoom = self._u(0.5, 1.0, B, C)
        out = x.clone()
        for b, c in on.nonzero().tolist():                  # few (sample, channel) pairs per step; each has its own grid size
            size = [max(1, int(round(d * float(zoom[b, c])))) for d in x.shape[2:]]
            small = F.interpolate(x[b:b + 1, c:c + 1], size=size, mode="nearest")
            out[b, c] = F.interpolate(small, size=list(x.shape[2:]), mode="trilinear", align_corners=False)[0, 0]
        return out

    def _gamma(self, x, p, invert):
        B, C = x.shape[:2]
        on = self._coin(p, B)
        if not bool(on.any()):
            return x
        v = -x if invert else x
        red = (2, 3, 4)
        mn, sd = v.mean(red, keepdim=True), v.std(red, keepdim=True)
        lo = v.amin(red, keepdim=True)
        rng = v.amax(red, keepdim=True) - lo
        gam = self._two_sided(0.7, 1.5, B, C)[:, :, None, None, None]
        w = ((v - lo) / (rng + 1e-7)).clamp_min(0).pow(gam) * rng + lo
        w = w - w.mean(red, keepdim=True)
        w = w / (w.std(red, keepdim=True) + 1e-8) * sd + mn
        if invert:
            w = -w
        return torch.where(on[:, None, None, None, None], w, x)

    def __call__(self, image: torch.Tensor, label: torch.Tensor):
        """image (B, C, D, H, W) float, label (B, D, H, W) integer class map -> augmented copies (same shapes / dtypes)"""
        x, y = image, label
        B, C = x.shape[:2]
        if self.spatial:
            x, y = self._spatial(x, y)
        noise = self._coin(0.1, B)
        if bool(noise.any()):
            s = self._u(0.0, 0.1, B) * noise
            x = x + torch.randn(x.shape, device=self.device, generator=self.g, dtype=x.dtype) * s[:, None, None, None, None]
        x = self._blur(x)
        bright = self._coin(0.15, B)
        x = x * torch.where(bright[:, None], self._u(0.75, 1.25, B, C), torch.ones(B, C, device=self.device))[:, :, None, None, None]
        con = self._coin(0.15, B)
        if bool(con.any()):
            red = (2, 3, 4)
            mn, lo, hi = x.mean(red, keepdim=True), x.amin(red, keepdim=True), x.amax(red, keepdim=True)
            f = self._two_sided(0.75, 1.25, B, C)[:, :, None, None, None]
            x = torch.where(con[:, None, None, None, None], torch.minimum(torch.maximum((x - mn) * f + mn, lo), hi), x)
        x = self._low_res(x)
        x = self._gamma(x, 0.1, invert=True)
        x = self._gamma(x, 0.3, invert=False)
        for ax in self.mirror_axes:
            flip = self._coin(0.5, B)
            if bool(flip.any()):
                x = torch.where(flip[:, None, None, None, None], x.flip(2 + ax), x)
                y = torch.where(flip[:, None, None, None], y.flip(1 + ax), y)
        return x.contiguous(), y.contiguous()


class SplineAugmenter:
    """The chain of `DeviceAugmenter` with the three stencil / gather transforms at the reference's interpolation orders, on the
    kernels of csrc/augment.hip, and with every decision drawn on the host.  Same call signature, output shapes and dtypes.

      SpatialTransform       data: cubic spline, `map_coordinates(order=3, mode='constant', cval=0)` on fp64 coefficients
                             (`ops_raw.spline_coefs` -> `affine_spline3`); label: linear per label with the `>= 0.5` rule
                             (`affine_labels`, 0 outside the volume).  Output voxel (z, y, x) of a sample reads the input at
                             M ((z, y, x) - c) + c, c = (n - 1) / 2, M = s (Rx Ry Rz)^T with
                             Rx = [[1,0,0],[0,c,-s],[0,s,c]], Ry = [[c,0,s],[0,1,0],[-s,0,c]], Rz = [[c,-s,0],[s,c,0],[0,0,1]]:
                             batchgenerators' create_zero_centered_coordinate_mesh / rotate_coords_3d / scale_coords with
                             random_crop=False, restated from the published source (batchgenerators is not in the reference tree).
                             Angles U(-30 deg, 30 deg) for the three axes with p 0.2 per sample, scale two-sided on (0.7, 1.4)
                             with p 0.2 per sample; a sample with neither passes through bit-equal.
      GaussianBlur           `scipy.ndimage.gaussian_filter` (truncate 4 sigma, reflect, fp32 between the passes): `gauss_blur`;
                             p 0.2 per sample, 0.5 per channel, sigma U(0.5, 1) per channel
      SimulateLowResolution  p 0.25 per sample, 0.5 per channel, zoom U(0.5, 1) per channel: `zoom_nearest` down to
                             round(shape * zoom), `ops_raw.zoom(order=3, clip=True)` back up
      noise, brightness, contrast, the two gammas, mirror: `DeviceAugmenter`'s ATen arithmetic, per sample that is on

    Every coin and every scalar parameter comes from one `np.random.RandomState(seed)` on the host (`draw`), so the host knows which
    transforms are on, launches only those and passes their parameters by value: a call copies nothing from the device and never
    waits for it.  Only the Gaussian noise field comes from a device generator.  The stream of draws differs from
    `DeviceAugmenter`'s: the two classes give different augmentations for one seed.  Batches of more than 8 samples or 8 channels go
    to the kernels in groups.  fp64 coefficients of the samples that are warped: B x C x D x H x W x 8 bytes (134 MB at 2 x 4 x 128^3).
    Needs the HIP library: tensors that are not on the device raise RuntimeError."""

    def __init__(self, device, seed: int = 42, mirror_axes=(0, 1, 2), spatial: bool = True):
        self.rs = np.random.RandomState(seed)
        self.g = torch.Generator(device=device).manual_seed(seed)
        self.device = torch.device(device)
        self.mirror_axes = tuple(mirror_axes or ())
        self.spatial = spatial

    # ---- host draws -------------------------------------------------------------------------------------------------------------------
    def _coin(self, name, p, *shape):
        """`name` tells a subclass which transform asks (tests force single transforms on)"""
        return self.rs.random_sample(shape) < p

    def _u(self, lo, hi, *shape):
        return lo + (hi - lo) * self.rs.random_sample(shape)

    def _two_sided(self, lo, hi, *shape):
        low, high = self._u(lo, 1.0, *shape), self._u(max(lo, 1.0), hi, *shape)
        return np.where(self.rs.random_sample(shape) < 0.5, low, high)

    @staticmethod
    def matrix(angles, scale, shape):
        """[A | t] (3, 4) float64 of one sample: output index (z, y, x) -> input coordinate"""
        cx, sx, cy, sy, cz, sz = (f(a) for a in angles for f in (math.cos, math.sin))
        Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], dtype=np.float64)
        Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], dtype=np.float64)
        Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], dtype=np.float64)
        M = float(scale) * (Rx @ Ry @ Rz).T
        ctr = (np.asarray(shape, dtype=np.float64) - 1.0) / 2.0
        return np.concatenate([M, (ctr - M @ ctr)[:, None]], 1)

    def draw(self, B, C, shape):
        """All decisions and parameters of one call, as host values, in the order of the chain."""
        plan = {}
        if self.spatial:
            rot, scl = self._coin("rotation", 0.2, B), self._coin("scale", 0.2, B)
            angles = self._u(-math.pi / 6, math.pi / 6, B, 3) * rot[:, None]
            scale = np.where(scl, self._two_sided(0.7, 1.4, B), 1.0)
            plan["spatial_on"] = rot | scl
            plan["matrices"] = np.stack([self.matrix(angles[b], scale[b], shape) for b in range(B)])
        plan["noise_on"], plan["noise_scale"] = self._coin("noise", 0.1, B), self._u(0.0, 0.1, B)
        plan["blur_on"] = self._coin("blur", 0.2, B)[:, None] & self._coin("blur_channel", 0.5, B, C)
        plan["blur_sigma"] = self._u(0.5, 1.0, B, C)
        plan["bright_on"], plan["bright"] = self._coin("brightness", 0.15, B), self._u(0.75, 1.25, B, C)
        plan["contrast_on"], plan["contrast"] = self._coin("contrast", 0.15, B), self._two_sided(0.75, 1.25, B, C)
        plan["lowres_on"] = self._coin("lowres", 0.25, B)[:, None] & self._coin("lowres_channel", 0.5, B, C)
        zoom = self._u(0.5, 1.0, B, C)
        plan["lowres_zoom"] = zoom
        plan["lowres_shape"] = np.maximum(np.round(np.asarray(shape)[None, None] * zoom[:, :, None]).astype(int), 1)
        plan["gamma_inv_on"], plan["gamma_inv"] = self._coin("gamma_inverted", 0.1, B), self._two_sided(0.7, 1.5, B, C)
        plan["gamma_on"], plan["gamma"] = self._coin("gamma", 0.3, B), self._two_sided(0.7, 1.5, B, C)
        plan["mirror"] = np.stack([self._coin("mirror", 0.5, B) for _ in self.mirror_axes], 1) if self.mirror_axes else np.zeros((B, 0), bool)
        return plan

    # ---- transforms on the kernels ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _groups(n, size):
        return [slice(i, min(i + size, n)) for i in range(0, n, size)]

    def _spatial(self, lib, x, y, plan):
        on = plan["spatial_on"]
        if not on.any():
            return x, y
        B, C = x.shape[:2]
        xs, ys = [], []
        for sb in self._groups(B, L.AUG_MAX_SAMPLES):
            flags, mats = on[sb].tolist(), plan["matrices"][sb]
            if not any(flags):
                xs.append(x[sb])
                ys.append(y[sb])
                continue
            parts = []
            for sc in self._groups(C, L.PREP_MAX_CHANNELS):
                part = x[sb, sc]
                parts.append(ops_raw.affine_spline3(lib, part, ops_raw.spline_coefs(lib, part, flags), mats, flags))
            xs.append(parts[0] if len(parts) == 1 else torch.cat(parts, 1))
            seg = y[sb]
            if seg.dtype not in (torch.int16, torch.int64):
                ys.append(ops_raw.affine_labels(lib, seg.long().contiguous(), mats, flags).to(seg.dtype))
            else:
                ys.append(ops_raw.affine_labels(lib, seg.contiguous(), mats, flags))
        return (xs[0] if len(xs) == 1 else torch.cat(xs)), (ys[0] if len(ys) == 1 else torch.cat(ys))

    def _blur(self, lib, x, plan):
        on, sigma = plan["blur_on"], plan["blur_sigma"]
        if not on.any():
            return x
        B, C = x.shape[:2]
        rows = []
        for sb in self._groups(B, L.AUG_MAX_SAMPLES):
            parts = [ops_raw.gauss_blur(lib, x[sb, sc], sigma[sb, sc].reshape(-1).tolist(), on[sb, sc].reshape(-1).tolist())
                     if on[sb, sc].any() else x[sb, sc] for sc in self._groups(C, L.PREP_MAX_CHANNELS)]
            rows.append(parts[0] if len(parts) == 1 else torch.cat(parts, 1))
        return rows[0] if len(rows) == 1 else torch.cat(rows)

    def _low_res(self, lib, x, plan, own):
        on = plan["lowres_on"]
        if not on.any():
            return x, own
        if not own:
            x, own = x.clone(), True
        full = tuple(x.shape[2:])
        for b, c in zip(*np.nonzero(on)):
            small = ops_raw.zoom_nearest(lib, x[b, c:c + 1], plan["lowres_shape"][b, c].tolist())
            x[b, c:c + 1] = ops_raw.zoom(lib, small, full, 3, True) if tuple(small.shape[1:]) != full else small
        return x, own

    # ---- per-sample ATen arithmetic, the parameters as device vectors built without a copy from the host ------------------------------
    def _vec(self, values, like):
        return torch.cat([torch.full((1,), float(v), dtype=like.dtype, device=like.device) for v in values]).view(-1, 1, 1, 1)

    def _gamma(self, v, gam, invert):
        """one sample (C, D, H, W), as DeviceAugmenter._gamma"""
        v = -v if invert else v
        red = (1, 2, 3)
        mn, sd = v.mean(red, keepdim=True), v.std(red, keepdim=True)
        lo = v.amin(red, keepdim=True)
        rng = v.amax(red, keepdim=True) - lo
        w = ((v - lo) / (rng + 1e-7)).clamp_min(0).pow(gam) * rng + lo
        w = w - w.mean(red, keepdim=True)
        w = w / (w.std(red, keepdim=True) + 1e-8) * sd + mn
        return -w if invert else w

    def __call__(self, image: torch.Tensor, label: torch.Tensor):
        """image (B, C, D, H, W) float32, label (B, D, H, W) integer class map -> augmented copies (same shapes / dtypes)"""
        if not L.on_device(image) or not L.on_device(label):
            raise RuntimeError("SplineAugmenter runs on the HIP library's kernels (csrc/augment.hip): image and label must live on "
                               "the GPU; on host tensors use DeviceAugmenter (augment=True)")
        if image.dim() != 5 or label.dim() != 4 or image.dtype != torch.float32:
            raise RuntimeError(f"SplineAugmenter: image (B, C, D, H, W) float32 and label (B, D, H, W) are required, got "
                               f"{tuple(image.shape)} {image.dtype} and {tuple(label.shape)}")
        lib = L.get_lib()
        B, C = image.shape[:2]
        plan = self.draw(B, C, tuple(image.shape[2:]))
        x, y = image, label
        if self.spatial:
            x, y = self._spatial(lib, x, y, plan)
        own = x is not image                           # whether x may be written in place
        own_y = y is not label
        for b in np.nonzero(plan["noise_on"])[0]:
            if not own:
                x, own = x.clone(), True
            x[b] += torch.randn(x.shape[1:], device=x.device, generator=self.g, dtype=x.dtype) * float(plan["noise_scale"][b])
        blurred = self._blur(lib, x, plan)
        own, x = own or blurred is not x, blurred
        for b in np.nonzero(plan["bright_on"])[0]:
            if not own:
                x, own = x.clone(), True
            x[b] *= self._vec(plan["bright"][b], x)
        for b in np.nonzero(plan["contrast_on"])[0]:
            if not own:
                x, own = x.clone(), True
            v, red = x[b], (1, 2, 3)
            mn, lo, hi = v.mean(red, keepdim=True), v.amin(red, keepdim=True), v.amax(red, keepdim=True)
            x[b] = torch.minimum(torch.maximum((v - mn) * self._vec(plan["contrast"][b], x) + mn, lo), hi)
        x, own = self._low_res(lib, x, plan, own)
        for key, invert in (("gamma_inv", True), ("gamma", False)):
            for b in np.nonzero(plan[key + "_on"])[0]:
                if not own:
                    x, own = x.clone(), True
                x[b] = self._gamma(x[b], self._vec(plan[key][b], x), invert)
        for b in range(B):
            axes = [ax for j, ax in enumerate(self.mirror_axes) if plan["mirror"][b, j]]
            if axes:
                if not own:
                    x, own = x.clone(), True
                if not own_y:
                    y, own_y = y.clone(), True
                x[b] = x[b].flip([1 + ax for ax in axes])
                y[b] = y[b].flip(axes)
        return x.contiguous(), y.contiguous()


class FusedAugmenter(SplineAugmenter):
    """`SplineAugmenter` with noise, brightness, contrast, the two gammas and the mirror on the kernels of csrc/intensity.hip in place
    of the per-sample ATen arithmetic.  `draw` and the `torch.randn` calls for the noise fields are the parent's, in the parent's
    order: for one seed the plan, the noise and the labels are `SplineAugmenter`'s.  The order of the chain is the parent's too, so
    the fusion happens inside the three groups that blur and low resolution separate:

      noise                           one apply pass
      brightness, contrast            brightness alone: one apply pass; with contrast the factor is folded into the loads of one
                                      statistics pass and one apply pass
      inverted gamma, gamma, mirror   per gamma two statistics passes (of t, then of w) and one apply pass; the flips ride on the
                                      last apply pass of the call (a plain copy pass where no gamma is on)

    A pass is one launch over up to 64 planes (sample, channel), each with its own op and parameters by value; the statistics stay
    in device memory, so a call copies nothing to the host and never waits for the device.  A pass runs in place on a tensor the call
    owns, and out of place where the batch has a flip or where the tensor is still the caller's (which is never written).  The
    standard deviation of the gammas is the population one (numpy.std, as in the published transform) where the ATen route takes the
    unbiased one; the factor cancels in sd0 / sd1 and only the 1e-8 term sees it.  The label flip stays one ATen `flip` per mirrored
    sample."""

    @staticmethod
    def _plane_groups(B, C):
        """(samples, channels) slices with at most 64 planes each"""
        cs = min(C, L.AUG_MAX_VOLUMES)
        ns = max(1, L.AUG_MAX_VOLUMES // cs)
        return [(sb, sc) for sb in SplineAugmenter._groups(B, ns) for sc in SplineAugmenter._groups(C, cs)]

    def _pass(self, lib, x, ops, own, mirror=None):
        """one fused transform of the batch: `ops[b][c]` as `ops_raw.intensity_apply` takes them, `mirror[b]` the flip mask of a
        sample -> (x, own)"""
        B, C = x.shape[:2]
        flips = mirror is not None and any(mirror)
        if not flips and not any(op is not None for row in ops for op in row):
            return x, own
        out_of_place = flips or not own
        groups = self._plane_groups(B, C)
        out = torch.empty(tuple(x.shape), dtype=x.dtype, device=x.device) if out_of_place and len(groups) > 1 else x
        for sb, sc in groups:
            part = x[sb, sc]
            flat = [op for row in ops[sb] for op in row[sc]]
            masks = [m for m in (mirror[sb] if mirror is not None else [0] * part.shape[0]) for _ in range(part.shape[1])]
            if not out_of_place and not any(op is not None for op in flat):
                continue
            stats = stats2 = None
            if any(op is not None and op[0] in ("contrast", "gamma") for op in flat):
                stats = ops_raw.intensity_stats(lib, part, flat, 0)
            if any(op is not None and op[0] == "gamma" for op in flat):
                stats2 = ops_raw.intensity_stats(lib, part, flat, 1, stats)
            if out_of_place:
                got = ops_raw.intensity_apply(lib, part, flat, stats, stats2, masks, out_of_place=True)
                if len(groups) == 1:
                    out = got
                else:
                    out[sb, sc] = got
            else:
                ops_raw.intensity_apply(lib, part, flat, stats, stats2)
        return out, True

    def _noise_ops(self, x, plan):
        """the noise fields come from the device generator, one `randn` per sample that is on, as the parent draws them"""
        B, C = x.shape[:2]
        ops = [[None] * C for _ in range(B)]
        for b in np.nonzero(plan["noise_on"])[0]:
            field = torch.randn(x.shape[1:], device=x.device, generator=self.g, dtype=x.dtype)
            ops[b] = [("noise", float(plan["noise_scale"][b]), field[c]) for c in range(C)]
        return ops

    @staticmethod
    def _contrast_ops(B, C, plan):
        ops = [[None] * C for _ in range(B)]
        for b in range(B):
            bright = [float(m) for m in plan["bright"][b]] if plan["bright_on"][b] else [1.0] * C
            if plan["contrast_on"][b]:
                ops[b] = [("contrast", bright[c], float(plan["contrast"][b][c])) for c in range(C)]
            elif plan["bright_on"][b]:
                ops[b] = [("scale", bright[c]) for c in range(C)]
        return ops

    @staticmethod
    def _gamma_ops(B, C, plan, key, invert):
        return [[("gamma", float(plan[key][b][c]), invert) for c in range(C)] if plan[key + "_on"][b] else [None] * C for b in range(B)]

    def _mirror_masks(self, B, plan):
        return [sum(1 << ax for j, ax in enumerate(self.mirror_axes) if plan["mirror"][b, j]) for b in range(B)]

    def _gammas_and_mirror(self, lib, x, plan, own):
        """the last group: the passes of the gammas that are on, the flips on the last of them"""
        B, C = x.shape[:2]
        rounds = [ops for ops in (self._gamma_ops(B, C, plan, "gamma_inv", True), self._gamma_ops(B, C, plan, "gamma", False))
                  if any(op is not None for row in ops for op in row)]
        masks = self._mirror_masks(B, plan)
        if any(masks) and not rounds:
            rounds = [[[None] * C for _ in range(B)]]
        for i, ops in enumerate(rounds):
            x, own = self._pass(lib, x, ops, own, masks if i == len(rounds) - 1 else None)
        return x, own

    def __call__(self, image: torch.Tensor, label: torch.Tensor):
        """image (B, C, D, H, W) float32, label (B, D, H, W) integer class map -> augmented copies (same shapes / dtypes)"""
        if not L.on_device(image) or not L.on_device(label):
            raise RuntimeError("FusedAugmenter runs on the HIP library's kernels (csrc/augment.hip, csrc/intensity.hip): image and "
                               "label must live on the GPU; on host tensors use DeviceAugmenter (augment=True)")
        if image.dim() != 5 or label.dim() != 4 or image.dtype != torch.float32:
            raise RuntimeError(f"FusedAugmenter: image (B, C, D, H, W) float32 and label (B, D, H, W) are required, got "
                               f"{tuple(image.shape)} {image.dtype} and {tuple(label.shape)}")
        lib = L.get_lib()
        B, C = image.shape[:2]
        plan = self.draw(B, C, tuple(image.shape[2:]))
        x, y = image, label
        if self.spatial:
            x, y = self._spatial(lib, x, y, plan)
        own = x is not image                           # whether x may be written in place
        own_y = y is not label
        x, own = self._pass(lib, x, self._noise_ops(x, plan), own)
        blurred = self._blur(lib, x, plan)
        own, x = own or blurred is not x, blurred
        x, own = self._pass(lib, x, self._contrast_ops(B, C, plan), own)
        x, own = self._low_res(lib, x, plan, own)
        x, own = self._gammas_and_mirror(lib, x, plan, own)
        for b in range(B):
            axes = [ax for j, ax in enumerate(self.mirror_axes) if plan["mirror"][b, j]]
            if axes:
                if not own_y:
                    y, own_y = y.clone(), True
                y[b] = y[b].flip(axes)
        return x.contiguous(), y.contiguous()


def select_augmenter(augment):
    """the class behind a feeder's truthy `augment` argument: "spline" -> SplineAugmenter, "fused" -> FusedAugmenter, anything else
    (True) -> DeviceAugmenter"""
    if isinstance(augment, str) and augment == "fused":
        return FusedAugmenter
    return SplineAugmenter if isinstance(augment, str) and augment == "spline" else DeviceAugmenter
