"""Resampling a case to the target spacing on the device (csrc/resample.hip).

The reference resamples every case in `run_case_npy` (light_training/preprocessing/preprocessors/default_preprocessor.py:187-201)
through resampling/default_resampling.py; the functions here carry its names.  Without a separate z axis - the only branch the
preprocessor takes, `force_separate_z` keeps its default False - that is, per channel,

  data  skimage's `resize(x.astype(float64), new_shape, order, mode='edge', anti_aliasing=False)` with its default clip=True, cast back
        to float32: a cubic B-spline (order 3) or trilinear (order 1) zoom, clipped to the channel's own range;
  seg   batchgenerators' `resize_segmentation(seg, new_shape, 1)`: per label in ascending order the trilinear zoom of its indicator,
        `out[r >= 0.5] = label` on zeros - the largest label whose weight reaches one half, else 0.

Device tensors in, device tensors out; nothing is read back.  Limits and deviations:
  * the separate-z branch (`force_separate_z=True`, or None with a spacing the reference's rule calls anisotropic) raises
    NotImplementedError, as do orders other than 3 or 1 for data and other than 1 for a seg;
  * at most 8 channels per call, every side at most 2048, fewer than 2^31 voxels per channel;
  * sums run in float64 in a fixed order that is not scipy's: values differ from the reference's by rounding (the tests hold them to
    2^-23 |v| + 2^-40 max|x|), and a seg voxel whose weight is within rounding of exactly 0.5 may fall on the other side;
  * a seg comes back as int16 whatever it went in as; non-finite data values are outside the contract."""
from __future__ import annotations

import numpy as np
import torch

from . import lib as L
from . import ops_raw
from .metrics import _to_device

ANISO_THRESHOLD = 3


def compute_new_shape(old_shape, old_spacing, new_spacing):
    """resampling/default_resampling.py:23-30"""
    return [int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)]


def get_do_separate_z(spacing, anisotropy_threshold=ANISO_THRESHOLD) -> bool:
    return bool((np.max(spacing) / np.min(spacing)) > anisotropy_threshold)


def get_lowres_axis(new_spacing):
    return np.where(max(new_spacing) / np.array(new_spacing) == 1)[0]


def _zoom_seg(lib, seg: torch.Tensor, new_shape):
    """(c, D, H, W) integer-valued seg -> ((c,) + new_shape int16, the label counts of its first channel)"""
    if seg.dtype != torch.int16:
        if seg.dtype.is_floating_point or seg.dtype in (torch.int32, torch.int64):
            lo, hi = seg.min(), seg.max()
            if bool((lo < -32768) | (hi > 32767)) or (seg.dtype.is_floating_point and bool((seg != seg.round()).any())):
                raise RuntimeError("resample_data_or_seg: a seg holds integer labels in [-32768, 32767]")
        seg = seg.to(torch.int16)
    outs, counts = [], None
    for c in range(seg.shape[0]):
        o, n = ops_raw.zoom_labels(lib, seg[c].contiguous(), new_shape, want_counts=(c == 0))
        outs.append(o)
        counts = n if c == 0 else counts
    return (outs[0][None] if len(outs) == 1 else torch.stack(outs)), counts


def _resample(data, new_shape, is_seg, order, with_counts=False):
    lib = L.get_lib()
    t = _to_device(data)
    if t.dim() != 4:
        raise RuntimeError(f"resample_data_or_seg: data must be (c, x, y, z), got shape {tuple(t.shape)}")
    new_shape = [int(v) for v in new_shape]
    if len(new_shape) != 3:
        raise RuntimeError(f"resample_data_or_seg: the new shape has three entries, got {new_shape}")
    if is_seg and order != 1:
        raise NotImplementedError(f"resample_data_or_seg: a seg is resized with order 1 only, got order {order}")
    if not is_seg and order not in (1, 3):
        raise NotImplementedError(f"resample_data_or_seg: data are resized with order 3 or 1, got order {order}")
    if list(t.shape[1:]) == new_shape:
        return (t, None) if with_counts else t
    if is_seg:
        out, counts = _zoom_seg(lib, t, new_shape)
        return (out, counts) if with_counts else out
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    parts = [ops_raw.zoom(lib, t[c0:c0 + L.PREP_MAX_CHANNELS], new_shape, order, True) for c0 in range(0, t.shape[0], L.PREP_MAX_CHANNELS)]
    out = parts[0] if len(parts) == 1 else torch.cat(parts)
    return (out, None) if with_counts else out


def resample_data_or_seg(data, new_shape, is_seg: bool = False, axis=None, order: int = 3, do_separate_z: bool = False, order_z: int = 0):
    """default_resampling.py:126-217 without its separate-z branch.  data (c, D, H, W) -> (c,) + new_shape on the device: float32
    for data, int16 for a seg; the input itself when the shapes are equal."""
    if do_separate_z:
        raise NotImplementedError("resample_data_or_seg: resampling the out-of-plane axis separately (do_separate_z) is not part of "
                                  "this module; the reference's preprocessor never asks for it")
    return _resample(data, new_shape, is_seg, order)


def resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, is_seg: bool = False, order: int = 3, order_z: int = 0,
                                  force_separate_z=False, separate_z_anisotropy_threshold: float = ANISO_THRESHOLD):
    """default_resampling.py:78-123: decides on the separate z axis as the reference does, then `resample_data_or_seg`"""
    if force_separate_z is not None:
        do_separate_z = bool(force_separate_z)
        axis = get_lowres_axis(current_spacing) if force_separate_z else None
    elif get_do_separate_z(current_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(current_spacing)
    elif get_do_separate_z(new_spacing, separate_z_anisotropy_threshold):
        do_separate_z, axis = True, get_lowres_axis(new_spacing)
    else:
        do_separate_z, axis = False, None
    if axis is not None and len(axis) in (2, 3):
        do_separate_z = False
    return resample_data_or_seg(data, new_shape, is_seg, axis, order, do_separate_z, order_z=order_z)
