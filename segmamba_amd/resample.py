"""Resampling a case to the target spacing on the device (csrc/resample.hip).

The reference resamples every case in `run_case_npy` (light_training/preprocessing/preprocessors/default_preprocessor.py:187-201)
through resampling/default_resampling.py; the functions here carry its names.  Without a separate z axis - the branch the
preprocessor takes, `force_separate_z` keeps its default False - that is, per channel,

  data  skimage's `resize(x.astype(float64), new_shape, order, mode='edge', anti_aliasing=False)` with its default clip=True, cast back
        to float32: a cubic B-spline (order 3) or trilinear (order 1) zoom, clipped to the channel's own range;
  seg   batchgenerators' `resize_segmentation(seg, new_shape, 1)`: per label in ascending order the trilinear zoom of its indicator,
        `out[r >= 0.5] = label` on zeros - the largest label whose weight reaches one half, else 0.

With a separate z axis (default_resampling.py:154-207: `do_separate_z=True`, `force_separate_z=True`, or `force_separate_z=None` on a
spacing whose max / min exceeds 3 with ONE coarsest axis) every 2-D slice across the coarse axis goes through the same two functions
on its own - so the clip is to the slice's range - and the coarse axis takes the nearest slice (`map_coordinates(order=0,
mode='nearest')`: slice `slice_table(n_in, n_out)[k]`).  The branch is opt-in: `allow_separate_z=True`.

Device tensors in, device tensors out; nothing is read back.  Limits and deviations:
  * without `allow_separate_z=True` the separate-z branch raises NotImplementedError, as do orders other than 3 or 1 for data and
    other than 1 for a seg; within the branch `order_z` other than 0 raises NotImplementedError (no caller of the reference passes one,
    and order 3 along z needs a prefilter pass of its own: out of scope);
  * in the branch, slices whose in-plane shape does not change are copied as they are (the reference's factor-1 resize reproduces
    them only up to float64 rounding); axis 0 goes to the kernels as it is, axis 1 as a permuted view with one copy to bring the
    result back to the caller's order, axis 2 through one transposed copy in and one out;
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


def slice_table(n_in: int, n_out: int) -> np.ndarray:
    """int32 (n_out,): the input slice that `map_coordinates(order=0, mode='nearest')` reads for output slice k at the coordinate
    (n_in / n_out) * (k + 0.5) - 0.5 (default_resampling.py:179-194): floor(coordinate + 0.5) clipped to the axis, in float64 with
    every operation rounded on its own - numpy on the host, so no fused multiply-add can move an index"""
    scale = float(n_in) / n_out
    k = np.arange(n_out, dtype=np.float64)
    return np.clip(np.floor(scale * (k + 0.5) - 0.5 + 0.5), 0, n_in - 1).astype(np.int32)


def _seg_int16(seg: torch.Tensor) -> torch.Tensor:
    if seg.dtype != torch.int16:
        if seg.dtype.is_floating_point or seg.dtype in (torch.int32, torch.int64):
            lo, hi = seg.min(), seg.max()
            if bool((lo < -32768) | (hi > 32767)) or (seg.dtype.is_floating_point and bool((seg != seg.round()).any())):
                raise RuntimeError("resample_data_or_seg: a seg holds integer labels in [-32768, 32767]")
        seg = seg.to(torch.int16)
    return seg


def _zoom_seg(lib, seg: torch.Tensor, new_shape):
    """(c, D, H, W) integer-valued seg -> ((c,) + new_shape int16, the label counts of its first channel)"""
    seg = _seg_int16(seg)
    outs, counts = [], None
    for c in range(seg.shape[0]):
        o, n = ops_raw.zoom_labels(lib, seg[c].contiguous(), new_shape, want_counts=(c == 0))
        outs.append(o)
        counts = n if c == 0 else counts
    return (outs[0][None] if len(outs) == 1 else torch.stack(outs)), counts


# the slice axis outermost, x (or, for axis 2, y) innermost: the permutation in, and the one that undoes it
_SLICES_FIRST = {0: ((0, 1, 2, 3), (0, 1, 2, 3)), 1: ((0, 2, 1, 3), (0, 2, 1, 3)), 2: ((0, 3, 1, 2), (0, 2, 3, 1))}


def _zoom_separate_z(lib, t: torch.Tensor, new_shape, is_seg: bool, axis: int, order: int):
    """(c, n0, n1, n2) float32 data or integer-valued seg on the device -> ((c,) + new_shape, the label counts of a seg's first
    channel or None).  Axis 0 goes to the kernels as it is; axis 1 as a permuted view, which keeps x at a unit stride (a seg, which
    the kernel takes contiguous, is copied); axis 2 through one transposed copy in and one out."""
    fwd, back = _SLICES_FIRST[axis]
    shape = [new_shape[i - 1] for i in fwd[1:]]
    source = torch.from_numpy(slice_table(int(t.shape[1 + axis]), new_shape[axis])).to(t.device)
    v = t.permute(*fwd)
    if is_seg:
        v = _seg_int16(v)
        outs, counts = [], None
        for c in range(v.shape[0]):
            o, n = ops_raw.zoom_labels_slices(lib, v[c].contiguous(), shape, source, want_counts=(c == 0))
            outs.append(o)
            counts = n if c == 0 else counts
        out = outs[0][None] if len(outs) == 1 else torch.stack(outs)
    else:
        if v.dtype != torch.float32:
            v = v.to(torch.float32)
        if v.shape[-1] > 1 and v.stride(-1) != 1:
            v = v.contiguous()
        parts = [ops_raw.zoom_slices(lib, v[c0:c0 + L.PREP_MAX_CHANNELS], shape, source, order, True)
                 for c0 in range(0, v.shape[0], L.PREP_MAX_CHANNELS)]
        out, counts = (parts[0] if len(parts) == 1 else torch.cat(parts)), None
    return (out if axis == 0 else out.permute(*back).contiguous()), counts


def _resample(data, new_shape, is_seg, order, with_counts=False, separate_axis=None):
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
    if separate_axis is not None:
        out, counts = _zoom_separate_z(lib, t, new_shape, is_seg, separate_axis, order)
        return (out, counts) if with_counts else out
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


def _separate_axis(axis, order_z: int) -> int:
    """the one slice axis of the separate-z branch, as default_resampling.py:156-157 asserts it"""
    axis = [] if axis is None else [int(a) for a in np.atleast_1d(axis)]
    if len(axis) != 1 or axis[0] not in (0, 1, 2):
        raise RuntimeError(f"resample_data_or_seg: only one anisotropic axis is supported, got axis {axis}")
    if order_z != 0:
        raise NotImplementedError(f"resample_data_or_seg: along the separate axis only order_z=0 (the nearest slice) is implemented, got {order_z}")
    return axis[0]


def resample_data_or_seg(data, new_shape, is_seg: bool = False, axis=None, order: int = 3, do_separate_z: bool = False, order_z: int = 0,
                         allow_separate_z: bool = False):
    """default_resampling.py:126-217.  data (c, D, H, W) -> (c,) + new_shape on the device: float32 for data, int16 for a seg; the
    input itself when the shapes are equal.  `do_separate_z` with the one-entry `axis` takes the reference's separate-z branch
    (:154-207) when `allow_separate_z=True` is given and raises NotImplementedError otherwise."""
    if do_separate_z:
        if not allow_separate_z:
            raise NotImplementedError("resample_data_or_seg: resampling the out-of-plane axis separately (do_separate_z) runs only "
                                      "with allow_separate_z=True; the reference's preprocessor never asks for it")
        return _resample(data, new_shape, is_seg, order, separate_axis=_separate_axis(axis, order_z))
    return _resample(data, new_shape, is_seg, order)


def decide_separate_z(current_spacing, new_spacing, force_separate_z=False, separate_z_anisotropy_threshold: float = ANISO_THRESHOLD):
    """default_resampling.py:40-66 / :91-117 -> (do_separate_z, axis): forced, or - with None - by the current spacing first, then the
    target's; two or three equally coarse axes decide against"""
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
    return do_separate_z, axis


def resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, is_seg: bool = False, order: int = 3, order_z: int = 0,
                                  force_separate_z=False, separate_z_anisotropy_threshold: float = ANISO_THRESHOLD,
                                  allow_separate_z: bool = False):
    """default_resampling.py:78-123: decides on the separate z axis as the reference does, then `resample_data_or_seg`"""
    do_separate_z, axis = decide_separate_z(current_spacing, new_spacing, force_separate_z, separate_z_anisotropy_threshold)
    return resample_data_or_seg(data, new_shape, is_seg, axis, order, do_separate_z, order_z=order_z, allow_separate_z=allow_separate_z)


def resample_data_or_seg_to_spacing(data, current_spacing, new_spacing, is_seg: bool = False, order: int = 3, order_z: int = 0,
                                    force_separate_z=False, separate_z_anisotropy_threshold: float = ANISO_THRESHOLD,
                                    allow_separate_z: bool = False):
    """default_resampling.py:33-75: the new shape is `compute_new_shape` of the data's own, then as `resample_data_or_seg_to_shape`"""
    shape = getattr(data, "shape", ())
    if len(shape) != 4:
        raise RuntimeError(f"resample_data_or_seg_to_spacing: data must be (c, x, y, z), got shape {tuple(shape)}")
    new_shape = compute_new_shape(shape[1:], current_spacing, new_spacing)
    return resample_data_or_seg_to_shape(data, new_shape, current_spacing, new_spacing, is_seg, order, order_z, force_separate_z,
                                         separate_z_anisotropy_threshold, allow_separate_z)
