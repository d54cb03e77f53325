"""Preparing a case on the device: non-zero crop, z-score normalisation, resampling, class locations (csrc/preprocess.hip, csrc/resample.hip).

The stage of the reference's pipeline in front of training (2_preprocessing_mri.py on light_training/preprocessing):
`MultiModalityPreprocessor.run_case_npy` (preprocessors/default_preprocessor.py:154-227 through preprocessor_mri.py) - the non-zero
mask over the channels, its holes filled, the bounding box, the crop of data and seg with `seg[(seg == 0) & ~mask] = -1`, the
per-channel z-score, the resampling to the target spacing (`resample=True`; segmamba_amd/resample.py), the class locations that
the patch sampler draws foreground from, and the `properties` that
`postprocess.labels_from_logits` and `Predictor.predict_labels` take back.  The functions carry the reference's names.  Tensors stay
on the device; numpy arrays and host tensors are uploaded.  A case costs two scalars-only readbacks before its class locations are
drawn - the box (6 ints) and the label counts (260 ints); nothing volume-sized goes back to the host except what is written to disk.

Limits and where this deliberately differs from the reference:
  * resampling is opt-in: by default a case whose `compute_new_shape` differs from its crop shape raises NotImplementedError (every
    BraTS case is 1 mm in, [1, 1, 1] out: the reference returns it unchanged).  With `resample=True` the normalised crop goes through
    the order-3 spline zoom and the relabelled seg through the order-1 label rule, as the reference's `run_case_npy` does; the
    limits and the rounding-level deviations of that step are stated in segmamba_amd/resample.py;
  * an all-zero volume raises RuntimeError (the reference fails inside `get_bbox_from_mask`);
  * `intensities_per_channel` and `intensity_statistics_per_channel` are not produced (the reference comments that it does not use
    them; the z-score never reads them);
  * mean and std are accumulated in fp64 in a fixed order and then rounded to fp32 (the reference lets numpy accumulate in fp32);
    the normalisation itself is the reference's fp32 arithmetic;
  * a seg value that is no integer in [-1, 32767] raises RuntimeError instead of becoming some label;
  * files are read with `nifti.read_nifti`: types it refuses stay refused; cases are processed one after the other, no process pool.
"""
from __future__ import annotations

import math
import os
import pickle
from typing import Optional, Sequence

import numpy as np
import torch

from . import lib as L
from . import ops_raw
from .metrics import _to_device
from .postprocess import _fill
from .resample import compute_new_shape            # noqa: F401  (resampling/default_resampling.py:23-30)

NUM_SAMPLES = 10000                   # _sample_foreground_locations (default_preprocessor.py:456-457)
MIN_PERCENT_COVERAGE = 0.01


def _data(x, what: str) -> torch.Tensor:
    """(C, D, H, W) fp32 on the device with a unit stride along x"""
    t = _to_device(x)
    if t.dim() != 4:
        raise RuntimeError(f"{what}: data (C, D, H, W) are required, got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.shape[-1] > 1 and t.stride(-1) != 1:
        t = t.contiguous()
    return t


def _seg(x, shape, what: str) -> Optional[torch.Tensor]:
    """(1, D, H, W) or (D, H, W) -> (D, H, W) float32 / uint8 / int16, contiguous, on the device"""
    if x is None:
        return None
    t = _to_device(x)
    if t.dim() == 4 and t.shape[0] == 1:
        t = t[0]
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: the seg must have the data's volume shape {tuple(shape)}, got {tuple(t.shape)}")
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    elif t.dtype == torch.int8:
        t = t.to(torch.int16)
    elif t.dtype not in (torch.float32, torch.uint8, torch.int16):
        t = t.to(torch.float32)                       # exact for every label the kernels accept; larger values are refused there
    return t.contiguous()


def _box(lib, data: torch.Tensor):
    """(filled mask, [[z0, z1], [y0, y1], [x0, x1]]): the first readback of a case"""
    mask, bbox = ops_raw.nonzero_mask_bbox(lib, data)
    filled = _fill(lib, mask)                         # queued before the readback: the box does not wait for it
    z0, y0, x0, z1, y1, x1 = (int(v) for v in bbox.tolist())
    if z1 == 0:
        raise RuntimeError("crop_to_nonzero: the volume is zero everywhere, there is nothing to crop to")
    return filled, [[z0, z1], [y0, y1], [x0, x1]]


def _check_counts(counts: torch.Tensor):
    """the second readback of a case: the label counts -> (list of 260 ints, the largest label or -1)"""
    c = [int(v) for v in counts.tolist()]
    if c[L.PREP_BIN_INVALID]:
        raise RuntimeError(f"the seg holds {c[L.PREP_BIN_INVALID]} voxels whose value is no integer in [-1, 32767]")
    top = 256 if c[L.PREP_BIN_ABOVE] else max([l for l in range(256) if c[l]], default=-1)
    return c, top


def _seg_out(seg_out: torch.Tensor, top: int) -> torch.Tensor:
    """(1, d, h, w), int16 if the largest label is above 127, else int8 (default_preprocessor.py:207-210)"""
    return (seg_out if top > 127 else seg_out.to(torch.int8))[None]


def create_nonzero_mask(data) -> torch.Tensor:
    """cropping.py:8-21: uint8 (D, H, W), 1 where any channel of data (C, D, H, W) is != 0, the holes filled"""
    lib = L.get_lib()
    return _fill(lib, ops_raw.nonzero_mask_bbox(lib, _data(data, "create_nonzero_mask"))[0])


def crop_to_nonzero(data, seg=None, nonzero_label: int = -1):
    """cropping.py:24-49.  -> (data (C, d, h, w) fp32, seg (1, d, h, w), bbox [[z0, z1], [y0, y1], [x0, x1]]).  The seg comes back as
    int16 (int8 when it was built from the mask because none was given), 0 outside the filled mask replaced by `nonzero_label`."""
    lib = L.get_lib()
    d = _data(data, "crop_to_nonzero")
    s = _seg(seg, d.shape[1:], "crop_to_nonzero")
    filled, bbox = _box(lib, d)
    identity = torch.cat([torch.zeros(8), torch.ones(8)]).to(d.device)          # (x - 0) / 1 = x, exactly
    out, seg_out, counts = ops_raw.crop_normalize(lib, d, identity, [b[0] for b in bbox], [b[1] - b[0] for b in bbox], mask=filled, seg=s,
                                                  nonzero_label=nonzero_label)
    _check_counts(counts)
    return out, (seg_out.to(torch.int8) if s is None else seg_out)[None], bbox


def zscore_normalize(data, seg=None, use_mask_for_norm: bool = False) -> torch.Tensor:
    """ZScoreNormalization.run per channel (default_normalization_schemes.py:31-50): (x - mean) / max(std, 1e-8), fp32, the
    statistics over the whole volume; with `use_mask_for_norm` over `seg >= 0` only, every other voxel left as it is."""
    lib = L.get_lib()
    d = _data(data, "zscore_normalize")
    mask = None
    if use_mask_for_norm:
        if seg is None:
            raise RuntimeError("zscore_normalize: use_mask_for_norm needs the seg")
        s = _to_device(seg)
        s = s[0] if s.dim() == 4 and s.shape[0] == 1 else s
        if tuple(s.shape) != tuple(d.shape[1:]):
            raise RuntimeError(f"zscore_normalize: the seg must have the data's volume shape {tuple(d.shape[1:])}, got {tuple(s.shape)}")
        mask = (s >= 0).to(torch.uint8).contiguous()
    _, stats32 = ops_raw.crop_stats(lib, d, mask=mask, masked=use_mask_for_norm)
    return ops_raw.crop_normalize(lib, d, stats32, mask=mask, masked=use_mask_for_norm, want_seg=False)[0]


def sample_foreground_locations(seg, classes_or_regions, seed: int = 1234, counts: Optional[Sequence[int]] = None) -> dict:
    """`_sample_foreground_locations` (default_preprocessor.py:453-482): per class (an int) or region (a tuple / list of labels)
    max(min(10000, n), ceil(0.01 n)) of its n voxels, drawn without replacement by ONE np.random.RandomState(seed) called once per
    non-empty class in order - the reference's calls, so the rows are the reference's.  The voxel list comes from torch.nonzero on the
    device (np.argwhere's order: four columns for the (1, d, h, w) seg); only the drawn rows go to the host.  -> {class: int64 (n, 4)
    array, or [] for an empty class}.  `counts` (label -> voxels, as `preprocess_case` has them) spares the search for empty classes."""
    t = _to_device(seg)
    if t.dim() == 3:
        t = t[None]
    if t.dim() != 4:
        raise RuntimeError(f"sample_foreground_locations: a (1, d, h, w) or (d, h, w) seg is required, got shape {tuple(t.shape)}")
    rndst = np.random.RandomState(seed)
    class_locs = {}
    for c in classes_or_regions:
        k = tuple(c) if isinstance(c, list) else c
        labels = list(c) if isinstance(c, (tuple, list)) else [c]
        if counts is not None and all(0 <= int(l) < 256 and counts[int(l)] == 0 for l in labels):
            class_locs[k] = []
            continue
        m = t == labels[0]
        for l in labels[1:]:
            m = m | (t == l)
        all_locs = torch.nonzero(m)
        n = int(all_locs.shape[0])
        if n == 0:
            class_locs[k] = []
            continue
        target = max(min(NUM_SAMPLES, n), int(math.ceil(n * MIN_PERCENT_COVERAGE)))
        chosen = rndst.choice(n, target, replace=False)
        class_locs[k] = all_locs[torch.from_numpy(chosen).to(all_locs.device)].cpu().numpy().astype(np.int64)
    return class_locs


def preprocess_case(data, seg, properties: dict, out_spacing=(1, 1, 1), all_labels=(1, 2, 3), use_mask_for_norm: bool = False,
                    resample: bool = False):
    """`run_case_npy` (default_preprocessor.py:154-227).  data (C, D, H, W); seg (1, D, H, W) / (D, H, W) or None; properties with
    `spacing` (SimpleITK's (x, y, z)).  -> (data (C, d, h, w) fp32, seg (1, d, h, w) int8 / int16) on the device; `properties` gains
    original_spacing_trans, target_spacing_trans, shape_before_cropping, bbox_used_for_cropping, shape_after_cropping_before_resample,
    shape_after_resample (plain ints, floats and lists) and class_locations (`sample_foreground_locations`).  With `resample` a crop
    whose `compute_new_shape` differs from its shape is resampled to it (data order 3, seg order 1: default_preprocessor.py:187-201);
    the class locations and the seg's dtype then come from the resampled seg.  Without it such a case raises NotImplementedError."""
    lib = L.get_lib()
    d = _data(data, "preprocess_case")
    s = _seg(seg, d.shape[1:], "preprocess_case")
    spacing_trans = [float(v) for v in list(properties["spacing"])[::-1]]
    target = [float(v) if float(v) != int(v) else int(v) for v in out_spacing]
    filled, bbox = _box(lib, d)
    crop_shape = [b[1] - b[0] for b in bbox]
    new_shape = compute_new_shape(crop_shape, spacing_trans, target)
    if new_shape != crop_shape and not resample:
        raise NotImplementedError(f"preprocess_case: the crop of shape {crop_shape} would be resampled to {new_shape} (spacing "
                                  f"{spacing_trans} -> {target}); spline resampling is not part of this module unless resample=True is given")
    start = [b[0] for b in bbox]
    _, stats32 = ops_raw.crop_stats(lib, d, start, crop_shape, mask=filled, seg=s, masked=use_mask_for_norm)
    out, seg_out, counts = ops_raw.crop_normalize(lib, d, stats32, start, crop_shape, mask=filled, seg=s, masked=use_mask_for_norm)
    if new_shape != crop_shape:
        # an invalid seg value was written as label 0 and would be lost in the zoom: the first counts flag it (on the device)
        invalid = counts[L.PREP_BIN_INVALID]
        out = ops_raw.zoom(lib, out, new_shape, 3, True)
        seg_out, counts = ops_raw.zoom_labels(lib, seg_out, new_shape)
        counts[L.PREP_BIN_INVALID] = invalid
    c, top = _check_counts(counts)
    properties["original_spacing_trans"] = spacing_trans
    properties["target_spacing_trans"] = target
    properties["shape_before_cropping"] = [int(v) for v in d.shape[1:]]
    properties["bbox_used_for_cropping"] = bbox
    properties["shape_after_cropping_before_resample"] = crop_shape
    properties["shape_after_resample"] = new_shape
    properties["class_locations"] = sample_foreground_locations(seg_out, all_labels, counts=c if top < 256 else None)
    return out, _seg_out(seg_out, top)


class CasePreprocessor:
    """`MultiModalityPreprocessor` (preprocessors/preprocessor_mri.py:32-134): a directory `base_dir/image_dir/<case>/` per case with
    one NIfTI file per modality (`data_filenames`) and optionally the seg (`seg_filename`).  `run` writes the reference's
    `<case>.npz` (data, seg) and `<case>.pkl` (properties) into `output_dir`, one case after the other."""

    def __init__(self, base_dir, image_dir, data_filenames: Sequence[str] = (), seg_filename: str = "", use_mask_for_norm: bool = False,
                 resample: bool = False):
        self.base_dir, self.image_dir = str(base_dir), str(image_dir)
        self.data_filenames, self.seg_filename = list(data_filenames), seg_filename
        self.use_mask_for_norm, self.resample = use_mask_for_norm, resample
        self.out_spacing, self.all_labels, self.output_dir = (1, 1, 1), (1, 2, 3), None

    def get_iterable_list(self):
        return sorted(os.listdir(os.path.join(self.base_dir, self.image_dir)))

    def read_data(self, case_name):
        from .nifti import read_nifti
        if not self.data_filenames:
            raise RuntimeError("CasePreprocessor: data_filenames is empty")
        folder = os.path.join(self.base_dir, self.image_dir, case_name)
        data, spacing = [], None
        for name in self.data_filenames:
            arr, spacing = read_nifti(os.path.join(folder, name))
            data.append(arr.astype(np.float32)[None])
        data = np.concatenate(data, axis=0)
        seg = None
        if self.seg_filename != "":
            seg = read_nifti(os.path.join(folder, self.seg_filename))[0].astype(np.float32)[None]
        properties = {"spacing": tuple(float(v) for v in spacing), "raw_size": tuple(int(v) for v in data.shape[1:]),
                      "name": case_name.split(".")[0]}
        return data, seg, properties

    def run_case(self, case_name):
        data, seg, properties = self.read_data(case_name)
        data, seg = preprocess_case(data, seg, properties, self.out_spacing, self.all_labels, self.use_mask_for_norm, self.resample)
        return data, seg, properties

    def run_case_save(self, case_name):
        data, seg, properties = self.run_case(case_name)
        stem = os.path.join(self.output_dir, case_name.split(".")[0])
        np.savez_compressed(stem + ".npz", data=data.cpu().numpy(), seg=seg.cpu().numpy())
        with open(stem + ".pkl", "wb") as f:
            pickle.dump(properties, f)
        return stem + ".npz"

    def run(self, output_spacing=(1, 1, 1), output_dir=None, all_labels=(1, 2, 3)):
        if output_dir is None:
            raise RuntimeError("CasePreprocessor.run: output_dir is required")
        self.out_spacing, self.all_labels, self.output_dir = output_spacing, all_labels, str(output_dir)
        os.makedirs(self.output_dir, exist_ok=True)
        return [self.run_case_save(case) for case in self.get_iterable_list()]
