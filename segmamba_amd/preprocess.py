"""Preparing a case on the device: non-zero crop, z-score or CT normalisation, the intensity fingerprint, resampling, class locations
(csrc/preprocess.hip, csrc/fingerprint.hip, csrc/resample.hip).

The stage of the reference's pipeline in front of training (2_preprocessing_mri.py on light_training/preprocessing):
`MultiModalityPreprocessor.run_case_npy` (preprocessors/default_preprocessor.py:154-227 through preprocessor_mri.py) - the non-zero
mask over the channels, its holes filled, the bounding box, the crop of data and seg with `seg[(seg == 0) & ~mask] = -1`, the
per-channel z-score, the resampling to the target spacing (`resample=True`; segmamba_amd/resample.py), the class locations that
the patch sampler draws foreground from, and the `properties` that
`postprocess.labels_from_logits` and `Predictor.predict_labels` take back.  The functions carry the reference's names.  Tensors stay
on the device; numpy arrays and host tensors are uploaded.  A case costs two scalars-only readbacks before its class locations are
drawn - the box (6 ints) and the label counts (260 ints); nothing volume-sized goes back to the host except what is written to disk.

CT cases go the way of the reference's `DefaultPreprocessor` (default_preprocessor.py:137-451, through 2_preprocessing_*.py of its CT
examples): `collect_foreground_intensities` is the per-case fingerprint (:413-451), `CTCasePreprocessor.run_plan` the dataset's
(:347-410), `ct_normalize` is `CTNormalization.run` (default_normalization_schemes.py:83-95) and `preprocess_case(normalization="ct")`
the reference's order: crop, CT normalisation, resampling, class locations.  The fingerprint costs two scalars-only readbacks of its
own: the foreground count n, then the order statistics, the sums and the C x num_samples samples.  With n == 0 nothing is launched
after the first.  Two calls give equal bits.

Limits and where this deliberately differs from the reference:
  * resampling is opt-in: by default a case whose `compute_new_shape` differs from its crop shape raises NotImplementedError (every
    BraTS case is 1 mm in, [1, 1, 1] out: the reference returns it unchanged).  With `resample=True` the normalised crop goes through
    the order-3 spline zoom and the relabelled seg through the order-1 label rule, as the reference's `run_case_npy` does; the
    limits and the rounding-level deviations of that step are stated in segmamba_amd/resample.py;
  * an all-zero volume raises RuntimeError (the reference fails inside `get_bbox_from_mask`);
  * `intensities_per_channel` and `intensity_statistics_per_channel` are produced by `collect_foreground_intensities` /
    `CTCasePreprocessor`; the MRI `CasePreprocessor` still omits them (the z-score never reads them);
  * the fingerprint's percentiles are `a + (b - a) * g` in float64 on the two exact order statistics around the virtual index
    (n - 1) q / 100, rounded once to float32.  numpy's np.percentile on a float32 array depends on the numpy version (2.2 takes the
    fraction g in float32, which moves the result by up to tens of fp32 ulps of |a| + |b|); the contract here is the float64 rule.
    The fingerprint's mean is the fp64 sum in a fixed order divided by n, rounded to float32 (numpy sums float32 pairwise).  min, max,
    median and the samples are numpy's, bit for bit;
  * `run_plan` leaves out the key `target medium patch size`: it comes from `get_pool_and_conv_props` (:59-134), nnU-Net's network
    planning, which is not case preparation;
  * the fingerprint takes up to 8 channels of fewer than 2^31 voxels; its workspace is 0.5 MB for one channel of 400 x 512 x 512;
  * mean and std are accumulated in fp64 in a fixed order and then rounded to fp32 (the reference lets numpy accumulate in fp32);
    the normalisation itself is the reference's fp32 arithmetic;
  * a seg value that is no integer in [-1, 32767] raises RuntimeError instead of becoming some label;
  * files are read with `nifti.read_nifti`: types it refuses stay refused; cases are processed one after the other, no process pool.
"""
from __future__ import annotations

import json
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
from . import resample as RS
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


def _fingerprint_ranks(n: int):
    """the 8 ranks one `fg_order_stats` call takes for a channel of n values: min, max, np.median's one or two middle ranks, and
    floor(h), min(floor(h) + 1, n - 1) of the virtual index h = (n - 1) * (q / 100) for q = 0.5 and 99.5 -> (ranks, [g_00_5, g_99_5])"""
    ranks, fracs = [0, n - 1, (n - 1) // 2, n // 2], []
    for q in (0.5, 99.5):
        h = (n - 1) * (q / 100.0)
        lo = int(math.floor(h))
        ranks += [lo, min(lo + 1, n - 1)]
        fracs.append(h - lo)
    return ranks, fracs


def collect_foreground_intensities(segmentation, images, seed: int = 1234, num_samples: int = 10000):
    """`DefaultPreprocessor.collect_foreground_intensities` (default_preprocessor.py:413-451).  segmentation (1, D, H, W) / (D, H, W),
    images (C, D, H, W), C <= 8.  The foreground is `segmentation[0] > 0`, n voxels.  -> (intensities_per_channel: per channel the
    float32 array `rs.choice(images[c][mask], num_samples, replace=True)` from ONE np.random.RandomState(seed) - the reference's draws,
    bit for bit - or [] when n == 0; intensity_statistics_per_channel: per channel a dict mean, median, min, max, percentile_99_5,
    percentile_00_5 as np.float32, NaN when n == 0).  The n-long compaction is never written: `segm_fg_gather` reads the drawn ranks,
    `segm_fg_order_stats` selects the 8 order statistics behind min, max, median and the percentiles in three passes.  Two scalars-only
    readbacks: n, then the results.  The percentile rule and the mean's accumulation differ from numpy's float32 forms as the module
    docstring states."""
    lib = L.get_lib()
    d = _data(images, "collect_foreground_intensities")
    s = _seg(segmentation, d.shape[1:], "collect_foreground_intensities")
    if s is None:
        raise RuntimeError("collect_foreground_intensities: the segmentation is required")
    num_samples = int(num_samples)
    if num_samples < 1:
        raise RuntimeError(f"collect_foreground_intensities: num_samples must be positive, got {num_samples}")
    channels = int(d.shape[0])
    count, sums, state = ops_raw.fg_count(lib, d, s)
    n = int(count.item())                             # the first readback
    if n == 0:
        keys = ("mean", "median", "min", "max", "percentile_99_5", "percentile_00_5")
        return [[] for _ in range(channels)], [{k: np.nan for k in keys} for _ in range(channels)]
    rs = np.random.RandomState(seed)
    # rs.choice(a, size, replace=True) is a[rs.randint(0, len(a), size)] from the same state (numpy's legacy generator)
    idx = np.stack([rs.randint(0, n, num_samples) for _ in range(channels)]).astype(np.int64)
    ranks, fracs = _fingerprint_ranks(n)
    order = ops_raw.fg_order_stats(lib, state, n, ranks)
    samples = ops_raw.fg_gather(lib, state, n, idx)
    nr = len(ranks)
    back = torch.cat([order.reshape(-1), sums[:channels].view(torch.float32), samples.reshape(-1)]).cpu().numpy()      # the second readback
    order_h = back[:channels * nr].reshape(channels, nr)
    sums_h = back[channels * nr:channels * (nr + 2)].copy().view(np.float64)
    samples_h = back[channels * (nr + 2):].reshape(channels, num_samples)
    intensities, statistics = [], []
    for c in range(channels):
        o = order_h[c]

        def lerp(a, b, g):
            return np.float32(float(a) + (float(b) - float(a)) * g)
        statistics.append({
            "mean": np.float32(sums_h[c] / n),
            "median": o[2] if n % 2 else np.mean(np.array([o[2], o[3]], dtype=np.float32)),
            "min": o[0],
            "max": o[1],
            "percentile_99_5": lerp(o[6], o[7], fracs[1]),
            "percentile_00_5": lerp(o[4], o[5], fracs[0]),
        })
        intensities.append(samples_h[c].copy())
    return intensities, statistics


def _channel_properties(props, c: int) -> dict:
    if isinstance(props, dict):
        if str(c) in props:
            return props[str(c)]
        if c in props:
            return props[c]
        raise RuntimeError(f"intensity properties: no entry for channel {c} (keys {sorted(props, key=str)})")
    if c >= len(props):
        raise RuntimeError(f"intensity properties: {len(props)} entries for channel {c}")
    return props[c]


def _ct_stats(props, channels: int, device) -> torch.Tensor:
    """float32 (32,) on the device for `crop_clip_normalize`: mean, std, percentile_00_5, percentile_99_5 per channel"""
    st = np.zeros(32, dtype=np.float32)
    st[8:16] = 1.0
    for c in range(channels):
        p = _channel_properties(props, c)
        for k, key in enumerate(("mean", "std", "percentile_00_5", "percentile_99_5")):
            if key not in p:
                raise RuntimeError(f"intensity properties of channel {c}: {key!r} is missing")
            st[8 * k + c] = np.float32(p[key])
    return torch.from_numpy(st).to(device)


def ct_normalize(data, intensityproperties) -> torch.Tensor:
    """CTNormalization.run per channel (default_normalization_schemes.py:83-95) on the whole volume: clip to [percentile_00_5,
    percentile_99_5], subtract mean, divide by max(std, 1e-8), all in fp32.  `intensityproperties`: a list, or a dict keyed str(c)
    or c, of per-channel dicts with mean, std, percentile_00_5, percentile_99_5."""
    lib = L.get_lib()
    d = _data(data, "ct_normalize")
    stats32 = _ct_stats(intensityproperties, int(d.shape[0]), d.device)
    return ops_raw.crop_clip_normalize(lib, d, stats32, want_seg=False)[0]


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
                    resample: bool = False, normalization: str = "zscore", foreground_intensity_properties_per_channel=None,
                    force_separate_z=False):
    """`run_case_npy` (default_preprocessor.py:154-227).  data (C, D, H, W); seg (1, D, H, W) / (D, H, W) or None; properties with
    `spacing` (SimpleITK's (x, y, z)).  -> (data (C, d, h, w) fp32, seg (1, d, h, w) int8 / int16) on the device; `properties` gains
    original_spacing_trans, target_spacing_trans, shape_before_cropping, bbox_used_for_cropping, shape_after_cropping_before_resample,
    shape_after_resample (plain ints, floats and lists) and class_locations (`sample_foreground_locations`).  With `resample` a crop
    whose `compute_new_shape` differs from its shape is resampled to it (data order 3, seg order 1: default_preprocessor.py:187-201);
    the class locations and the seg's dtype then come from the resampled seg.  Without it such a case raises NotImplementedError.
    `force_separate_z` (False / None / True, with `resample`) is the reference's: True, or None on a spacing - the case's first, then
    the target's - whose max / min exceeds 3 with one coarsest axis, resamples data and seg slice by slice across that axis and
    takes the nearest slice along it (segmamba_amd/resample.py); the default False keeps the one 3-D zoom.
    `normalization="ct"` replaces the z-score by `CTNormalization` with the dataset's `foreground_intensity_properties_per_channel`
    (per channel mean, std, percentile_00_5, percentile_99_5; keys str(c) as in the reference, or ints): DefaultPreprocessor's
    `run_case_npy` (:154-227, `_normalize` :235-242)."""
    lib = L.get_lib()
    if normalization not in ("zscore", "ct"):
        raise RuntimeError(f'preprocess_case: normalization is "zscore" or "ct", got {normalization!r}')
    if normalization == "ct":
        if foreground_intensity_properties_per_channel is None:
            raise RuntimeError('preprocess_case: normalization="ct" needs foreground_intensity_properties_per_channel')
        if use_mask_for_norm:
            raise RuntimeError("preprocess_case: the CT normalisation has no masked form (the reference runs it with use_mask_for_norm=False)")
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
    if normalization == "ct":
        stats32 = _ct_stats(foreground_intensity_properties_per_channel, int(d.shape[0]), d.device)
        out, seg_out, counts = ops_raw.crop_clip_normalize(lib, d, stats32, start, crop_shape, mask=filled, seg=s)
    else:
        _, stats32 = ops_raw.crop_stats(lib, d, start, crop_shape, mask=filled, seg=s, masked=use_mask_for_norm)
        out, seg_out, counts = ops_raw.crop_normalize(lib, d, stats32, start, crop_shape, mask=filled, seg=s, masked=use_mask_for_norm)
    if new_shape != crop_shape:
        # an invalid seg value was written as label 0 and would be lost in the zoom: the first counts flag it (on the device)
        invalid = counts[L.PREP_BIN_INVALID]
        do_separate_z, axis = RS.decide_separate_z(spacing_trans, target, force_separate_z)
        if do_separate_z:
            axis = RS._separate_axis(axis, 0)
            out = RS._resample(out, new_shape, False, 3, separate_axis=axis)
            seg_out, counts = RS._resample(seg_out[None], new_shape, True, 1, with_counts=True, separate_axis=axis)
            seg_out = seg_out[0]
        else:
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
                 resample: bool = False, force_separate_z=False):
        self.base_dir, self.image_dir = str(base_dir), str(image_dir)
        self.data_filenames, self.seg_filename = list(data_filenames), seg_filename
        self.use_mask_for_norm, self.resample, self.force_separate_z = use_mask_for_norm, resample, force_separate_z
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
        data, seg = preprocess_case(data, seg, properties, self.out_spacing, self.all_labels, self.use_mask_for_norm, self.resample,
                                    force_separate_z=self.force_separate_z)
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


class CTCasePreprocessor:
    """`DefaultPreprocessor` (preprocessors/default_preprocessor.py:137-505): one NIfTI file per case in `base_dir/image_dir`, its
    label under the same name in `base_dir/label_dir`; single channel.  `run_plan` is the dataset fingerprint, `run` writes the
    reference's `<case>.npz` / `<case>.pkl` with the CT normalisation, one case after the other."""

    def __init__(self, base_dir, image_dir, label_dir=None, data_type: str = "CT", resample: bool = True, force_separate_z=False):
        self.base_dir, self.image_dir = str(base_dir), str(image_dir)
        self.label_dir = None if label_dir is None else str(label_dir)
        self.data_type, self.resample, self.force_separate_z = data_type, resample, force_separate_z
        self.out_spacing, self.all_labels, self.output_dir = (1, 1, 1), (1, 2, 3), None
        self.foreground_intensity_properties_per_channel = None

    def get_iterable_list(self):
        return sorted(os.listdir(os.path.join(self.base_dir, self.image_dir)))

    def read_data(self, case_name):
        """:245-270: data (1, D, H, W) float32, seg (1, D, H, W) float32 or None, properties with the case's fingerprint"""
        from .nifti import read_nifti
        arr, spacing = read_nifti(os.path.join(self.base_dir, self.image_dir, case_name))
        data = arr.astype(np.float32)[None]
        seg, intensities, statistics = None, [], []
        if self.label_dir is not None:
            seg = read_nifti(os.path.join(self.base_dir, self.label_dir, case_name))[0].astype(np.float32)[None]
            intensities, statistics = collect_foreground_intensities(seg, data)
        properties = {"spacing": tuple(float(v) for v in spacing), "raw_size": tuple(int(v) for v in data.shape[1:]),
                      "name": case_name.split(".")[0], "intensities_per_channel": intensities,
                      "intensity_statistics_per_channel": statistics}
        return data, seg, properties

    def run_case(self, case_name):
        data, seg, properties = self.read_data(case_name)
        data, seg = preprocess_case(data, seg, properties, self.out_spacing, self.all_labels, False, self.resample, normalization="ct",
                                    foreground_intensity_properties_per_channel=self.foreground_intensity_properties_per_channel,
                                    force_separate_z=self.force_separate_z)
        return data, seg, properties

    def run_case_save(self, case_name):
        data, seg, properties = self.run_case(case_name)
        stem = os.path.join(self.output_dir, case_name.split(".")[0])
        np.savez_compressed(stem + ".npz", data=data.cpu().numpy(), seg=None if seg is None else seg.cpu().numpy())
        with open(stem + ".pkl", "wb") as f:
            pickle.dump(properties, f)
        return stem + ".npz"

    def experiment_plan(self, case_name):
        """:294-302"""
        _, _, properties = self.read_data(case_name)
        return properties["spacing"], properties["raw_size"], properties["intensities_per_channel"]

    def determine_fullres_target_spacing(self, spacings, sizes) -> np.ndarray:
        """:304-333: the median spacing; where one axis is more than 3 x coarser than the others AND has fewer than a third of
        their voxels, that axis takes the 10th percentile of its spacings, kept above the other axes' spacing"""
        target = np.percentile(np.vstack(spacings), 50, 0)
        target_size = np.percentile(np.vstack(sizes), 50, 0)
        worst = int(np.argmax(target))
        others = [i for i in range(len(target)) if i != worst]
        other_spacings = [target[i] for i in others]
        other_sizes = [target_size[i] for i in others]
        has_aniso_spacing = target[worst] > (3 * max(other_spacings))
        has_aniso_voxels = target_size[worst] * 3 < min(other_sizes)
        if has_aniso_spacing and has_aniso_voxels:
            of_that_axis = np.percentile(np.vstack(spacings)[:, worst], 10)
            if of_that_axis < max(other_spacings):
                of_that_axis = max(max(other_spacings), of_that_axis) + 1e-5
            target[worst] = of_that_axis
        return target

    def compute_new_shape(self, old_shape, old_spacing, new_spacing) -> np.ndarray:
        """:335-345: the spacings arrive as (x, y, z) and are reversed to the shape's order"""
        old_spacing, new_spacing = list(old_spacing)[::-1], list(new_spacing)[::-1]
        if not len(old_spacing) == len(old_shape) == len(new_spacing):
            raise RuntimeError("compute_new_shape: shape and spacings differ in length")
        return np.array([int(round(i / j * k)) for i, j, k in zip(old_spacing, new_spacing, old_shape)])

    def run_plan(self, analysis_path="./data_analysis_result.txt") -> dict:
        """:347-410 without `target medium patch size`: per case spacing, raw size and the fingerprint's samples; over the dataset the
        statistics of the pooled samples (plain numpy on 10 000 x cases floats), the target spacing, the median shape after
        resampling and the initial patch size.  Writes the reference's JSON to `analysis_path` and returns the dict."""
        spacings, sizes, per_case = [], [], []
        for case in self.get_iterable_list():
            spacing, size, intensities = self.experiment_plan(case)
            spacings.append(spacing)
            sizes.append(size)
            per_case.append(intensities)
        if not per_case:
            raise RuntimeError(f"run_plan: no case in {os.path.join(self.base_dir, self.image_dir)}")
        num_channels = len(per_case[0])
        pooled = [np.concatenate([r[i] for r in per_case]) for i in range(num_channels)]
        statistics = {}
        for i in range(num_channels):
            statistics[i] = {
                "mean": float(np.mean(pooled[i])),
                "median": float(np.median(pooled[i])),
                "std": float(np.std(pooled[i])),
                "min": float(np.min(pooled[i])),
                "max": float(np.max(pooled[i])),
                "percentile_99_5": float(np.percentile(pooled[i], 99.5)),
                "percentile_00_5": float(np.percentile(pooled[i], 0.5)),
            }
        fullres_spacing = self.determine_fullres_target_spacing(spacings, sizes)
        new_shapes = [self.compute_new_shape(j, i, fullres_spacing) for i, j in zip(spacings, sizes)]
        median_shape = np.median(new_shapes, 0)
        tmp = 1 / np.array(fullres_spacing)
        initial_patch_size = [int(round(i)) for i in tmp * (256 ** 3 / np.prod(tmp)) ** (1 / 3)]
        plan = {"intensity_statistics_per_channel": statistics, "fullres spacing": fullres_spacing.tolist(),
                "median_shape": median_shape.tolist(), "initial_patch_size": initial_patch_size}
        if analysis_path is not None:
            with open(analysis_path, "w") as f:
                f.write(json.dumps(plan))
        return plan

    def run(self, output_spacing, output_dir, all_labels, foreground_intensity_properties_per_channel=None):
        """:484-505.  `foreground_intensity_properties_per_channel`: `run_plan`'s `intensity_statistics_per_channel` (keys str(c) as
        the JSON gives them back, or ints)"""
        if output_dir is None:
            raise RuntimeError("CTCasePreprocessor.run: output_dir is required")
        if foreground_intensity_properties_per_channel is None:
            raise RuntimeError("CTCasePreprocessor.run: the CT normalisation needs foreground_intensity_properties_per_channel (run_plan)")
        self.out_spacing, self.all_labels, self.output_dir = output_spacing, all_labels, str(output_dir)
        self.foreground_intensity_properties_per_channel = foreground_intensity_properties_per_channel
        os.makedirs(self.output_dir, exist_ok=True)
        return [self.run_case_save(case) for case in self.get_iterable_list()]
