"""Training patches from preprocessed cases, cut on the device.

The reference's `MedicalDataset` (light_training/dataloading/dataset.py:27-98) and `DataLoaderMultiProcess`
(light_training/dataloading/base_data_loader.py:5-213): cases as `preprocess.CasePreprocessor` (or the reference's
2_preprocessing_mri.py) wrote them, a batch of random patches of which the last third is centred on a foreground voxel.  Which case
and which box is decided on the host with the reference's `np.random` calls in the reference's order - under the same
`np.random.seed` the keys and boxes are the reference's - and the patch is then cut from the case where it already lies, in device
memory: two strided copies per sample into a zeroed batch, no worker processes, no host round trip.

`PatchLoader.next()` returns what `trainer.SyntheticBraTS.next()` returns and `trainer.train_step` takes; the seg's -1 ("outside the
brain") becomes 0 there, which the reference does in its transforms (`RemoveLabelTransform(-1, 0)`, augment/train_augment.py:57).
"""
from __future__ import annotations

import os
import pickle
from typing import Optional, Sequence

import numpy as np
import torch

from .metrics import BRATS_REGIONS


class CaseDataset:
    """`<case>.npz` + `<case>.pkl`, or the `<case>.npy` / `<case>_seg.npy` that the reference's `unpack_dataset` leaves next to
    them (taken when present).  `paths` name the `.npz` files, as the reference's datalists do.  `__getitem__` returns the
    reference's dict - data (C, d, h, w) fp32, seg (1, d, h, w) (absent with `test`), properties - with the arrays on `device`.
    Uploaded cases are kept there while they fit in `cache_bytes`; the default is half of the device's free memory at construction
    (a BraTS training set of 1251 cases of about 45 MB fits an MI355X), and every case when the device is the host.
    `sdm_dir`: the folder of the `<case>_seg_sdm.npy` files of tools/make_sdm_targets.py (the reference's ./data/fullres/train_sdm);
    the file's `[0]`, (3, d, h, w), is appended to the seg's channels, which become fp32, as the `__getitem__` of the reference's
    dataset_sdm_edge.py does (:166-171)."""

    def __init__(self, paths: Sequence[str], test: bool = False, device=None, cache_bytes: Optional[int] = None,
                 sdm_dir: Optional[str] = None):
        self.datalist = [str(p) for p in paths]
        self.test = test
        self.sdm_dir = None if sdm_dir is None else str(sdm_dir)
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        if cache_bytes is None:
            cache_bytes = torch.cuda.mem_get_info(self.device)[0] // 2 if self.device.type == "cuda" else 1 << 62
        self.cache_bytes = int(cache_bytes)
        self.cached_bytes = 0
        self._cache = {}
        self.data_cached = [self.load_pkl(p) for p in self.datalist]

    def load_pkl(self, data_path: str) -> dict:
        with open(data_path[:-4] + ".pkl", "rb") as f:
            return pickle.load(f)

    def read_data(self, data_path: str):
        image_path, seg_path = data_path[:-4] + ".npy", data_path[:-4] + "_seg.npy"
        if os.path.exists(image_path) and (self.test or os.path.exists(seg_path)):
            return np.load(image_path, "r"), None if self.test else np.load(seg_path, "r")
        with np.load(data_path) as z:
            return z["data"], None if self.test else z["seg"]

    def _upload(self, i: int):
        image, seg = self.read_data(self.datalist[i])
        data = torch.from_numpy(np.array(image, dtype=np.float32)).to(self.device)            # a copy: the file may be mapped read-only
        seg = None if seg is None else torch.from_numpy(np.array(seg)).to(self.device)
        if seg is not None and self.sdm_dir is not None:
            sdm = np.load(os.path.join(self.sdm_dir, f"{self.data_cached[i]['name']}_seg_sdm.npy"), "r")[0]
            seg = torch.cat([seg.float(), torch.from_numpy(np.array(sdm, dtype=np.float32)).to(self.device)])
        return data, seg

    def __getitem__(self, i):
        i = int(i)
        hit = self._cache.get(i)
        if hit is None:
            hit = self._upload(i)
            nbytes = sum(t.numel() * t.element_size() for t in hit if t is not None)
            if self.cached_bytes + nbytes <= self.cache_bytes:
                self._cache[i] = hit
                self.cached_bytes += nbytes
        item = {"data": hit[0], "properties": self.data_cached[i]}
        if hit[1] is not None:
            item["seg"] = hit[1]
        return item

    def __len__(self):
        return len(self.datalist)


class PatchLoader:
    """`DataLoaderMultiProcess`: `batch_size` patches of `patch_size` from random cases of `dataset` (anything whose items are the
    reference's dicts).  Sample j is centred on a random voxel of a random non-empty class of the case's `class_locations` when
    `j >= round(batch_size * (1 - oversample_foreground_percent))`, or with probability `oversample_foreground_percent` under
    `probabilistic_oversampling`; otherwise its box is uniform.  A case smaller than the patch is padded with zeros on both sides.
    All draws come from the global `np.random`, in the reference's order.  `seed` seeds the augmenter (`augment=True`: the batch of
    `next()` goes through `augment.DeviceAugmenter`; `augment="spline"`: through `augment.SplineAugmenter`; `augment="fused"`: through
    `augment.FusedAugmenter`, the same chain with the intensity transforms and the mirror on the kernels of csrc/intensity.hip).
    `targets="sdm_edge"` enables `next_with_targets()`, which adds the edge masks and signed-distance maps of `regions`
    (segmamba_amd/sdm.py), computed from the label as it leaves the augmenter."""

    def __init__(self, dataset, patch_size, batch_size: int = 2, oversample_foreground_percent: float = 0.33,
                 probabilistic_oversampling: bool = False, device=None, augment: bool = False, seed: int = 42,
                 targets: Optional[str] = None, regions=BRATS_REGIONS):
        self.dataset = dataset
        self.patch_size = [int(p) for p in patch_size]
        if len(self.patch_size) != 3 or min(self.patch_size) < 1:
            raise RuntimeError(f"PatchLoader: patch_size must be three positive ints, got {patch_size}")
        if targets not in (None, "sdm_edge"):
            raise RuntimeError(f"PatchLoader: targets must be None or 'sdm_edge', got {targets!r}")
        self.targets = targets
        self.regions = tuple(tuple(int(v) for v in r) for r in regions)
        self.batch_size = int(batch_size)
        self.keys = list(range(len(dataset)))
        self.oversample_foreground_percent = oversample_foreground_percent
        self.need_to_pad = np.array([0, 0, 0]).astype(int)
        self.get_do_oversample = self._probabilistic_oversampling if probabilistic_oversampling else self._oversample_last_XX_percent
        self.device = torch.device(device if device is not None else getattr(dataset, "device", "cpu"))
        self.augmenter = None
        if augment:
            from .augment import select_augmenter
            self.augmenter = select_augmenter(augment)(self.device, seed=seed)

    def _oversample_last_XX_percent(self, sample_idx: int) -> bool:
        return not sample_idx < round(self.batch_size * (1 - self.oversample_foreground_percent))

    def _probabilistic_oversampling(self, sample_idx: int) -> bool:
        return np.random.uniform() < self.oversample_foreground_percent

    def get_bbox(self, data_shape, force_fg: bool, class_locations, overwrite_class=None):
        """-> (lower, upper) corners of the patch in the case's coordinates; they may lie outside the case (zero padding)"""
        dim = len(data_shape)
        need = [max(int(self.need_to_pad[d]), self.patch_size[d] - int(data_shape[d])) for d in range(dim)]
        lbs = [(-need[d]) // 2 for d in range(dim)]
        ubs = [int(data_shape[d]) + need[d] // 2 + need[d] % 2 - self.patch_size[d] for d in range(dim)]
        voxel = None
        if force_fg:
            if class_locations is None:
                raise RuntimeError("PatchLoader.get_bbox: a forced-foreground sample needs the case's class_locations")
            eligible = [k for k in class_locations.keys() if len(class_locations[k]) > 0]
            if eligible:
                if overwrite_class is not None and overwrite_class in eligible:
                    chosen = overwrite_class
                else:
                    chosen = eligible[np.random.choice(len(eligible))]
                locs = class_locations[chosen]
                voxel = locs[np.random.choice(len(locs))]
        if voxel is None:                             # a uniform box; also what a case without foreground falls back to
            lower = [int(np.random.randint(lbs[d], ubs[d] + 1)) for d in range(dim)]
        else:                                         # centred on the voxel (column 0 is the seg's channel), clamped from below only
            lower = [max(lbs[d], int(voxel[d + 1]) - self.patch_size[d] // 2) for d in range(dim)]
        return lower, [lower[d] + self.patch_size[d] for d in range(dim)]

    def _draw(self):
        """the host side of a batch: keys, items and boxes, with the reference's draws in the reference's order"""
        keys = np.random.choice(self.keys, self.batch_size, True, None)
        picks = []
        for j, key in enumerate(keys):
            force_fg = self.get_do_oversample(j)
            item = self.dataset[key]
            if "seg" not in item:
                raise RuntimeError("PatchLoader: the dataset's items have no seg (a test dataset cannot feed training)")
            lower, upper = self.get_bbox(item["data"].shape[1:], force_fg, item["properties"]["class_locations"])
            picks.append((item, lower, upper))
        return keys, picks

    def _cut(self, picks):
        first = picks[0][0]
        data_all = torch.zeros((self.batch_size, first["data"].shape[0], *self.patch_size), dtype=torch.float32, device=self.device)
        seg_all = torch.zeros((self.batch_size, first["seg"].shape[0], *self.patch_size), dtype=torch.float32, device=self.device)
        for j, (item, lower, upper) in enumerate(picks):
            shape = item["data"].shape[1:]
            src = tuple(slice(max(0, lo), min(int(n), up)) for lo, up, n in zip(lower, upper, shape))
            dst = tuple(slice(s.start - lo, s.stop - lo) for s, lo in zip(src, lower))
            data, seg = item["data"], item["seg"]
            if not isinstance(data, torch.Tensor):
                data, seg = torch.from_numpy(np.ascontiguousarray(data[(slice(None), *src)])), torch.from_numpy(np.ascontiguousarray(seg[(slice(None), *src)]))
                src = (slice(None),) * 3
            data_all[(j, slice(None), *dst)] = data[(slice(None), *src)].to(self.device)
            seg_all[(j, slice(None), *dst)] = seg[(slice(None), *src)].to(self.device)
        return data_all, seg_all

    def next_batch(self) -> dict:
        """`generate_train_batch`: {data (B, C, *patch) fp32, seg (B, 1, *patch) fp32 with the -1 kept, properties, keys}"""
        keys, picks = self._draw()
        data_all, seg_all = self._cut(picks)
        return {"data": data_all, "seg": seg_all, "properties": [p[0]["properties"] for p in picks], "keys": keys}

    __next__ = next_batch

    def next(self):
        """-> (image (B, C, *patch) float32, label (B, *patch) int64), -1 mapped to 0"""
        batch = self.next_batch()
        image, label = batch["data"], batch["seg"][:, 0].clamp_min(0).long()
        if self.augmenter is not None:
            image, label = self.augmenter(image, label)
        return image, label

    def next_with_targets(self):
        """-> (image, label, edge, sdm): `next()`, then the edge masks and `1 - sdf + edge` of the label that `next()` returned, each
        (B, R, *patch) fp32 (`sdm.sdm_edge_targets`): the targets of the augmented patch, not a warped copy of a whole-case file"""
        if self.targets != "sdm_edge":
            raise RuntimeError("PatchLoader.next_with_targets: construct the loader with targets='sdm_edge'")
        from .sdm import sdm_edge_targets
        image, label = self.next()
        edge, sdm = sdm_edge_targets(label, self.regions)
        return image, label, edge, sdm
