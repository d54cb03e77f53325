"""Signed-distance and edge training targets on the device (csrc/sdm.hip).

The reference's `light_training/dataloading/dataset_sdm_edge.py` builds, per BraTS region (TC, WT, ET), the edge mask
`mask - binary_erosion(mask)` and the normalised signed distance map (two `scipy.ndimage.distance_transform_edt` and skimage's
`find_boundaries(mode='inner')`), and appends `seg_sdm = 1 - compute_sdf(seg) + seg_edge` to the seg.  It cannot afford that per
batch - its `post()` hook is commented out - and loads a `<case>_seg_sdm.npy` made offline, whose float distances its augmentation
then warps with the label rule.  Here the targets come from the label patch as it leaves the augmenter: one stencil pass
(`segm_sdm_masks`), the library's exact distance transform on the bit planes, one pointwise pass (`segm_sdm_compose`).  Nothing is
copied to the host and nothing waits for the device (the 256-byte region table is uploaded at the first call per device).

`sdm_edge_targets` and `signed_distance` take label volumes; `convert_labels`, `get_edge_points`, `edge_3d` and `compute_sdf` carry
the reference's names and take what it passes them.  The mask-taking forms run the same kernels: every (b, c) mask is a uint8
"label volume" with the one-region table {1}.

Deviations from the reference: its two asserts (`min == -1`, `max == 1`) are not reproduced - they fail on any region without a
voxel off its inner boundary, e.g. one that is two voxels thick; a region that fills the volume gives `sdf = 0` like an empty one
(the reference divides 0 by 0); the output is fp32 (the reference's is float64); 2-D input is a ValueError.
Limits: 3-D volumes, unit spacing (the reference passes no `sampling`), sides up to 2048 and 2^30 voxels per volume.
Memory: the two int32 transforms of a group of pairs take 8 bytes per voxel and (volume, region) pair, at most 8 pairs at a time.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import lib as L
from . import metrics as M
from . import ops_raw

BRATS_REGIONS = M.BRATS_REGIONS
_PAIRS = L.METRICS_MAX_PLANES // 2                  # (volume, region) pairs per distance-transform call: two planes each
_VOLUMES = L.METRICS_MAX_PLANES // 2                # volumes per mask call: their inside and outside volumes are one EDT batch
_ONE = ((1,),)


def _volumes(x, what: str) -> torch.Tensor:
    """label volumes as the mask pass reads them: uint8, int16 or int64 on the device, contiguous.  bool, int8 and int32 are
    widened; floating-point labels are refused (a cast would turn 1.5 into 1 without a word, and checking would wait for the device)"""
    t = M._to_device(x)
    if t.dtype not in (torch.uint8, torch.int16, torch.int64):
        if t.dtype == torch.bool:
            t = t.to(torch.uint8)
        elif t.dtype in (torch.int8, torch.int32):
            t = t.to(torch.int64)
        else:
            raise RuntimeError(f"{what}: integer or bool labels are required, got {t.dtype}")
    return t.contiguous()


def _run(labels: torch.Tensor, regions, want_sdf: bool, want_sdm: bool, want_edge: bool):
    """labels (n, D, H, W) -> [sdf, sdm, edge], each (n, R, D, H, W) fp32 or None.  Volumes in groups of 8 per mask pass, regions in
    groups of 8 per table, their pairs in groups of 8 per distance transform (16 planes: pos^2 and neg^2 of each)."""
    lib = L.get_lib()
    n, shape = labels.shape[0], tuple(labels.shape[1:])
    regions = [tuple(r) for r in regions]
    R = len(regions)
    if R == 0 or n == 0:
        raise RuntimeError("at least one region and one volume are required")
    outs = [torch.empty((n * R,) + shape, dtype=torch.float32, device=labels.device) if w else None for w in (want_sdf, want_sdm, want_edge)]
    dist = want_sdf or want_sdm
    for v0 in range(0, n, _VOLUMES):
        vols = labels[v0:v0 + _VOLUMES]
        nv = vols.shape[0]
        for r0 in range(0, R, L.METRICS_MAX_REGIONS):
            regs = regions[r0:r0 + L.METRICS_MAX_REGIONS]
            bits, counts = ops_raw.sdm_masks(lib, vols, M._table(regs, labels.device), len(regs))
            seeds = bits[:2].reshape((2 * nv,) + shape)                   # volume v: its inside bits; nv + v: its outside bits
            pairs = [(v, r) for v in range(nv) for r in range(len(regs))]
            for p0 in range(0, len(pairs), _PAIRS):
                group = pairs[p0:p0 + _PAIRS]
                edt = None
                if dist:                                                  # plane 2 i: pos^2 (seeds outside), 2 i + 1: neg^2 (seeds inside)
                    planes = [pl for v, r in group for pl in ((nv + v, r), (v, r))]
                    edt = M._edt_sq(lib, seeds, planes, None, "")
                items = [(v, r, 2 * i, 2 * i + 1, (v0 + v) * R + r0 + r) for i, (v, r) in enumerate(group)]
                ops_raw.sdm_compose(lib, bits, counts, edt, items, *outs)
    return [None if t is None else t.view((n, R) + shape) for t in outs]


def _label_batch(labels, what: str):
    t = _volumes(labels, what)
    if t.dim() == 2:
        raise ValueError(f"{what}: 3-D volumes are required, got shape {tuple(t.shape)}")
    if t.dim() not in (3, 4):
        raise RuntimeError(f"{what}: (D, H, W) or (B, D, H, W) labels are required, got shape {tuple(t.shape)}")
    return t if t.dim() == 4 else t[None]


def sdm_edge_targets(labels, regions: Sequence[Sequence[int]] = BRATS_REGIONS) -> Tuple[torch.Tensor, torch.Tensor]:
    """labels (B, D, H, W) or (D, H, W), any integer dtype (uint8, int16 and int64 are read as they are; a value outside 0 .. 255 is
    in no region) -> (edge, sdm), each (B, R, D, H, W) fp32 on the labels' device: the reference's `seg_edge = edge_3d(seg)` and
    `seg_sdm = 1 - compute_sdf(seg) + seg_edge` of `seg = convert_labels(labels)`.  Any number of regions and volumes."""
    _, sdm, edge = _run(_label_batch(labels, "sdm_edge_targets"), regions, False, True, True)
    return edge, sdm


def signed_distance(labels, regions: Sequence[Sequence[int]] = BRATS_REGIONS) -> torch.Tensor:
    """-> sdf (B, R, D, H, W) fp32: `compute_sdf(convert_labels(labels))`, in [-1, 1], 0 on the inner boundary of a region and
    everywhere for a region that is empty or fills the volume"""
    return _run(_label_batch(labels, "signed_distance"), regions, True, False, False)[0]


# ---- the reference's names ------------------------------------------------------------------------------------------------------------
def convert_labels(labels) -> torch.Tensor:
    """(1, 3, *labels.shape) fp32 masks in the order TC, WT, ET (dataset_sdm_edge.py:87-92): `metrics.region_masks` with the
    reference's leading axes.  A label outside 0 .. 255 is in no region, as in `sdm_edge_targets`: it is set to 0 before
    `region_masks` narrows the labels to uint8 (where 300 would become 44 and -1 would become 255)."""
    t = M._to_device(labels)
    if t.dtype not in (torch.uint8, torch.bool):
        t = torch.where((t < 0) | (t > 255), torch.zeros_like(t), t)
    return M.region_masks(t, BRATS_REGIONS)[None]


def _masks(x, what: str) -> torch.Tensor:
    """binary masks (B, C, D, H, W), non-zero = inside -> (B * C, D, H, W) uint8 of 0 / 1"""
    t = M._to_device(x)
    if t.dim() == 4:
        raise ValueError(f"{what}: (B, C, D, H, W) masks of 3-D volumes are required, got the 2-D shape {tuple(t.shape)}")
    if t.dim() != 5:
        raise RuntimeError(f"{what}: (B, C, D, H, W) masks are required, got shape {tuple(t.shape)}")
    return (t != 0).to(torch.uint8).reshape((-1,) + tuple(t.shape[2:])).contiguous()


def get_edge_points(img) -> torch.Tensor:
    """`img - binary_erosion(img)` of one 3-D binary volume (connectivity 1, border_value 0): (D, H, W) fp32 of 0.0 / 1.0"""
    t = M._to_device(img)
    if t.dim() == 2:
        raise ValueError(f"get_edge_points: 3-D volumes are required, got shape {tuple(t.shape)}")
    if t.dim() != 3:
        raise RuntimeError(f"get_edge_points: a (D, H, W) volume is required, got shape {tuple(t.shape)}")
    return edge_3d(t[None, None])[0, 0]


def edge_3d(image_3d) -> torch.Tensor:
    """`get_edge_points` of every (b, c) mask of (B, C, D, H, W): fp32 of 0.0 / 1.0"""
    shape = tuple(M._to_device(image_3d).shape)
    m = _masks(image_3d, "edge_3d")
    return _run(m, _ONE, False, False, True)[2].view(shape)


def compute_sdf(img_gt, out_shape: Optional[Sequence[int]] = None) -> torch.Tensor:
    """The normalised signed distance map of every (b, c) mask of (B, C, D, H, W) (dataset_sdm_edge.py:56-85), fp32.  `out_shape`,
    which the reference takes beside the array, must be the array's shape when given."""
    shape = tuple(M._to_device(img_gt).shape)
    if out_shape is not None and tuple(int(s) for s in out_shape) != shape:
        raise RuntimeError(f"compute_sdf: out_shape {tuple(out_shape)} is not the masks' shape {shape}")
    m = _masks(img_gt, "compute_sdf")
    return _run(m, _ONE, True, False, False)[0].view(shape)
