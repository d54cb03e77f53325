"""Finishing a prediction on the device: logits -> label volume, connected components, hole filling (csrc/postprocess.hip,
csrc/ccl_roots.hip).

The stage of the reference's pipeline between `maybe_mirror_and_predict` and the file on disk (4_predict.py:75-99 on
light_training/prediction.py): resample the logits to the pre-resample crop shape, arg-max, paste into the un-cropped volume
(`labels_from_logits`: one launch), and the optional `large_connected_domain` post-processing - label the components, keep the
largest, fill its holes (`largest_connected_domain`).  The functions carry the reference's, scipy's and skimage's names and
definitions for 3-D volumes of fewer than 2^31 voxels.  Tensors stay on the device; numpy arrays and host tensors are uploaded.  No
call reads a volume back.

`connectivity` is 1, 2 or 3 as in `scipy.ndimage.generate_binary_structure(3, c)` and `skimage.measure.label(connectivity=c)`: 6
(faces), 18 (faces and edges) or 26 (faces, edges and corners) neighbours.  The default everywhere is 1, which is what the reference's
`large_connected_domain` passes; nnU-Net's post-processing, cc3d and the BraTS lesion-wise tooling label at 3.
It is the connectivity of the FOREGROUND components.  Where a function also fills holes (`largest_connected_domain`,
`postprocess_labels`, `keep_largest_per_class(fill_holes=True)`) the background flood stays at connectivity 1 whatever the foreground's:
that is `measure.label(connectivity=c)` followed by `ndimage.binary_fill_holes(...)` with its default structure, and the topologically
consistent pairing (a 26-connected foreground with a 6-connected background).  Only `binary_fill_holes` takes the background's
connectivity itself.  Any other value is a ValueError.

Where this deliberately differs from the reference:
  * `largest_connected_domain` of an empty mask returns the empty mask (the reference raises IndexError on `volume_sort[-1]`);
  * of equally large components the one whose first voxel comes LAST in memory order is kept - a definition; the reference takes
    `np.argsort(volume)[-1]`, which numpy leaves undefined for ties;
  * the resampled logits are compared in fp32 (the CPU branch of `predict_raw_probability`; its GPU branch rounds them to fp16 first).
`postprocess_labels` (per region of a label map) is this project's addition: the reference applies its function to one binary mask.

Multi-organ label maps (the reference's CT example, light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:87-109: the
argmax over 10 classes, one file per organ): `labels_from_logits` takes up to 32 classes, and `keep_largest_per_class` keeps the
largest component of every class from ONE labelled connected-components pass (csrc/ccl_roots.hip, csrc/ccl_labels.hip)
instead of one pass per class.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import lib as L
from . import ops_raw
from .metrics import BRATS_REGIONS, _table, _to_device


def _mask(x, what: str) -> torch.Tensor:
    """non-zero = inside: uint8, contiguous, (D, H, W), on the device"""
    t = _to_device(x)
    if t.dim() != 3:
        raise RuntimeError(f"{what}: a (D, H, W) volume is required, got shape {tuple(t.shape)}")
    if t.numel() == 0 or t.numel() > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"{what}: between 1 and 2^31 - 1 voxels, got shape {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        t = (t != 0).to(torch.uint8)
    return t.contiguous()


def component_roots(mask, connectivity: int = 1) -> torch.Tensor:
    """int32 (D, H, W): -1 outside the mask, otherwise the smallest linear index of the voxel's component at `connectivity`"""
    connectivity = ops_raw._connectivity(connectivity, "component_roots")
    return ops_raw.ccl_roots(L.get_lib(), _mask(mask, "component_roots"), connectivity=connectivity)


def label(mask, return_num: bool = True, connectivity: int = 1):
    """scipy.ndimage.label(structure=generate_binary_structure(3, connectivity)) / skimage.measure.label(connectivity=connectivity):
    int32 labels, 0 = background, the components numbered 1 .. num in memory order of their first voxel (ascending root: scipy's
    raster order at every connectivity).  -> (labels, num) or labels."""
    connectivity = ops_raw._connectivity(connectivity, "label")
    roots = ops_raw.ccl_roots(L.get_lib(), _mask(mask, "label"), connectivity=connectivity)
    flat = roots.reshape(-1)
    is_root = flat == torch.arange(flat.numel(), dtype=torch.int32, device=flat.device)
    rank = torch.cumsum(is_root, 0, dtype=torch.int32)                    # rank of a root among the roots = its number
    labels = torch.where(flat >= 0, rank[flat.clamp(min=0).long()], torch.zeros((), dtype=torch.int32, device=flat.device))
    labels = labels.reshape(roots.shape)
    return (labels, int(rank[-1].item())) if return_num else labels


def _fill(lib, m: torch.Tensor, connectivity: int = 1) -> torch.Tensor:
    """`connectivity` of the background flood"""
    roots = ops_raw.ccl_roots(lib, m, invert=True, connectivity=connectivity)
    sizes, touches = ops_raw.ccl_sizes(lib, roots)
    return ops_raw.ccl_select(lib, roots, sizes, L.CCL_FILL, touches=touches)[0]


def _keep(lib, m: torch.Tensor, keep, bit: int = -1, connectivity: int = 1) -> torch.Tensor:
    roots = ops_raw.ccl_roots(lib, m, bit=bit, connectivity=connectivity)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    if keep == "largest":
        return ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST)[0]
    return ops_raw.ccl_select(lib, roots, sizes, L.CCL_MIN_SIZE, min_size=int(keep))[0]


def binary_fill_holes(mask, connectivity: int = 1) -> torch.Tensor:
    """scipy.ndimage.binary_fill_holes: the mask plus every zero voxel that no path of neighbouring zero voxels connects to a face of
    the volume.  `connectivity` is that of the BACKGROUND flood, scipy's `structure=generate_binary_structure(3, connectivity)`; the
    default 1 (face-adjacent zero voxels) is scipy's default structure.  At 3 a hole that opens to the outside through a corner is no
    hole.  -> uint8 0 / 1."""
    connectivity = ops_raw._connectivity(connectivity, "binary_fill_holes")
    return _fill(L.get_lib(), _mask(mask, "binary_fill_holes"), connectivity)


def remove_small_components(mask, min_size: int, connectivity: int = 1) -> torch.Tensor:
    """the voxels of the components (at `connectivity`) of at least `min_size` voxels (skimage.morphology.remove_small_objects keeps
    size >= min_size)"""
    connectivity = ops_raw._connectivity(connectivity, "remove_small_components")
    return _keep(L.get_lib(), _mask(mask, "remove_small_components"), int(min_size), connectivity=connectivity)


def largest_connected_domain(mask, connectivity: int = 1) -> torch.Tensor:
    """`large_connected_domain` of the reference (prediction.py:17-27): the largest component, its holes filled.  -> uint8 0 / 1.
    An empty mask comes back empty; equal sizes: the component that comes last in memory order.  `connectivity` is that of the
    components (the reference passes 1); the holes are filled at background connectivity 1 whatever it is, as
    `measure.label(connectivity=c)` followed by `ndimage.binary_fill_holes(...)` does."""
    connectivity = ops_raw._connectivity(connectivity, "largest_connected_domain")
    lib = L.get_lib()
    return _fill(lib, _keep(lib, _mask(mask, "largest_connected_domain"), "largest", connectivity=connectivity))


def component_summary(mask, connectivity: int = 1) -> Tuple[int, int]:
    """(number of components at `connectivity`, voxels of the largest): two scalars read back"""
    connectivity = ops_raw._connectivity(connectivity, "component_summary")
    lib = L.get_lib()
    roots = ops_raw.ccl_roots(lib, _mask(mask, "component_summary"), connectivity=connectivity)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    info = ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST)[1].tolist()
    return int(info[0]), int(info[2])


def _ints(v, n: int, what: str):
    out = [int(x.item()) if isinstance(x, torch.Tensor) else int(x) for x in list(v)[:n]]
    if len(out) != n:
        raise RuntimeError(f"{what}: {n} entries required, got {v}")
    return out


def labels_from_logits(logits, properties: Optional[dict] = None, regions: Optional[Sequence[Sequence[int]]] = None):
    """(C, d, h, w) or (1, C, d, h, w) logits -> uint8 label volume on the device, in one launch: `predict_raw_probability`, `argmax`
    over the classes and `predict_noncrop_probability` of the reference.  With `properties` (the reference's loader's dict; ints or
    0-d tensors) the logits are resampled to `shape_after_cropping_before_resample` and pasted at `bbox_used_for_cropping` into zeros of
    `shape_before_cropping`; without it the labels have the logits' shape.  With `regions` also the region bit planes of the labels
    (what `ops_raw.edt_sq` and the other evaluation kernels take): -> (labels, planes)."""
    t = _to_device(logits)
    if t.dim() == 5 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 4:
        raise RuntimeError(f"labels_from_logits: (C, d, h, w) logits are required, got shape {tuple(t.shape)}")
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        t = t.contiguous()
    table = None if regions is None else _table(regions, t.device)
    if properties is None:
        return ops_raw.resample_argmax(L.get_lib(), t, table=table, max_classes=L.RESAMPLE_CLASS_LIMIT)
    box_shape = _ints(properties["shape_after_cropping_before_resample"], 3, "shape_after_cropping_before_resample")
    out_shape = _ints(properties["shape_before_cropping"], 3, "shape_before_cropping")
    bbox = [_ints(bb, 2, "bbox_used_for_cropping") for bb in list(properties["bbox_used_for_cropping"])[:3]]
    if len(bbox) != 3 or any(b1 - b0 != n for (b0, b1), n in zip(bbox, box_shape)):
        raise RuntimeError(f"labels_from_logits: bbox_used_for_cropping {bbox} does not have the shape {box_shape}")
    return ops_raw.resample_argmax(L.get_lib(), t, out_shape, [b0 for b0, _ in bbox], box_shape, table=table,
                                   max_classes=L.RESAMPLE_CLASS_LIMIT)


def postprocess_labels(labels, regions: Sequence[Sequence[int]] = BRATS_REGIONS, keep="largest", fill_holes: bool = True,
                       connectivity: int = 1) -> torch.Tensor:
    """The per-region form for a label map (this project's addition).  For every region in turn: its mask is reduced to the kept
    components (`keep` = "largest" or a minimum voxel count; components at `connectivity`) and, with `fill_holes`, filled (at
    background connectivity 1 whatever `connectivity` is); the region's voxels that fall outside the result become 0.  Voxels are
    only ever removed: a filled hole keeps whatever label it had.  -> uint8 labels."""
    connectivity = ops_raw._connectivity(connectivity, "postprocess_labels")
    t = _to_device(labels)
    if t.dim() != 3:
        raise RuntimeError(f"postprocess_labels: a (D, H, W) label volume is required, got shape {tuple(t.shape)}")
    out = (t if t.dtype == torch.uint8 else t.to(torch.uint8)).contiguous().clone()
    lib = L.get_lib()
    for r in range(len(regions)):
        bits = _table(regions, out.device)[out.long()].contiguous()
        kept = _keep(lib, bits, keep, bit=r, connectivity=connectivity)
        if fill_holes:
            kept = _fill(lib, kept)
        inside = ((bits >> r) & 1).bool()
        out[inside & (kept == 0)] = 0
    return out


# ---- every class of a label map in one pass (csrc/ccl_roots.hip, csrc/ccl_labels.hip) ---------------------------------------------------
def _label_volume(x, what: str) -> torch.Tensor:
    """uint8, contiguous, (D, H, W), on the device; integer label maps of other types are converted"""
    t = _to_device(x)
    if t.dim() != 3:
        raise RuntimeError(f"{what}: a (D, H, W) label volume is required, got shape {tuple(t.shape)}")
    if t.numel() == 0 or t.numel() > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"{what}: between 1 and 2^31 - 1 voxels, got shape {tuple(t.shape)}")
    if t.dtype != torch.uint8:
        if t.dtype.is_floating_point or t.dtype == torch.bool:
            raise RuntimeError(f"{what}: integer labels 0 .. 255 are required, got {t.dtype}")
        t = t.to(torch.uint8)
    return t.contiguous()


def label_component_roots(labels, connectivity: int = 1) -> torch.Tensor:
    """int32 (D, H, W): -1 where the label is 0, otherwise the smallest linear index of the voxel's component; a component is a set
    of voxels of ONE non-zero label joined by neighbours at `connectivity`.  On `labels == k` this is
    `component_roots(labels == k, connectivity)`."""
    connectivity = ops_raw._connectivity(connectivity, "label_component_roots")
    return ops_raw.ccl_label_roots(L.get_lib(), _label_volume(labels, "label_component_roots"), connectivity=connectivity)


def _label_select(lib, t: torch.Tensor, keep, apply=None, connectivity: int = 1):
    roots = ops_raw.ccl_label_roots(lib, t, connectivity=connectivity)
    sizes, _ = ops_raw.ccl_sizes(lib, roots)
    if keep == "largest":
        return ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_LARGEST, apply=apply)
    return ops_raw.ccl_label_select(lib, t, roots, sizes, L.CCL_MIN_SIZE, min_size=int(keep), apply=apply)


def keep_largest_per_class(labels, classes: Optional[Sequence[int]] = None, keep="largest", fill_holes: bool = False,
                           connectivity: int = 1) -> torch.Tensor:
    """nnU-Net's per-class post-processing / the reference's `large_connected_domain` per organ, for a whole label map: every voxel
    whose component is not the largest of its label becomes 0 (`keep` = a voxel count: not of at least that many voxels).  Equal
    sizes: the component that comes last in memory order.  `classes` = None selects on every non-zero label, otherwise on the listed
    ones only and the others pass through.  One labelled pass whatever the number of classes; nothing is read back.
    With `fill_holes` every selected class present, in ascending order, then has its holes filled (`binary_fill_holes` of its mask);
    only voxels that are 0 at that moment receive the label.  This reads the per-label summary back once when `classes` is None.
    `connectivity` (1, 2, 3) is that of the components; nnU-Net labels at 3, where a vessel that hangs on its organ by an edge or a
    corner stays.  The hole filling is at background connectivity 1 whatever it is.  -> uint8 labels."""
    connectivity = ops_raw._connectivity(connectivity, "keep_largest_per_class")
    t = _label_volume(labels, "keep_largest_per_class")
    lib = L.get_lib()
    apply = None
    if classes is not None:
        classes = sorted({int(c) for c in classes})
        if any(not 1 <= c <= 255 for c in classes):
            raise RuntimeError(f"keep_largest_per_class: classes must lie in 1 .. 255, got {classes}")
        table = torch.zeros(256, dtype=torch.uint8)
        table[classes] = 1
        apply = table.to(t.device)
    out, info = _label_select(lib, t, keep, apply, connectivity)
    if fill_holes:
        present = classes
        if present is None:
            counts = info[:, 0].tolist()                                  # one readback: which labels there are
            present = [c for c in range(1, 256) if counts[c]]
        for c in present:
            filled = _fill(lib, (out == c).to(torch.uint8))
            out[(out == 0) & (filled != 0)] = c
    return out


def class_component_summary(labels, connectivity: int = 1) -> dict:
    """{label: (number of components at `connectivity`, voxels of the largest)} for every label present: one labelled pass, one
    readback of 256 x 3 integers"""
    connectivity = ops_raw._connectivity(connectivity, "class_component_summary")
    t = _label_volume(labels, "class_component_summary")
    info = _label_select(L.get_lib(), t, "largest", connectivity=connectivity)[1].tolist()
    return {c: (int(info[c][0]), int(info[c][2])) for c in range(1, 256) if info[c][0]}
