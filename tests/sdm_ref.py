"""numpy float64 restatement of the reference's light_training/dataloading/dataset_sdm_edge.py: `compute_sdf`, `get_edge_points`,
`edge_3d` and `convert_labels`, with the scipy calls the reference makes.  skimage's `find_boundaries(mode='inner')` is restated
from its published source for a boolean image: `(grey_dilation(u, cross) != grey_erosion(u, cross)) & mask` with scipy's default
reflecting border.  The reference's two asserts (min == -1, max == 1) are left out: `asserts_hold` reports them.  `full_is_zero`
states the device's rule for a region that fills the volume (sdf = 0), where the reference divides 0 by 0."""
import numpy as np
from scipy import ndimage
from scipy.ndimage import distance_transform_edt as distance

BRATS_REGIONS = ((1, 3), (1, 2, 3), (3,))           # TC, WT, ET


def find_boundaries_inner(mask):
    """skimage.segmentation.find_boundaries(mask, mode='inner') for a boolean image"""
    u = np.asarray(mask).astype(np.uint8)
    cross = ndimage.generate_binary_structure(u.ndim, 1)
    return (ndimage.grey_dilation(u, footprint=cross) != ndimage.grey_erosion(u, footprint=cross)) & (u != 0)


def get_edge_points(img):
    strt = ndimage.generate_binary_structure(len(img.shape), 1)
    ero = ndimage.binary_erosion(img, strt)
    return np.asarray(img, np.uint8) - np.asarray(ero, np.uint8)


def edge_3d(image_3d):
    out = np.zeros_like(image_3d)
    for i in range(image_3d.shape[0]):
        for j in range(image_3d.shape[1]):
            out[i, j] = get_edge_points(image_3d[i, j])
    return out


def sdf_of_mask(posmask, full_is_zero=True):
    """one (b, c) plane of compute_sdf, float64"""
    posmask = np.asarray(posmask).astype(np.uint8).astype(np.bool_)
    if not posmask.any() or (full_is_zero and posmask.all()):
        return np.zeros(posmask.shape)
    negmask = ~posmask
    posdis = distance(posmask)
    negdis = distance(negmask)
    boundary = find_boundaries_inner(posmask).astype(np.uint8)
    sdf = (negdis - np.min(negdis)) / (np.max(negdis) - np.min(negdis)) - (posdis - np.min(posdis)) / (np.max(posdis) - np.min(posdis))
    sdf[boundary == 1] = 0
    return sdf


def compute_sdf(img_gt, out_shape=None, full_is_zero=True):
    img_gt = np.asarray(img_gt).astype(np.uint8)
    out_shape = img_gt.shape if out_shape is None else out_shape
    out = np.zeros(out_shape)
    for b in range(out_shape[0]):
        for c in range(out_shape[1]):
            out[b][c] = sdf_of_mask(img_gt[b, c], full_is_zero)
    return out


def asserts_hold(sdf):
    """the reference's two asserts on one plane"""
    return np.min(sdf) == -1.0 and np.max(sdf) == 1.0


def region_masks(labels, regions=BRATS_REGIONS):
    """(R, *labels.shape) float64 of 0 / 1; a label outside every region's list (such as -1 or 300) is in none"""
    labels = np.asarray(labels)
    return np.stack([np.isin(labels, list(r)) for r in regions]).astype(np.float64)


def convert_labels(labels):
    """(1, 3, *labels.shape) float64: TC, WT, ET"""
    return region_masks(labels, BRATS_REGIONS)[None]


def targets(labels, regions=BRATS_REGIONS):
    """labels (B, D, H, W) -> (edge, sdf, sdm), each (B, R, D, H, W) float64: what dataset_sdm_edge.py's `post` makes of a batch"""
    labels = np.asarray(labels)
    seg = np.stack([region_masks(v, regions) for v in labels])
    edge = edge_3d(seg)
    sdf = compute_sdf(seg, seg.shape)
    return edge, sdf, 1 - sdf + edge
