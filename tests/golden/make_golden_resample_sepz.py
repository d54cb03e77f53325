"""Generate tests/golden/resample_sepz.npz by running the REFERENCE's own `resample_data_or_seg(..., do_separate_z=True, order_z=0)`.

    python tests/golden/make_golden_resample_sepz.py <path of the reference checkout>

light_training/preprocessing/resampling/default_resampling.py is loaded from the checkout at generation time.  It imports
`skimage.transform.resize` and `batchgenerators.augmentations.utils.resize_segmentation`; neither package is needed to state what the
two do on a 2-D slice, so this maker puts stand-ins on scipy under those names:

  resize(x, shape, order, mode='edge', anti_aliasing=False)   skimage's documented path for these arguments: scipy.ndimage.zoom(x,
      shape / x.shape, order=order, mode='nearest', grid_mode=True), then `_clip_warp_output` with the default clip=True - the result
      clipped to [x.min(), x.max()] of THIS input, which in the separate-z branch is one slice;
  resize_segmentation(seg, shape, order)                      batchgenerators: per label of `np.unique(seg)`, ascending, the `resize`
      above (clip=True, anti_aliasing=False) of the label's indicator as float, `out[r >= 0.5] = label` on zeros of the seg's dtype.

Inputs: channel 0 of tests/resample_sepz_ref.data_case() at DATA_TARGETS (order 3 at all five, order 1 at the first and the last) and
tests/resample_ref.label_case() at SEG_TARGETS.  Recorded: inputs, (axis, new shape, order) per case and the reference's outputs in
the inputs' dtypes.  The fixture holds numbers only; no reference code goes into this repository.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import scipy
from scipy import ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import resample_ref as RR  # noqa: E402
from tests import resample_sepz_ref as SR  # noqa: E402


def resize(image, output_shape, order=1, mode="reflect", anti_aliasing=True, clip=True):
    assert mode == "edge" and not anti_aliasing and clip, "the stand-in covers the reference's arguments only"
    image = np.asarray(image, dtype=np.float64)
    out = ndimage.zoom(image, [o / i for o, i in zip(output_shape, image.shape)], order=order, mode="nearest", grid_mode=True)
    return np.clip(out, image.min(), image.max())


def resize_segmentation(segmentation, new_shape, order=3):
    out = np.zeros(tuple(new_shape), dtype=segmentation.dtype)
    for c in np.unique(segmentation):
        r = resize((segmentation == c).astype(float), new_shape, order, mode="edge", anti_aliasing=False)
        out[r >= 0.5] = c
    return out


def load_reference(reference: str):
    for name, attrs in {"skimage": {}, "skimage.transform": {"resize": resize}, "batchgenerators": {},
                        "batchgenerators.augmentations": {}, "batchgenerators.augmentations.utils": {"resize_segmentation": resize_segmentation}}.items():
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        mod.__path__ = []
        sys.modules[name] = mod
    path = os.path.join(reference, "light_training", "preprocessing", "resampling", "default_resampling.py")
    spec = importlib.util.spec_from_file_location("reference_default_resampling", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main(reference: str):
    ref = load_reference(reference)
    data = SR.data_case()[:1]
    seg = RR.label_case()[None]
    rec = {"data": data, "seg": seg}
    cases = [(axis, shape, 3) for axis, shape in SR.DATA_TARGETS] + [(axis, shape, 1) for axis, shape in (SR.DATA_TARGETS[0], SR.DATA_TARGETS[-1])]
    rec["data_cases"] = np.array([[axis, *shape, order] for axis, shape, order in cases], dtype=np.int64)
    for i, (axis, shape, order) in enumerate(cases):
        out = ref.resample_data_or_seg(data, shape, False, [axis], order, True, order_z=0)
        assert out.dtype == np.float32 and out.shape == (1,) + tuple(shape)
        rec[f"data_out_{i}"] = out
    rec["seg_cases"] = np.array([[axis, *shape] for axis, shape in SR.SEG_TARGETS], dtype=np.int64)
    for i, (axis, shape) in enumerate(SR.SEG_TARGETS):
        out = ref.resample_data_or_seg(seg, shape, True, [axis], 1, True, order_z=0)
        assert out.dtype == np.int16 and out.shape == (1,) + tuple(shape)
        rec[f"seg_out_{i}"] = out
    dst = os.path.join(HERE, "resample_sepz.npz")
    np.savez_compressed(dst, scipy_version=np.array(scipy.__version__), **rec)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
