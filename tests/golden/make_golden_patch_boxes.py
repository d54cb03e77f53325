"""Generate tests/golden/patch_boxes.npz by running the REFERENCE's own patch loader.

    python tests/golden/make_golden_patch_boxes.py <path of the reference checkout>

The reference's `DataLoaderMultiProcess` (light_training/dataloading/base_data_loader.py; the module imports numpy only) is loaded
from the checkout at generation time and its `generate_train_batch` is run, as it is, on the stand-in dataset of
tests/preprocess_ref.py under fixed `np.random.seed` values, for both oversampling rules.  What its `get_bbox` was asked and what it
answered is recorded on the way: per scenario the keys (batches, batch), the lower and upper corners (batches, batch, 3) and the
forced-foreground flags.  The fixture holds integers only; no reference code goes into this repository.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import preprocess_ref as R  # noqa: E402


def main(reference: str):
    path = os.path.join(reference, "light_training", "dataloading", "base_data_loader.py")
    spec = importlib.util.spec_from_file_location("reference_base_data_loader", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = {}
    for name, (probabilistic, seed) in R.PATCH_SCENARIOS.items():
        dataset = R.patch_standin_dataset()
        loader = mod.DataLoaderMultiProcess(dataset, list(R.PATCH_SIZE), batch_size=R.PATCH_BATCH, oversample_foreground_percent=0.33,
                                            probabilistic_oversampling=probabilistic)
        asked = []
        inner = loader.get_bbox

        def recording(data_shape, force_fg, class_locations, *a, _inner=inner, _asked=asked, **k):
            lbs, ubs = _inner(data_shape, force_fg, class_locations, *a, **k)
            _asked.append((bool(force_fg), [int(v) for v in lbs], [int(v) for v in ubs]))
            return lbs, ubs
        loader.get_bbox = recording
        np.random.seed(seed)
        keys = []
        for _ in range(R.PATCH_BATCHES):
            batch = loader.generate_train_batch()
            keys.append([int(k) for k in batch["keys"]])
            assert batch["data"].shape == (R.PATCH_BATCH, 2) + tuple(R.PATCH_SIZE)
        shape = (R.PATCH_BATCHES, R.PATCH_BATCH)
        out[name + "_keys"] = np.asarray(keys, dtype=np.int32)
        out[name + "_forced"] = np.asarray([a[0] for a in asked], dtype=np.uint8).reshape(shape)
        out[name + "_lbs"] = np.asarray([a[1] for a in asked], dtype=np.int32).reshape(shape + (3,))
        out[name + "_ubs"] = np.asarray([a[2] for a in asked], dtype=np.int32).reshape(shape + (3,))
    dst = os.path.join(HERE, "patch_boxes.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
