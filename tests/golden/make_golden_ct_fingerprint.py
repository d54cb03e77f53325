"""Generate tests/golden/ct_fingerprint.npz by running the REFERENCE's own `collect_foreground_intensities`.

    python tests/golden/make_golden_ct_fingerprint.py <path of the reference checkout>

`DefaultPreprocessor.collect_foreground_intensities` (light_training/preprocessing/preprocessors/default_preprocessor.py) needs numpy
only, but its module imports SimpleITK, batchgenerators, tqdm and the package's cropping / resampling / normalisation modules at the
top.  The file is loaded from the checkout at generation time with empty stand-in modules under those names (the star import from
batchgenerators must bring `List`, which the class's annotations use) and the method is run, as it is, on the stand-in CT case of
tests/ct_ref.py.  Recorded: the 10 000 drawn samples of the one channel (float32) and its six statistics as float32, with their
names.  The fixture holds numbers only; no reference code goes into this repository.
"""
import importlib.util
import os
import sys
import types
import typing

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import ct_ref as CR  # noqa: E402

STAND_INS = {
    "batchgenerators": {}, "batchgenerators.utilities": {},
    "batchgenerators.utilities.file_and_folder_operations": {"List": typing.List, "os": os},
    "light_training": {}, "light_training.preprocessing": {},
    "light_training.preprocessing.cropping": {}, "light_training.preprocessing.cropping.cropping": {"crop_to_nonzero": None},
    "light_training.preprocessing.resampling": {},
    "light_training.preprocessing.resampling.default_resampling": {"resample_data_or_seg_to_shape": None, "compute_new_shape": None},
    "light_training.preprocessing.normalization": {},
    "light_training.preprocessing.normalization.default_normalization_schemes": {"CTNormalization": None, "ZScoreNormalization": None},
    "tqdm": {"tqdm": None}, "SimpleITK": {},
}


def main(reference: str):
    for name, attrs in STAND_INS.items():
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            mod.__path__ = []
            sys.modules[name] = mod
    path = os.path.join(reference, "light_training", "preprocessing", "preprocessors", "default_preprocessor.py")
    spec = importlib.util.spec_from_file_location("reference_default_preprocessor", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pre = mod.DefaultPreprocessor("", "", "")
    data, seg = CR.ct_case()
    samples, stats = pre.collect_foreground_intensities(seg, data)
    assert len(samples) == 1 and samples[0].dtype == np.float32 and samples[0].shape == (10000,)
    keys = sorted(stats[0])
    dst = os.path.join(HERE, "ct_fingerprint.npz")
    np.savez_compressed(dst, samples=np.stack(samples), keys=np.array(keys), numpy_version=np.array(np.__version__),
                        statistics=np.array([[np.float32(s[k]) for k in keys] for s in stats], dtype=np.float32))
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
