"""Generate tests/golden/sdm_edge.npz by running the REFERENCE's own `convert_labels`, `edge_3d` and `compute_sdf`.

    python tests/golden/make_golden_sdm.py <path of the reference checkout>

`light_training/dataloading/dataset_sdm_edge.py` imports sklearn, SimpleITK, tqdm, monai, batchgenerators and skimage at its top; the
three functions use numpy, torch, scipy.ndimage and one skimage call, `segmentation.find_boundaries(posmask, mode='inner')`.  The
modules the functions do not need are put in front of the import as empty stand-ins.  skimage is not a dependency of this
repository: `skimage.segmentation.find_boundaries` is forwarded to the restatement in tests/sdm_ref.py (which
tests/test_sdm_ref_cpu.py pins to the real function where skimage is installed).  Everything else - the erosion, the two distance
transforms, the normalisation, the two asserts, the label regions - is the reference's code, imported from the checkout at
generation time and run as it is.  Recorded for the case of tests/sdm_checks.fixture_labels: the labels, `convert_labels` (1, 3, ...),
`edge_3d` of it, `compute_sdf` of it (float64; all three regions pass the reference's asserts) and `1 - sdf + edge`.  The fixture
holds numbers only; no reference code goes into this repository.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def stand_in(name, **attrs):
    mod = types.ModuleType(name)
    for k, v in attrs.items():
        setattr(mod, k, v)
    sys.modules[name] = mod
    parent, _, child = name.rpartition(".")
    if parent:
        setattr(sys.modules[parent], child, mod)
    return mod


def main(reference: str):
    import torch
    from tests import sdm_checks as C
    from tests import sdm_ref as S

    def find_boundaries(label_img, connectivity=1, mode="thick", background=0):
        assert mode == "inner" and connectivity == 1 and label_img.dtype == np.bool_
        return S.find_boundaries_inner(label_img)

    stand_in("sklearn")
    stand_in("sklearn.model_selection", KFold=object)
    stand_in("SimpleITK")
    stand_in("tqdm", tqdm=lambda it, **kw: it)
    stand_in("monai", transforms=types.ModuleType("monai.transforms"))
    stand_in("batchgenerators")
    stand_in("batchgenerators.utilities")
    stand_in("batchgenerators.utilities.file_and_folder_operations", isfile=os.path.isfile, subfiles=None)
    stand_in("skimage")
    stand_in("skimage.segmentation", find_boundaries=find_boundaries)
    stand_in("skimage.morphology", dilation=None, disk=None)
    sys.path.insert(0, reference)
    from light_training.dataloading import dataset_sdm_edge as ref

    labels = C.fixture_labels()
    seg = ref.convert_labels(torch.from_numpy(labels.astype(np.int64))).numpy()
    edge = ref.edge_3d(seg)
    sdf = ref.compute_sdf(seg, seg.shape)                                # the reference's asserts run here
    sdm = 1 - sdf + edge
    out = os.path.join(HERE, "sdm_edge.npz")
    np.savez_compressed(out, labels=labels, seg=seg.astype(np.uint8), edge=edge.astype(np.uint8), sdf=sdf.astype(np.float64),
                        sdm=sdm.astype(np.float64))
    print(out, os.path.getsize(out), "bytes; shape", seg.shape, "sdm in", [float(sdm.min()), float(sdm.max())],
          "WT edge voxels", int(edge[0, 1].sum()))


if __name__ == "__main__":
    main(sys.argv[1])
