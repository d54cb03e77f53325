"""Generate tests/golden/eval_report.npz by running the REFERENCE's own metric table.

    python tests/golden/make_golden_eval_report.py <path of the reference checkout>

`light_training/evaluation/metric.py` needs numpy and `medpy.metric`, of which it calls `hd`, `hd95`, `asd` and `assd`.  medpy is not
a dependency of this repository: a module of that name is put in front of the import that forwards the four calls to the numpy
restatement of medpy's definitions in tests/surface_ref.py (brute-force distances, connectivity 1).  Everything else - the
`ConfusionMatrix`, the 19 functions of `ALL_METRICS`, their names and their rules for masks that are empty or full - is the
reference's code, imported from the checkout at generation time and run as it is.  Recorded: per case of
tests/surface_ref.golden_cases (inputs are generator arguments, not volumes), per BraTS region and per name the value with
nan_for_nonexisting True and False; the names in the reference's order.  The fixture holds numbers and names only; no reference code
goes into this repository.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def main(reference: str):
    from tests import metrics_ref as R
    from tests import surface_ref as S
    medpy, metric = types.ModuleType("medpy"), types.ModuleType("medpy.metric")
    for name in ("hd", "hd95", "asd", "assd"):
        setattr(metric, name, getattr(S, name))
    medpy.metric = metric
    sys.modules["medpy"], sys.modules["medpy.metric"] = medpy, metric
    sys.path.insert(0, reference)
    from light_training.evaluation import metric as ref
    names = list(ref.ALL_METRICS)
    cases = S.golden_cases()
    values = np.zeros((2, len(cases), len(R.BRATS_REGIONS), len(names)), dtype=np.float64)
    for k, nan in enumerate((True, False)):
        for c, (_, pred, gt, spacing) in enumerate(cases):
            for r, reg in enumerate(R.BRATS_REGIONS):
                p, g = R.region_mask(pred, reg), R.region_mask(gt, reg)
                cm = ref.ConfusionMatrix(p, g)
                for m, name in enumerate(names):
                    values[k, c, r, m] = ref.ALL_METRICS[name](p, g, cm, nan_for_nonexisting=nan, voxel_spacing=spacing)
    out = os.path.join(HERE, "eval_report.npz")
    np.savez_compressed(out, names=np.array(names), cases=np.array([c[0] for c in cases]), values=values)
    print(out, os.path.getsize(out), "bytes;", len(cases), "cases x 3 regions x", len(names), "names")


if __name__ == "__main__":
    main(sys.argv[1])
