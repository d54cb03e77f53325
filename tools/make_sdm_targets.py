"""Write the `<case>_seg_sdm.npy` files that the reference's dataset_sdm_edge.py loads (its ./data/fullres/train_sdm), on the device.

    python tools/make_sdm_targets.py --data DIR --out DIR [--float64] [--device cuda]

For every case of --data - a `<case>_seg.npy` as the reference's `unpack_dataset` leaves it, taken when present, else the `seg` of
`<case>.npz` - the file holds `seg_sdm = 1 - compute_sdf(seg) + seg_edge` of `seg = convert_labels(labels)` (TC, WT, ET) with shape
(1, 3, X, Y, Z), the layout `MedicalDataset.__getitem__` indexes with `[0]`; `segmamba_amd.dataloading.CaseDataset(sdm_dir=...)` reads
it the same way.  float32 as the kernels write it; --float64 widens on the host to the reference's dtype.  No scipy, no skimage:
segmamba_amd.sdm.sdm_edge_targets.  The seg's first channel is the label volume; its -1 ("outside the brain") is in no region."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402


def case_labels(data_dir: str):
    """-> [(case, loader of its (X, Y, Z) label volume)], sorted by case"""
    cases = {}
    for n in sorted(os.listdir(data_dir)):
        if n.endswith("_seg.npy"):
            cases[n[:-len("_seg.npy")]] = os.path.join(data_dir, n)
        elif n.endswith(".npz"):
            cases.setdefault(n[:-4], os.path.join(data_dir, n))
    if not cases:
        raise RuntimeError(f"{data_dir} holds no <case>.npz and no <case>_seg.npy")

    def load(path):
        if path.endswith(".npy"):
            seg = np.load(path)
        else:
            with np.load(path) as z:
                seg = z["seg"]
        seg = np.asarray(seg)
        if seg.ndim == 4:
            seg = seg[0]
        if seg.ndim != 3:
            raise RuntimeError(f"{path}: a (1, X, Y, Z) or (X, Y, Z) seg is required, got shape {seg.shape}")
        return np.ascontiguousarray(seg.astype(np.int16))
    return [(c, (lambda p=p: load(p))) for c, p in sorted(cases.items())]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data", required=True, help="folder of <case>.npz / <case>_seg.npy")
    ap.add_argument("--out", required=True, help="folder for <case>_seg_sdm.npy")
    ap.add_argument("--float64", action="store_true", help="widen to the reference's float64 on the host")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    import torch
    from segmamba_amd.sdm import sdm_edge_targets
    os.makedirs(args.out, exist_ok=True)
    written = []
    for case, load in case_labels(args.data):
        labels = torch.from_numpy(load()).to(args.device)
        _, sdm = sdm_edge_targets(labels)                                  # (1, 3, X, Y, Z)
        a = sdm.cpu().numpy()
        path = os.path.join(args.out, f"{case}_seg_sdm.npy")
        np.save(path, a.astype(np.float64) if args.float64 else a)
        written.append(path)
        print(f"{case}: {tuple(a.shape)} -> {path}")
    return written


if __name__ == "__main__":
    main()
