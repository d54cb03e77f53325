"""Logits to label volumes on the device: the command-line form of the reference's steps between `maybe_mirror_and_predict` and the
file on disk (4_predict.py:75-99).

    python tools/finish_predictions.py --logits DIR --out DIR [--postprocess | --per-class] [--connectivity {1,2,3}]
                                       [--organs NAME,NAME,...] [--spacing X Y Z]

Every .npy / .npz of --logits holds the (C, d, h, w) logits of one case (.npz: the array called "logits" / "arr_0", or the first one).
A .npz may also carry the reference loader's properties as arrays of the same names (`shape_after_cropping_before_resample`,
`bbox_used_for_cropping`, `shape_before_cropping`, and `spacing` for the header); without them the labels have the logits' shape.
Writes <case>.nii.gz label volumes that tools/compute_metrics.py reads.  --postprocess keeps, per BraTS region, the largest component
with its holes filled (segmamba_amd.postprocess.postprocess_labels).  --per-class keeps the largest component of every class of the
label map (segmamba_amd.postprocess.keep_largest_per_class: one labelled pass for all classes).  --connectivity is that of the
components of both (1: faces, the default and the reference's; 2: faces and edges; 3: faces, edges and corners, nnU-Net's).
--organs also writes <out>/<case>/<NAME>.nii.gz = `labels == i` for the i-th name (1-based) of the label map as written (the loop of
the reference's light_training/examples/AbdomenAtlas1.0Mini/4_predict_diffunet.py:97-109)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402

PROPS = ("shape_after_cropping_before_resample", "bbox_used_for_cropping", "shape_before_cropping")


def load_case(path: str):
    """-> (logits, properties or None, spacing or None)"""
    if path.endswith(".npy"):
        return np.load(path), None, None
    with np.load(path) as z:
        name = next((k for k in ("logits", "arr_0") if k in z.files), z.files[0])
        logits = z[name]
        have = [k for k in PROPS if k in z.files]
        if have and len(have) != len(PROPS):
            raise RuntimeError(f"{path}: properties need all of {PROPS}, found {have}")
        props = {k: z[k].tolist() for k in PROPS} if have else None
        spacing = z["spacing"].tolist() if "spacing" in z.files else None
    return logits, props, spacing


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--logits", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--postprocess", action="store_true")
    ap.add_argument("--per-class", action="store_true", help="keep the largest component of every class")
    ap.add_argument("--connectivity", type=int, choices=(1, 2, 3), default=1,
                    help="of the components of --postprocess / --per-class: 6, 18 or 26 neighbours")
    ap.add_argument("--organs", default=None, help="comma-separated organ names for labels 1, 2, ...: one file per organ and case")
    ap.add_argument("--spacing", type=float, nargs=3, default=None, metavar=("X", "Y", "Z"))
    args = ap.parse_args(argv)
    if args.postprocess and args.per_class:
        raise RuntimeError("--postprocess (per BraTS region) and --per-class exclude each other")
    organs = None if args.organs is None else [v.strip() for v in args.organs.split(",") if v.strip()]
    from segmamba_amd import nifti, postprocess
    from segmamba_amd.predictor import Predictor
    names = sorted(n for n in os.listdir(args.logits) if n.endswith((".npy", ".npz")))
    if not names:
        raise RuntimeError(f"no .npy / .npz file in {args.logits}")
    os.makedirs(args.out, exist_ok=True)
    written = []
    for n in names:
        logits, props, spacing = load_case(os.path.join(args.logits, n))
        if logits.ndim != 4:
            raise RuntimeError(f"{n}: (C, d, h, w) logits are required, got shape {logits.shape}")
        labels = postprocess.labels_from_logits(np.ascontiguousarray(logits, dtype=np.float32), props)
        if args.postprocess:
            labels = postprocess.postprocess_labels(labels, connectivity=args.connectivity)
        if args.per_class:
            labels = postprocess.keep_largest_per_class(labels, connectivity=args.connectivity)
        path = os.path.join(args.out, n[:-4] + ".nii.gz")
        nifti.write_nifti(path, labels.cpu().numpy(), args.spacing or spacing or (1.0, 1.0, 1.0))
        print(path, tuple(labels.shape))
        written.append(path)
        if organs is not None:
            written += Predictor(None).save_organs_to_nii(labels, args.spacing or spacing or (1.0, 1.0, 1.0),
                                                          os.path.join(args.out, n[:-4]), organs)
    return written


if __name__ == "__main__":
    main()
