"""Dice and HD95 per BraTS region (TC / WT / ET) of predicted label volumes against ground truth, on the device: the command-line
form of the reference's 5_compute_metrics.py.

    python tools/compute_metrics.py --pred DIR --gt DIR [--out FILE.npy] [--spacing Z Y X] [--labels 1,2,...]
                                    [--report FILE.json [--tolerance T]]

--labels scores one region per listed label (e.g. the nine organs of a CT label map) instead of the BraTS regions; any number of them.
--report also writes the metric table of the reference's light_training/evaluation/metric.py (its 19 entries and the voxel-counted
"Surface Dice" at --tolerance, default 1.0; segmamba_amd.metrics.case_report) per case and on average over the cases that have a
value, as JSON: {"regions", "tolerance", "cases": {name: {metric: [per region]}}, "mean": {metric: [per region]}}, null for NaN.

Cases are the files of --pred that have a file of the same name in --gt.  Label volumes are read from .npy and .npz (the first
array, or the one called "labels" / "seg" / "arr_0"); .nii / .nii.gz through nibabel or SimpleITK where one is installed, else through
segmamba_amd.nifti.read_nifti (single-file NIfTI-1 as tools/finish_predictions.py and Predictor.save_to_nii write it).  Prints the
per-case array, then its mean and standard deviation over the cases, and saves the (cases, regions, 2) array to --out.

Volumes may measure up to 2048 voxels per side (CT cases of 512 x 512 x several hundred included): a volume with a side beyond 256 is
scored on the crops to each region's border box, by the linear-time distance transform where a crop is still longer than 256."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402

EXTS = (".npy", ".npz", ".nii.gz", ".nii")


def load_labels(path: str) -> np.ndarray:
    if path.endswith(".npy"):
        a = np.load(path)
    elif path.endswith(".npz"):
        with np.load(path) as z:
            name = next((k for k in ("labels", "seg", "arr_0") if k in z.files), z.files[0])
            a = z[name]
    else:
        try:
            import nibabel
            a = np.asarray(nibabel.load(path).dataobj).transpose(2, 1, 0)          # (x, y, z) on disk -> (z, y, x)
        except ImportError:
            try:
                import SimpleITK as sitk
                a = sitk.GetArrayFromImage(sitk.ReadImage(path))
            except ImportError:
                from segmamba_amd.nifti import read_nifti
                a = read_nifti(path)[0]                                                # the library's own reader: (z, y, x)
    a = np.squeeze(np.asarray(a))
    if a.ndim != 3:
        raise RuntimeError(f"{path}: a 3-D label volume is required, got shape {a.shape}")
    if a.min() < 0 or a.max() > 255:
        raise RuntimeError(f"{path}: labels must lie in [0, 255]")
    return np.ascontiguousarray(a.astype(np.uint8))


def case_files(pred_dir: str, gt_dir: str):
    names = sorted(n for n in os.listdir(pred_dir) if n.endswith(EXTS) and os.path.exists(os.path.join(gt_dir, n)))
    if not names:
        raise RuntimeError(f"no file of {pred_dir} ({', '.join(EXTS)}) has a file of the same name in {gt_dir}")
    return names


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0] + "  " + __doc__.split("\n\n")[-1].replace("\n", " "))
    ap.add_argument("--pred", required=True)
    ap.add_argument("--gt", required=True)
    ap.add_argument("--out")
    ap.add_argument("--spacing", type=float, nargs=3, default=(1.0, 1.0, 1.0), metavar=("Z", "Y", "X"))
    ap.add_argument("--labels", default=None, help="comma-separated labels: one region per label instead of the BraTS regions")
    ap.add_argument("--report", default=None, metavar="FILE.json", help="also write the full metric table per case and on average")
    ap.add_argument("--tolerance", type=float, default=1.0, help="the tolerance of the report's Surface Dice, in the unit of --spacing")
    args = ap.parse_args(argv)
    from segmamba_amd import metrics
    regions = metrics.BRATS_REGIONS
    if args.labels is not None:
        regions = tuple((int(v),) for v in args.labels.split(",") if v.strip())
        if not regions or any(not 1 <= r[0] <= 255 for r in regions):
            raise RuntimeError(f"--labels: labels in 1 .. 255 are required, got {args.labels!r}")
    names = case_files(args.pred, args.gt)

    def cases():
        for n in names:
            yield load_labels(os.path.join(args.pred, n)), load_labels(os.path.join(args.gt, n)), tuple(args.spacing)
    results, mean, std = metrics.evaluate(cases(), regions, max_regions=None)
    for n, r in zip(names, results):
        print(n, r.tolist())
    print(results.shape)
    print(mean)
    print(std)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        np.save(args.out, results)
    if args.report:
        import json
        per_case, mean = metrics.evaluate_report(cases(), regions, tolerance=args.tolerance)

        def plain(a):
            return [None if np.isnan(v) else float(v) for v in a]
        rec = {"regions": [list(r) for r in regions], "tolerance": args.tolerance, "spacing": list(args.spacing),
               "cases": {n: {m: plain(a[i]) for m, a in per_case.items()} for i, n in enumerate(names)},
               "mean": {m: plain(a) for m, a in mean.items()}}
        os.makedirs(os.path.dirname(os.path.abspath(args.report)), exist_ok=True)
        with open(args.report, "w") as f:
            json.dump(rec, f, indent=1)
    return results


if __name__ == "__main__":
    main()
