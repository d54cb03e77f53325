"""Prepare raw cases for training and prediction on the device: the reference's 2_preprocessing_mri.py.

    python tools/preprocess_cases.py --raw DIR --out DIR [--data-files t1.nii.gz t1ce.nii.gz ...] [--seg-file seg.nii.gz] [--mask-norm] [--resample]
                                    [--separate-z {never,auto,always}]
    python tools/preprocess_cases.py --raw DIR --out DIR --ct --plan FILE [--label-dir NAME] [--labels 1 2] [--spacing z y x]

`--raw` holds one directory per case, each with one NIfTI file per modality and, for training data, the segmentation.  Every case
becomes `<case>.npz` (data, seg) and `<case>.pkl` (properties) in `--out`: what `segmamba_amd.dataloading.CaseDataset` and the
reference's `MedicalDataset` read.  `--seg-file ""` prepares unlabelled cases.  `--resample` resamples cases whose spacing is not
`--spacing` (without it such a case is an error); `--separate-z` is the reference's `force_separate_z` for that step (never = False,
the default: one 3-D zoom; auto = None: slice by slice across the one coarse axis of an anisotropic spacing; always = True).  See segmamba_amd/preprocess.py for the stated limits.

`--ct` prepares CT cases the way of the reference's DefaultPreprocessor: `--raw` holds one NIfTI file per case, `--label-dir` names the
directory beside it with the segmentations under the same file names (none: unlabelled cases), `--plan` is the file
`tools/plan_cases.py` wrote.  The cases are clipped and normalised with the plan's foreground statistics and resampled to the plan's
`fullres spacing` unless `--spacing` (z, y, x) is given.  (`--labels` keeps its meaning, the label values to draw class locations for;
the label directory therefore has its own option.)
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmamba_amd.preprocess import CasePreprocessor, CTCasePreprocessor      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--data-files", nargs="+", default=["t2w.nii.gz", "t2f.nii.gz", "t1n.nii.gz", "t1c.nii.gz"],
                    help="the modalities' file names inside a case directory (default: the reference's BraTS2023 names)")
    ap.add_argument("--seg-file", default="seg.nii.gz", help='the segmentation\'s file name; "" for unlabelled cases')
    ap.add_argument("--spacing", nargs=3, type=float, default=None, help="default 1 1 1; with --ct the plan's fullres spacing")
    ap.add_argument("--labels", nargs="+", type=int, default=[1, 2, 3])
    ap.add_argument("--mask-norm", action="store_true", help="z-score over seg >= 0 only (use_mask_for_norm)")
    ap.add_argument("--resample", action="store_true", help="resample to --spacing (data order 3, seg order 1)")
    ap.add_argument("--separate-z", choices=["never", "auto", "always"], default="never",
                    help="resample across one coarse axis slice by slice, nearest slice along it (force_separate_z False / None / True)")
    ap.add_argument("--ct", action="store_true", help="CT cases: one file per case, CT normalisation from --plan, resampled")
    ap.add_argument("--plan", default=None, help="with --ct: the JSON tools/plan_cases.py wrote")
    ap.add_argument("--label-dir", default=None, help="with --ct: the directory beside --raw that holds the segmentations")
    args = ap.parse_args()
    raw = os.path.abspath(args.raw)
    force_separate_z = {"never": False, "auto": None, "always": True}[args.separate_z]
    if args.ct:
        if args.plan is None:
            ap.error("--ct needs --plan FILE (tools/plan_cases.py)")
        import json
        with open(args.plan) as f:
            plan = json.load(f)
        spacing = args.spacing if args.spacing is not None else plan["fullres spacing"][::-1]
        pre = CTCasePreprocessor(os.path.dirname(raw), os.path.basename(raw), args.label_dir, force_separate_z=force_separate_z)
        t0 = time.perf_counter()
        written = pre.run([int(s) if s == int(s) else s for s in spacing], args.out, list(args.labels),
                          plan["intensity_statistics_per_channel"])
        print(f"{len(written)} CT cases -> {args.out} in {time.perf_counter() - t0:.1f} s")
        return
    if args.plan is not None or args.label_dir is not None:
        ap.error("--plan and --label-dir belong to --ct")
    if args.spacing is None:
        args.spacing = [1.0, 1.0, 1.0]
    pre = CasePreprocessor(os.path.dirname(raw), os.path.basename(raw), args.data_files, args.seg_file, use_mask_for_norm=args.mask_norm,
                           resample=args.resample, force_separate_z=force_separate_z)
    t0 = time.perf_counter()
    spacing = [int(s) if s == int(s) else s for s in args.spacing]
    written = pre.run(spacing, args.out, list(args.labels))
    print(f"{len(written)} cases -> {args.out} in {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
