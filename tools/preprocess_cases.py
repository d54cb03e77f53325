"""Prepare raw cases for training and prediction on the device: the reference's 2_preprocessing_mri.py.

    python tools/preprocess_cases.py --raw DIR --out DIR [--data-files t1.nii.gz t1ce.nii.gz ...] [--seg-file seg.nii.gz] [--mask-norm] [--resample]

`--raw` holds one directory per case, each with one NIfTI file per modality and, for training data, the segmentation.  Every case
becomes `<case>.npz` (data, seg) and `<case>.pkl` (properties) in `--out`: what `segmamba_amd.dataloading.CaseDataset` and the
reference's `MedicalDataset` read.  `--seg-file ""` prepares unlabelled cases.  `--resample` resamples cases whose spacing is not
`--spacing` (without it such a case is an error).  See segmamba_amd/preprocess.py for the stated limits.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmamba_amd.preprocess import CasePreprocessor      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--raw", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--data-files", nargs="+", default=["t2w.nii.gz", "t2f.nii.gz", "t1n.nii.gz", "t1c.nii.gz"],
                    help="the modalities' file names inside a case directory (default: the reference's BraTS2023 names)")
    ap.add_argument("--seg-file", default="seg.nii.gz", help='the segmentation\'s file name; "" for unlabelled cases')
    ap.add_argument("--spacing", nargs=3, type=float, default=[1.0, 1.0, 1.0])
    ap.add_argument("--labels", nargs="+", type=int, default=[1, 2, 3])
    ap.add_argument("--mask-norm", action="store_true", help="z-score over seg >= 0 only (use_mask_for_norm)")
    ap.add_argument("--resample", action="store_true", help="resample to --spacing (data order 3, seg order 1)")
    args = ap.parse_args()
    raw = os.path.abspath(args.raw)
    pre = CasePreprocessor(os.path.dirname(raw), os.path.basename(raw), args.data_files, args.seg_file, use_mask_for_norm=args.mask_norm,
                           resample=args.resample)
    t0 = time.perf_counter()
    spacing = [int(s) if s == int(s) else s for s in args.spacing]
    written = pre.run(spacing, args.out, list(args.labels))
    print(f"{len(written)} cases -> {args.out} in {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
