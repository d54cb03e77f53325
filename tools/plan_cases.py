"""Fingerprint a CT dataset on the device: the `run_plan` step of the reference's CT examples (2_preprocessing_*.py on DefaultPreprocessor).

    python tools/plan_cases.py --base DIR --images NAME --labels NAME [--out FILE]

`DIR/NAME` of `--images` holds one NIfTI file per case, `DIR/NAME` of `--labels` its segmentation under the same file name.  Per case
10 000 foreground intensities are drawn (`segmamba_amd.preprocess.collect_foreground_intensities`); over the dataset the plan holds
their statistics per channel, the target spacing, the median shape after resampling and the initial patch size, written as the
reference's JSON to `--out` (default ./data_analysis_result.txt) - what `tools/preprocess_cases.py --ct --plan FILE` reads.  The key
`target medium patch size` (network planning) is left out.  See segmamba_amd/preprocess.py for the stated limits.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmamba_amd.preprocess import CTCasePreprocessor      # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--base", required=True)
    ap.add_argument("--images", required=True)
    ap.add_argument("--labels", required=True)
    ap.add_argument("--out", default="./data_analysis_result.txt")
    args = ap.parse_args()
    pre = CTCasePreprocessor(os.path.abspath(args.base), args.images, args.labels)
    t0 = time.perf_counter()
    plan = pre.run_plan(args.out)
    print(json.dumps(plan))
    print(f"{len(pre.get_iterable_list())} cases -> {args.out} in {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
