"""Time the case-preparation stage (segmamba_amd/preprocess.py, segmamba_amd/dataloading.py) at BraTS size, 155 x 240 x 240 x 4.

    python tools/gpu_preprocess_time.py [--calls 30] [--no-host] [--out profiles/preprocess_time.json]

(a) `preprocess_case` as a whole - readbacks and the drawing of the class locations included - and its parts: mask + box, the hole
    filling (nine launches), the statistics (four launches), the crop / normalise / relabel launch; each with the bytes it moves by the
    algorithm's count and the resulting TB/s;
(b) the numpy / scipy restatement (tests/preprocess_ref.py) of the same case on one host core, the fill apart;
(c) `PatchLoader.next()` at the reference's 128^3 patch and batch 2 from a resident case, with and without augmentation.
HIP events around whole calls, the median over `--calls` calls after warm-up; the host restatement by the wall clock."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from segmamba_amd import lib as L                       # noqa: E402
from segmamba_amd import ops_raw                        # noqa: E402
from segmamba_amd import postprocess as PP              # noqa: E402
from segmamba_amd import preprocess as P                # noqa: E402
from segmamba_amd.dataloading import PatchLoader        # noqa: E402
from tests import preprocess_ref as R                   # noqa: E402
from tools.gpu_metrics_time import event_ms, kernel_split      # noqa: E402


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def with_rate(ms, nbytes):
    out = stats(ms)
    out["bytes_by_count"] = int(nbytes)
    out["TB_per_s"] = nbytes / (out["ms_median"] * 1e-3) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "preprocess_time.json"))
    args = ap.parse_args()
    lib = L.get_lib()
    data, seg, _ = R.brats_case()
    C, (D, H, W) = data.shape[0], data.shape[1:]
    n = D * H * W
    td, ts = torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda()
    props = {"spacing": (1.0, 1.0, 1.0)}
    out, sout = P.preprocess_case(td, ts, props)
    bb = props["bbox_used_for_cropping"]
    start, shape = [b[0] for b in bb], [b[1] - b[0] for b in bb]
    nb = int(np.prod(shape))
    # what the box kernels touch: whole 16-byte packets of every box row
    nbp = shape[0] * shape[1] * 4 * ((bb[2][1] + 3) // 4 - bb[2][0] // 4)
    rec = {"case": "tests/preprocess_ref.brats_case: 4 x 155 x 240 x 240 fp32, seg fp32", "device": torch.cuda.get_device_name(0),
           "calls": args.calls, "box": bb, "crop_voxels": nb}
    mask, _ = ops_raw.nonzero_mask_bbox(lib, td)
    filled = PP._fill(lib, mask)
    _, s32 = ops_raw.crop_stats(lib, td, start, shape)
    rec["preprocess_case"] = stats(event_ms(lambda: P.preprocess_case(td, ts, {"spacing": (1.0, 1.0, 1.0)}), args.calls))
    rec["preprocess_case_mask_norm"] = stats(event_ms(lambda: P.preprocess_case(td, ts, {"spacing": (1.0, 1.0, 1.0)}, use_mask_for_norm=True),
                                                      args.calls))
    rec["preprocess_case_without_seg"] = stats(event_ms(lambda: P.preprocess_case(td, None, {"spacing": (1.0, 1.0, 1.0)}), args.calls))
    rec["parts"] = {
        "mask_and_box": with_rate(event_ms(lambda: ops_raw.nonzero_mask_bbox(lib, td), args.calls), 4 * C * n + n),
        "fill_nine_launches": stats(event_ms(lambda: PP._fill(lib, mask), args.calls)),
        "statistics_two_passes": with_rate(event_ms(lambda: ops_raw.crop_stats(lib, td, start, shape), args.calls), 2 * 4 * C * nbp),
        "statistics_two_passes_masked": with_rate(event_ms(lambda: ops_raw.crop_stats(lib, td, start, shape, mask=filled, seg=ts[0], masked=True),
                                                           args.calls), 2 * (4 * C + 4 + 1) * nbp),
        "crop_normalise_relabel": with_rate(event_ms(lambda: ops_raw.crop_normalize(lib, td, s32, start, shape, mask=filled, seg=ts[0]),
                                                     args.calls), (4 * C + 4 + 1) * nbp + (4 * C + 2) * nb),
        "class_locations": stats(event_ms(lambda: P.sample_foreground_locations(sout, (1, 2, 3)), args.calls)),
    }
    try:
        split = kernel_split(lambda: P.preprocess_case(td, ts, {"spacing": (1.0, 1.0, 1.0)}))
        rec["kernels"] = {k: {"calls": c, "us_per_call": us / c} for k, (c, us) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"

    if not args.no_host:
        t0 = time.perf_counter()
        raw = R.nonzero_mask(data)
        t1 = time.perf_counter()
        R.fill(raw)
        t2 = time.perf_counter()
        R.run_case(data, seg, (1.0, 1.0, 1.0))
        t3 = time.perf_counter()
        rec["host_restatement"] = {"mask_s": t1 - t0, "fill_s": t2 - t1, "run_case_with_fill_s": t3 - t2, "host_cpus_used": 1,
                                   "note": "numpy / scipy on one core; run_case normalises in float64"}

    class Resident:                       # one preprocessed case, as CaseDataset keeps it
        device = td.device

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"data": out, "seg": sout, "properties": props}
    np.random.seed(0)
    plain = PatchLoader(Resident(), (128, 128, 128), batch_size=2)
    aug = PatchLoader(Resident(), (128, 128, 128), batch_size=2, augment=True)
    rec["patch_loader_next"] = {"patch": [128, 128, 128], "batch": 2,
                                "plain": with_rate(event_ms(plain.next, args.calls), 2 * 2 * (4 * C + 1) * 128 ** 3 + 2 * 12 * 128 ** 3),
                                "augmented": stats(event_ms(aug.next, args.calls))}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
