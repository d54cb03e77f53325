"""Time the selection route of the evaluation report against the list route of `case_metrics`, on the case at BraTS size of
tests/test_gpu_metrics.py (155 x 240 x 240, three regions).

    python tools/gpu_surface_time.py [--calls 30] [--out profiles/surface_time.json]

(a) `case_report(metrics=["Dice", "Hausdorff Distance 95"])` (segm_border_stats: counts and radix selection) against `case_metrics`
    (segm_border_distances, one torch.sort per region), the two alternating call by call in one run: medians over `--calls` calls after
    warm-up, HIP events around the whole call, both readbacks included.  The outputs are asserted equal bit for bit.
(b) the full 20-entry report, timed the same way.
(c) in a profiler run of its own (torch.profiler's device activity, one call each): the per-kernel split of both routes, the number of
    launches of each, and the bytes per second of segm_border_stats' passes from the algorithm's count - per pass and item the item's
    border volume once, plus 4 bytes of `edt` per set voxel."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from segmamba_amd import metrics as M          # noqa: E402
from tests import metrics_ref as R             # noqa: E402

PAIR = ["Dice", "Hausdorff Distance 95"]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def kernel_split(fn):
    """{kernel name: [calls, total microseconds]} of one call"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {}
    for e in prof.key_averages():
        dev_us = getattr(e, "device_time_total", None)
        if dev_us is None:
            dev_us = getattr(e, "cuda_time_total", 0.0)
        if dev_us and str(getattr(e, "device_type", "")).endswith("CUDA"):
            split[e.key] = [int(e.count), float(dev_us)]
    return split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "surface_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_surface_time.py needs a GPU: nothing is measured without one")
    pred, gt = R.brats_size_case()
    tp, tg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    routes = {"case_metrics": lambda: M.case_metrics(tp, tg),
              "case_report_dice_hd95": lambda: M.case_report(tp, tg, metrics=PAIR),
              "case_report_full": lambda: M.case_report(tp, tg)}
    for _ in range(args.warmup):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in routes}
    for _ in range(args.calls):                       # alternating call by call
        for k, fn in routes.items():
            t, out = event_ms(fn)
            ms[k].append(t)
            if k == "case_metrics":
                cm = out
            elif k == "case_report_dice_hd95":
                assert np.array_equal(np.stack([out[m] for m in PAIR], axis=1).view(np.int64), cm.view(np.int64)), (out, cm)
    full = routes["case_report_full"]()
    rec = {"case": "tests/metrics_ref.brats_size_case: 155 x 240 x 240, regions TC / WT / ET, spacing (1, 1, 1)",
           "device": torch.cuda.get_device_name(0), "calls": args.calls, "outputs_equal_bit_for_bit": True,
           "case_metrics": cm.tolist(), "case_report_full": {m: v.tolist() for m, v in full.items()}}
    for k, v in ms.items():
        rec[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    try:
        n = pred.size
        borders = int(sum(R.counts(pred, gt)[3:].sum(axis=0)))
        for k in ("case_metrics", "case_report_dice_hd95"):
            split = kernel_split(routes[k])
            rec[k + "_kernels_us"] = split
            rec[k + "_launches"] = int(sum(c for c, _ in split.values()))
        passes = {name: v for name, v in rec["case_report_dice_hd95_kernels_us"].items() if "bstat_pass_kernel" in name}
        nbytes = 6 * n + 4 * borders                  # one pass: six items read their border volume, edt at the set voxels
        for name, (cnt, us) in passes.items():
            rec["bstat_pass_bytes_per_s"] = {"calls": cnt, "us_per_call": us / cnt, "bytes_per_call": nbytes,
                                             "TB_per_s": nbytes / (us / cnt * 1e-6) / 1e12}
    except Exception as exc:          # the split is a record, not a result: say why it is missing
        rec["kernels_us"] = f"unavailable: {type(exc).__name__}: {exc}"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
