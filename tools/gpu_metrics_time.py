"""Time `segmamba_amd.metrics.case_metrics` on the case at BraTS size of tests/test_gpu_metrics.py (155 x 240 x 240, three regions).

    python tools/gpu_metrics_time.py [--calls 30] [--no-scipy] [--out profiles/metrics_time.json]

(a) the whole call on the device - median over `--calls` calls after warm-up, HIP events around the call, both readbacks included - and
    the per-kernel split of one call (torch.profiler's device activity);
(b) where scipy imports: the same definition with scipy.ndimage on the host, once.
Also the bytes per second of the three distance-transform passes (x: reads the two border volumes, writes six planes; y and z: read and
write six planes)."""
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

from segmamba_amd import metrics as M          # noqa: E402
from tests import metrics_ref as R             # noqa: E402


def event_ms(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


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
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time.json"))
    args = ap.parse_args()
    pred, gt = R.brats_size_case()
    tp, tg = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    result = M.case_metrics(tp, tg)
    ms = event_ms(lambda: M.case_metrics(tp, tg), args.calls)
    t0 = time.perf_counter()
    for _ in range(args.calls):
        M.case_metrics(tp, tg)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / args.calls
    rec = {"case": "tests/metrics_ref.brats_size_case: 155 x 240 x 240, regions TC / WT / ET, spacing (1, 1, 1)",
           "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "case_metrics": result.tolist(),
           "case_metrics_ms_median": statistics.median(ms), "case_metrics_ms_min": min(ms), "case_metrics_ms_max": max(ms),
           "case_metrics_wall_ms_mean": wall_ms}
    try:
        split = kernel_split(lambda: M.case_metrics(tp, tg))
        rec["kernels_us"] = split
        n = pred.size
        nbytes = {"edt_x_kernel": 2 * n + 6 * n * 4, "edt_line_kernel": 2 * 6 * n * 4}
        for name, (cnt, us) in split.items():
            for key, b in nbytes.items():
                if key in name:
                    rec.setdefault("edt_pass_bytes_per_s", {})[name] = {"calls": cnt, "us_per_call": us / cnt, "bytes_per_call": b,
                                                                        "TB_per_s": b / (us / cnt * 1e-6) / 1e12}
    except Exception as exc:          # the split is a record, not a result: say why it is missing
        rec["kernels_us"] = f"unavailable: {type(exc).__name__}: {exc}"
    if not args.no_scipy:
        try:
            import scipy.ndimage  # noqa: F401
            t0 = time.perf_counter()
            ref = np.zeros((3, 2))
            for r, reg in enumerate(R.BRATS_REGIONS):
                a, b = R.region_mask(pred, reg), R.region_mask(gt, reg)
                ref[r] = (R.dc(a, b), R.scipy_hd95(a, b))
            rec["scipy_host_s"] = time.perf_counter() - t0
            rec["scipy_case_metrics"] = ref.tolist()
            rec["host_cpus_used"] = 1
        except ImportError:
            rec["scipy_host_s"] = None
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
