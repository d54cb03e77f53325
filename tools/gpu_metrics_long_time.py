"""Time the evaluation of volumes with sides beyond 256 (segmamba_amd.metrics on csrc/edt_long.hip: the box route, `edt_sq_long`,
`planes_bbox`).

    python tools/gpu_metrics_long_time.py [--calls 30] [--no-scipy] [--no-ct] [--out profiles/metrics_long_time.json]

(a) a synthetic CT-size case, 400 x 512 x 512 with three regions: an organ-sized ellipsoid whose box exceeds 256 on two sides, a
    small one, and one whose prediction has a far false-positive island - `case_metrics` at spacing (1, 1, 1) and (2.5, 0.8, 0.8),
    the per-kernel split of one call, the boxes and the workspace bytes; where scipy imports, the same definition with
    scipy.ndimage on one core, once, by the wall clock (unit spacing);
(b) tests/metrics_ref.brats_size_case() (155 x 240 x 240) under the default route, `SEGM_EDT_LONG=box` and `SEGM_EDT_LONG=1`.
Medians over `--calls` calls after warm-up, HIP events around whole calls, both readbacks included.  Bytes are by the algorithm's
count, not by a hardware counter: the x pass reads two border bytes and writes two planes per crop voxel, a line pass reads and
writes two planes (16 bytes per crop voxel) plus between 0 and 16 bytes per voxel and plane of stack traffic, which is NOT
counted - the rates are therefore lower bounds of what the passes move."""
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

from segmamba_amd import lib as L              # noqa: E402
from segmamba_amd import metrics as M          # noqa: E402
from tests import metrics_ref as R             # noqa: E402

CT_SHAPE = (400, 512, 512)
CT_REGIONS = ((1,), (2,), (3,))


def event_ms(fn, calls, warmup=3):
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


def _ellipsoid(shape, centre, radii, dev):
    z, y, x = [torch.arange(n, dtype=torch.float32, device=dev) for n in shape]
    d = ((z - centre[0]) / radii[0])[:, None, None] ** 2 + ((y - centre[1]) / radii[1])[None, :, None] ** 2 + \
        ((x - centre[2]) / radii[2])[None, None, :] ** 2
    return d <= 1.0


def ct_case(dev):
    """(pred, gt) uint8 on `dev`: label 1 an organ of 200 x 300 x 280, label 2 a small ellipsoid, label 3 a middle-sized one whose
    prediction has a 4^3 island in the far corner; the prediction is shifted by (2, -3, 4) and scaled 0.96"""
    def labels(shift, scale, island):
        lab = torch.zeros(CT_SHAPE, dtype=torch.uint8, device=dev)
        for value, c, r in ((1, (200, 250, 260), (100, 150, 140)), (2, (60, 80, 420), (12, 14, 10)), (3, (330, 420, 110), (30, 40, 36))):
            c = tuple(ci + s for ci, s in zip(c, shift))
            lab[_ellipsoid(CT_SHAPE, c, tuple(ri * scale for ri in r), dev)] = value
        if island:
            lab[:4, :4, -4:] = 3
        return lab
    return labels((2, -3, 4), 0.96, True), labels((0, 0, 0), 1.0, False)


def timed_case(tp, tg, spacing, regions, calls):
    def fn():
        return M.case_metrics(tp, tg, spacing, regions)
    result = fn()
    ms = event_ms(fn, calls)
    rec = {"case_metrics": result.tolist(), "ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    try:
        rec["kernels_us"] = kernel_split(fn)
    except Exception as exc:          # the split is a record, not a result: say why it is missing
        rec["kernels_us"] = f"unavailable: {type(exc).__name__}: {exc}"
    return rec


def pass_rates(rec, long_voxels, brute_voxels):
    """lower bounds of the bytes per second of the distance-transform passes and the box pass, from the split of one call"""
    split = rec.get("kernels_us")
    if not isinstance(split, dict):
        return
    counts = {"edt_long_x_kernel": 2 + 8, "edt_long_line_kernel": 2 * 16, "edt_x_kernel": 2 + 8, "edt_line_kernel": 2 * 16}
    out = {}
    for name, (cnt, us) in split.items():
        for key, per_voxel in counts.items():
            if key in name:
                b = per_voxel * (long_voxels if key.startswith("edt_long") else brute_voxels)
                out[name] = {"launches": cnt, "us_total": us, "bytes_min_by_count": b, "TB_per_s_lower_bound": b / (us * 1e-6) / 1e12}
    rec["edt_pass_rates"] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--no-ct", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_long_time.json"))
    args = ap.parse_args()
    dev = "cuda"
    os.environ.pop("SEGM_EDT_LONG", None)
    rec = {"device": torch.cuda.get_device_name(0), "calls": args.calls,
           "bytes": "by the algorithm's count (see the tool's docstring), stack traffic not counted: lower bounds"}
    if not args.no_ct:
        tp, tg = ct_case(dev)
        p = M._Pass(tp, tg, CT_REGIONS)
        boxes = [p.boxes[r] for r in range(3)]
        crops = [[b[1] - b[0], b[3] - b[2], b[5] - b[4]] for b in boxes]
        long_voxels = sum(c[0] * c[1] * c[2] for c in crops if max(c) > L.EDT_MAX_LINE)      # crops that take edt_sq_long
        brute_voxels = sum(c[0] * c[1] * c[2] for c in crops if max(c) <= L.EDT_MAX_LINE)
        lib = L.get_lib()
        ct = {"case": "400 x 512 x 512, regions (1,), (2,), (3,): tools/gpu_metrics_long_time.ct_case", "boxes": boxes, "crops": crops,
              "border_counts": [p.counts[3][:3], p.counts[4][:3]],
              "workspace_bytes_whole_volume_2_planes": lib.dll.segm_edt_sq_long_workspace_bytes(*CT_SHAPE, 2, 0),
              "workspace_bytes_per_crop": [lib.dll.segm_edt_sq_long_workspace_bytes(*c, 2, 0) for c in crops]}
        for key, sp in (("unit", (1, 1, 1)), ("aniso", (2.5, 0.8, 0.8))):
            ct[key] = timed_case(tp, tg, sp, CT_REGIONS, args.calls)
            ct[key]["spacing"] = list(sp)
            pass_rates(ct[key], long_voxels, brute_voxels)
        borders = p.borders
        items = [(0, r, 1, r) for r in range(3)]
        from segmamba_amd import ops_raw
        ms = event_ms(lambda: ops_raw.planes_bbox(lib, borders, items), args.calls)
        nbytes = 2 * borders[0].numel()
        ct["planes_bbox"] = {"ms_median": statistics.median(ms), "bytes_by_count": nbytes,
                             "TB_per_s": nbytes / (statistics.median(ms) * 1e-3) / 1e12}
        if not args.no_scipy:
            try:
                import scipy.ndimage  # noqa: F401
                hp, hg = tp.cpu().numpy(), tg.cpu().numpy()
                t0 = time.perf_counter()
                ref = np.zeros((3, 2))
                for r, reg in enumerate(CT_REGIONS):
                    a, b = R.region_mask(hp, reg), R.region_mask(hg, reg)
                    ref[r] = (R.dc(a, b), R.scipy_hd95(a, b))
                ct["scipy_host_s"] = time.perf_counter() - t0
                ct["scipy_case_metrics"] = ref.tolist()
                ct["host_cpus_used"] = 1
            except ImportError:
                ct["scipy_host_s"] = None
        rec["ct_size_case"] = ct
        del tp, tg, p, borders
    pred, gt = R.brats_size_case()
    tp, tg = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    brats = {"case": "tests/metrics_ref.brats_size_case: 155 x 240 x 240, regions TC / WT / ET, spacing (1, 1, 1)"}
    for key, mode in (("default", None), ("box", "box"), ("long", "1")):
        if mode is None:
            os.environ.pop("SEGM_EDT_LONG", None)
        else:
            os.environ["SEGM_EDT_LONG"] = mode
        brats[key] = timed_case(tp, tg, (1, 1, 1), R.BRATS_REGIONS, args.calls)
    os.environ["SEGM_EDT_LONG"] = "box"
    p = M._Pass(tp, tg, R.BRATS_REGIONS)
    os.environ.pop("SEGM_EDT_LONG", None)
    brats["boxes"] = [p.boxes[r] for r in range(3)]
    rec["brats_size_case"] = brats
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
