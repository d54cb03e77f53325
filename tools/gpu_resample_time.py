"""Time the resampling stage (segmamba_amd/resample.py on csrc/resample.hip) on a 4 x 155 x 240 x 240 crop with its int16 seg.

    python tools/gpu_resample_time.py [--calls 30] [--no-host] [--out profiles/resample_time.json]

Two resamplings: 2 mm -> 1 mm along x (155 x 240 x 240 -> 155 x 240 x 480) and 1 mm -> 1.5 mm isotropic (-> 103 x 160 x 160).  For
each: the cubic zoom of the data with the clip, the linear zoom, the label zoom with its counts - HIP events around whole calls, the
median over `--calls` calls after warm-up - and the per-kernel split of one cubic call and one label call (torch.profiler's device
activity) with the bytes each kernel moves BY THE ALGORITHM'S COUNT (not by a hardware counter) and the resulting TB/s.  Where scipy
imports, `scipy.ndimage.zoom` (order 3 per channel, and the per-label order-1 loop of `resize_segmentation`) on one core of the same
box for the same volumes, by the wall clock, once.

Every step runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"x_2mm_to_1mm": (155, 240, 480), "iso_1mm_to_1p5mm": (103, 160, 160)}
STEP_SECONDS = {"x_2mm_to_1mm": 300, "iso_1mm_to_1p5mm": 300, "host": 900}


def _inputs():
    import numpy as np
    from tests import preprocess_ref as R
    data, seg, _ = R.brats_case()
    return data, seg[0].astype(np.int16)


def kernel_bytes(C, shape, new_shape):
    """bytes per kernel of one cubic call and one label call, counted from the shapes: every array a kernel must read or write, once"""
    D, H, W = shape
    n, nout = D * H * W, new_shape[0] * new_shape[1] * new_shape[2]

    def line(lines, m):                  # causal: reads m, writes m + 4; anti-causal: reads and writes m + 4
        return 8 * C * lines * (m + 3 * (m + 4))
    return {"zoom_minmax_kernel": 4 * C * n,
            "zoom_fir_x_kernel": 4 * C * n + 8 * C * D * H * (W + 4),
            "zoom_line_kernel": [line(D * (W + 4), H), line((H + 4) * (W + 4), D)],        # y, then z
            "zoom_eval_kernel": 8 * C * (D + 4) * (H + 4) * (W + 4) + 4 * C * nout,
            "zoom_labels_kernel": 2 * n + 2 * nout}


def gpu_step(name, calls):
    import torch
    from segmamba_amd import lib as L
    from segmamba_amd import ops_raw
    from tools.gpu_metrics_time import event_ms, kernel_split
    lib = L.get_lib()
    data, seg = _inputs()
    td, ts = torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda()
    C, shape, new_shape = data.shape[0], data.shape[1:], CASES[name]

    def stats(ms, nbytes=None):
        out = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
        if nbytes is not None:
            out["bytes_by_count"] = int(nbytes)
            out["TB_per_s_by_count"] = nbytes / (out["ms_median"] * 1e-3) / 1e12
        return out
    kb = kernel_bytes(C, shape, new_shape)
    cubic_bytes = kb["zoom_minmax_kernel"] + kb["zoom_fir_x_kernel"] + sum(kb["zoom_line_kernel"]) + kb["zoom_eval_kernel"]
    rec = {"shape": list(shape), "new_shape": list(new_shape), "channels": C, "device": torch.cuda.get_device_name(0), "calls": calls,
           "workspace_bytes": int(lib.dll.segm_zoom_workspace_bytes(C, *shape, 3)),
           "zoom_order3_clip": stats(event_ms(lambda: ops_raw.zoom(lib, td, new_shape, 3, True), calls), cubic_bytes),
           "zoom_order1_clip": stats(event_ms(lambda: ops_raw.zoom(lib, td, new_shape, 1, True), calls)),
           "zoom_labels": stats(event_ms(lambda: ops_raw.zoom_labels(lib, ts, new_shape), calls), kb["zoom_labels_kernel"])}
    try:
        split = kernel_split(lambda: (ops_raw.zoom(lib, td, new_shape, 3, True), ops_raw.zoom_labels(lib, ts, new_shape)))
        kernels = {}
        for key, (cnt, us) in sorted(split.items(), key=lambda kv: -kv[1][1]):
            k = {"calls": cnt, "us_per_call": us / cnt}
            for short, b in kb.items():
                if short in key:
                    total = sum(b) if isinstance(b, list) else b
                    k["bytes_by_count"] = int(total)
                    k["TB_per_s_by_count"] = total / (us * 1e-6) / 1e12
            kernels[key] = k
        rec["kernels"] = kernels
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"
    return rec


def host_step():
    import numpy as np
    try:
        from scipy import ndimage
    except ImportError:
        return {"scipy": None}
    data, seg = _inputs()
    rec = {"host_cpus_used": 1, "note": "scipy.ndimage.zoom(mode='nearest', grid_mode=True) in float64, one call per channel / per label"}
    for name, new_shape in CASES.items():
        factors = [o / i for o, i in zip(new_shape, data.shape[1:])]
        t0 = time.perf_counter()
        for c in range(data.shape[0]):
            x = data[c].astype(np.float64)
            np.clip(ndimage.zoom(x, factors, order=3, mode="nearest", grid_mode=True), x.min(), x.max()).astype(np.float32)
        t1 = time.perf_counter()
        out = np.zeros(new_shape, dtype=np.int16)
        for lab in np.unique(seg):
            out[ndimage.zoom((seg == lab).astype(np.float64), factors, order=1, mode="nearest", grid_mode=True) >= 0.5] = lab
        t2 = time.perf_counter()
        rec[name] = {"zoom_order3_four_channels_s": t1 - t0, "resize_segmentation_s": t2 - t1, "labels": int(len(np.unique(seg)))}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step and print its record")
    args = ap.parse_args()
    if args.step is not None:
        rec = host_step() if args.step == "host" else gpu_step(args.step, args.calls)
        print("RECORD " + json.dumps(rec))
        return 0
    rec = {"case": "tests/preprocess_ref.brats_case: 4 x 155 x 240 x 240 fp32 with its seg as int16",
           "bytes": "by the algorithm's count from the shapes (tools/gpu_resample_time.py kernel_bytes), not by a hardware counter"}
    for step in list(CASES) + ([] if args.no_host else ["host"]):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--calls", str(args.calls)],
                               capture_output=True, text=True, timeout=STEP_SECONDS[step])
        except subprocess.TimeoutExpired:
            print(f"step {step}: no result within {STEP_SECONDS[step]} s; stopping", file=sys.stderr)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            print(f"step {step}: exit status {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        rec["scipy_one_core" if step == "host" else step] = json.loads(lines[-1][len("RECORD "):])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
