"""Time the separate-z resampling branch (segmamba_amd/resample.py `allow_separate_z=True` on segm_zoom_slices /
segm_zoom_labels_slices of csrc/resample.hip) on a synthetic thick-slice CT crop: 1 x 120 x 512 x 512 fp32 with its int16 seg at
spacing (5, 0.75, 0.75) -> (2.5, 1, 1), that is 240 x 384 x 384.

    python tools/gpu_resample_sepz_time.py [--calls 30] [--no-host] [--out profiles/resample_sepz_time.json]

HIP events around whole calls, the median over `--calls` calls after warm-up:
  * `resample_data_or_seg_to_shape(allow_separate_z=True, force_separate_z=None)` for the data (order 3) and for the seg, and the data
    at order 1;
  * the same output computed once per DISTINCT source slice and then copied (`zoom_slices` with the identity table to 120 slices, then
    `index_select` by the table): what copy-on-repeat instead of recomputing would cost at best;
  * for scale only, `ops_raw.zoom` and `ops_raw.zoom_labels` to the same shape - the one 3-D route, which computes something else;
and the per-kernel split of one data call and one seg call (torch.profiler's device activity) with the bytes each kernel moves BY THE
ALGORITHM'S COUNT (not by a hardware counter), and the workspace bytes.  Where scipy imports, the same resampling with
`scipy.ndimage.zoom` per slice (and per label of a slice) on one core of the same box, by the wall clock, once.

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

SHAPE, NEW_SHAPE = (120, 512, 512), (240, 384, 384)
SPACING, NEW_SPACING = (5.0, 0.75, 0.75), (2.5, 1.0, 1.0)
STEP_SECONDS = {"gpu": 300, "host": 600}


def _inputs():
    """a smooth body of soft tissue with two organs and a bright core in air, noise on top: HU-like values, labels 0 .. 3"""
    import numpy as np
    rng = np.random.RandomState(11)
    z, y, x = np.meshgrid(*[np.linspace(-1.0, 1.0, n, dtype=np.float32) for n in SHAPE], indexing="ij")
    r2 = (z / 0.95) ** 2 + (y / 0.8) ** 2 + (x / 0.9) ** 2
    data = np.where(r2 < 1.0, 40.0 + 60.0 * np.sin(5.0 * x) * np.cos(4.0 * y), -1000.0).astype(np.float32)
    data += (15.0 * rng.standard_normal(SHAPE)).astype(np.float32)
    seg = np.zeros(SHAPE, dtype=np.int16)
    seg[(z / 0.6) ** 2 + ((y - 0.1) / 0.45) ** 2 + ((x + 0.2) / 0.4) ** 2 < 1.0] = 1
    seg[(z / 0.3) ** 2 + ((y - 0.1) / 0.2) ** 2 + ((x + 0.2) / 0.2) ** 2 < 1.0] = 2
    seg[(z / 0.5) ** 2 + ((y + 0.3) / 0.15) ** 2 + ((x - 0.4) / 0.2) ** 2 < 1.0] = 3
    data[seg == 2] += 900.0
    return data[None], seg


def kernel_bytes(C, shape, new_shape):
    """bytes per kernel of one data call (order 3) and one seg call, counted from the shapes: every array a kernel must read or write, once"""
    S, H, W = shape
    n, nout = S * H * W, new_shape[0] * new_shape[1] * new_shape[2]
    return {"zoom_slice_minmax_kernel": 4 * C * n,
            "zoom_fir_x_kernel": 4 * C * n + 8 * C * S * H * (W + 4),
            "zoom_line_kernel": 8 * C * S * (W + 4) * (H + 3 * (H + 4)),      # causal: reads H, writes H + 4; anti-causal: both H + 4
            "zoom_slices_eval_kernel": 8 * C * S * (H + 4) * (W + 4) + 4 * C * nout,
            "zoom_labels_slices_kernel": 2 * n + 2 * nout}


def gpu_step(calls):
    import torch
    from segmamba_amd import lib as L
    from segmamba_amd import ops_raw
    from segmamba_amd import resample as RS
    from tools.gpu_metrics_time import event_ms, kernel_split
    lib = L.get_lib()
    data, seg = _inputs()
    td, ts = torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda()
    C = data.shape[0]

    def stats(ms, nbytes=None):
        out = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
        if nbytes is not None:
            out["bytes_by_count"] = int(nbytes)
            out["TB_per_s_by_count"] = nbytes / (out["ms_median"] * 1e-3) / 1e12
        return out

    def sepz(t, is_seg, order):
        return RS.resample_data_or_seg_to_shape(t, NEW_SHAPE, SPACING, NEW_SPACING, is_seg, order, 0, None, allow_separate_z=True)
    table = torch.from_numpy(RS.slice_table(SHAPE[0], NEW_SHAPE[0])).cuda()
    identity = torch.arange(SHAPE[0], dtype=torch.int32).cuda()
    once = (SHAPE[0],) + NEW_SHAPE[1:]

    def copy_on_repeat():
        return ops_raw.zoom_slices(lib, td, once, identity, 3, True).index_select(1, table.long())
    assert torch.equal(copy_on_repeat(), sepz(td, False, 3)), "computing once and copying gives the same bits"
    kb = kernel_bytes(C, SHAPE, NEW_SHAPE)
    data_bytes = sum(v for k, v in kb.items() if k != "zoom_labels_slices_kernel")
    rec = {"shape": list(SHAPE), "new_shape": list(NEW_SHAPE), "spacing": list(SPACING), "new_spacing": list(NEW_SPACING), "channels": C,
           "device": torch.cuda.get_device_name(0), "calls": calls,
           "workspace_bytes": int(lib.dll.segm_zoom_slices_workspace_bytes(C, *SHAPE, *NEW_SHAPE[1:], 3)),
           "workspace_bytes_3d_zoom": int(lib.dll.segm_zoom_workspace_bytes(C, *SHAPE, 3)),
           "separate_z_data_order3": stats(event_ms(lambda: sepz(td, False, 3), calls), data_bytes),
           "separate_z_data_order1": stats(event_ms(lambda: sepz(td, False, 1), calls)),
           "separate_z_seg": stats(event_ms(lambda: sepz(ts[None], True, 1), calls), kb["zoom_labels_slices_kernel"]),
           "compute_once_then_copy_order3": stats(event_ms(copy_on_repeat, calls)),
           "yardstick_3d_zoom_order3": stats(event_ms(lambda: ops_raw.zoom(lib, td, NEW_SHAPE, 3, True), calls)),
           "yardstick_3d_zoom_labels": stats(event_ms(lambda: ops_raw.zoom_labels(lib, ts, NEW_SHAPE), calls))}
    try:
        split = kernel_split(lambda: (sepz(td, False, 3), sepz(ts[None], True, 1)))
        kernels = {}
        for key, (cnt, us) in sorted(split.items(), key=lambda kv: -kv[1][1]):
            k = {"calls": cnt, "us_per_call": us / cnt}
            for short, b in kb.items():
                if short in key:
                    k["bytes_by_count"] = int(b)
                    k["TB_per_s_by_count"] = b / (us * 1e-6) / 1e12
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
    from segmamba_amd.resample import slice_table
    data, seg = _inputs()
    factors = [o / i for o, i in zip(NEW_SHAPE[1:], SHAPE[1:])]
    table = slice_table(SHAPE[0], NEW_SHAPE[0])
    t0 = time.perf_counter()
    slices = []
    for k in range(SHAPE[0]):
        x = data[0, k].astype(np.float64)
        slices.append(np.clip(ndimage.zoom(x, factors, order=3, mode="nearest", grid_mode=True), x.min(), x.max()))
    np.stack(slices)[table].astype(np.float32)
    t1 = time.perf_counter()
    slices = []
    for k in range(SHAPE[0]):
        out = np.zeros(NEW_SHAPE[1:], dtype=np.int16)
        for lab in np.unique(seg[k]):
            out[ndimage.zoom((seg[k] == lab).astype(np.float64), factors, order=1, mode="nearest", grid_mode=True) >= 0.5] = lab
        slices.append(out)
    np.stack(slices)[table]
    t2 = time.perf_counter()
    return {"host_cpus_used": 1, "note": "scipy.ndimage.zoom(mode='nearest', grid_mode=True) in float64 per slice / per label of a slice, then the table",
            "data_order3_s": t1 - t0, "seg_s": t2 - t1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_sepz_time.json"))
    ap.add_argument("--step", default=None, help="(internal) run one step and print its record")
    args = ap.parse_args()
    if args.step is not None:
        rec = host_step() if args.step == "host" else gpu_step(args.calls)
        print("RECORD " + json.dumps(rec))
        return 0
    rec = {"case": "synthetic CT crop 1 x 120 x 512 x 512 fp32 with its seg as int16 (tools/gpu_resample_sepz_time.py _inputs)",
           "bytes": "by the algorithm's count from the shapes (tools/gpu_resample_sepz_time.py kernel_bytes), not by a hardware counter"}
    for step in ["gpu"] + ([] if args.no_host else ["host"]):
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
        rec["scipy_one_core" if step == "host" else "separate_z"] = json.loads(lines[-1][len("RECORD "):])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
