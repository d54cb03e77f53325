"""Time the prediction-finishing stage (segmamba_amd/postprocess.py) at BraTS size, 155 x 240 x 240.

    python tools/gpu_postprocess_time.py [--calls 30] [--no-scipy] [--out profiles/postprocess_time.json]

(a) `labels_from_logits` against the route it replaces (`Predictor.predict_raw_probability` -> `argmax` -> `.cpu()` ->
    `predict_noncrop_probability`) on the same 4-class fp32 logits, at identity size and at a resampling size;
(b) `label`, `binary_fill_holes`, `largest_connected_domain` on the prediction's WT mask and on `pred == 2` (the shell whose hole is
    filled), against scipy.ndimage on one host core (where it imports) and against the propagation written with ATen ops on the device
    (tests/postprocess_checks.torch_roots);
(c) per kernel of one call: time, bytes moved by the algorithm's count, launches.
HIP events around whole calls, the median over `--calls` calls after warm-up; the host route and scipy by the wall clock."""
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
from segmamba_amd.predictor import Predictor            # noqa: E402
from tests import metrics_ref as MR                     # noqa: E402
from tests import postprocess_checks as K               # noqa: E402
from tools.gpu_metrics_time import event_ms, kernel_split      # noqa: E402

SHAPE = (155, 240, 240)


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def wall_ms(fn, calls, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def logits_for(labels: np.ndarray, shape) -> torch.Tensor:
    """4-class fp32 logits on the device whose arg-max at `labels`' size follows the label map: smooth, no ties"""
    g = torch.Generator(device="cuda").manual_seed(0)
    onehot = torch.stack([torch.from_numpy(labels == c) for c in range(4)]).float().cuda()
    v = torch.nn.functional.interpolate(onehot[None] * 4.0, size=tuple(shape), mode="trilinear", align_corners=False)[0]
    return (v + 0.3 * torch.randn(v.shape, device="cuda", generator=g)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "postprocess_time.json"))
    args = ap.parse_args()
    lib = L.get_lib()
    pred, _ = MR.brats_size_case()
    n = pred.size
    rec = {"case": "tests/metrics_ref.brats_size_case: 155 x 240 x 240", "device": torch.cuda.get_device_name(0), "calls": args.calls}

    # (a) logits -> labels
    rec["labels_from_logits"] = {}
    for name, in_shape, box, full, start in (("identity", SHAPE, SHAPE, SHAPE, (0, 0, 0)),
                                              ("identity_pasted", (136, 176, 152), (136, 176, 152), SHAPE, (10, 32, 44)),
                                              ("resampled", (124, 192, 192), SHAPE, SHAPE, (0, 0, 0))):
        small = pred if in_shape == SHAPE else pred[:in_shape[0], :in_shape[1], :in_shape[2]]
        logits = logits_for(small, in_shape)
        props = {"shape_after_cropping_before_resample": list(box), "shape_before_cropping": list(full),
                 "bbox_used_for_cropping": [[s, s + b] for s, b in zip(start, box)]}

        def parent_route():
            return Predictor.predict_noncrop_probability(Predictor.predict_raw_probability(logits, props).argmax(dim=0), props)

        def parent_device_part():
            return Predictor.predict_raw_probability(logits, props).argmax(dim=0)
        got = PP.labels_from_logits(logits, props)
        differ = int((got.cpu().numpy() != parent_route()).sum())
        esize = logits.element_size()
        entry = {"logits": list(logits.shape), "box": list(box), "output": list(full), "voxels_that_differ_from_the_parent_route": differ,
                 "this": stats(event_ms(lambda: PP.labels_from_logits(logits, props), args.calls)),
                 "this_with_region_planes": stats(event_ms(lambda: PP.labels_from_logits(logits, props, regions=MR.BRATS_REGIONS), args.calls)),
                 "parent_route_wall": stats(wall_ms(parent_route, max(3, args.calls // 6))),
                 "parent_route_device_part": stats(event_ms(parent_device_part, args.calls)),
                 "bytes_by_count": {"this": logits.numel() * esize + int(np.prod(full)),
                                    "parent_device_part": 4 * (logits.numel() // 4 * esize + int(np.prod(box)) * 4)      # interpolations
                                    + 2 * 4 * int(np.prod(box)) * 4                                                      # stack
                                    + 4 * int(np.prod(box)) * 4 + int(np.prod(box)) * 8}}                                # argmax
        entry["this_TB_per_s"] = entry["bytes_by_count"]["this"] / (entry["this"]["ms_median"] * 1e-3) / 1e12
        rec["labels_from_logits"][name] = entry

    # (b) components
    masks = {"pred_WT": MR.region_mask(pred, (1, 2, 3)).astype(np.uint8), "pred_label2": (pred == 2).astype(np.uint8)}
    rec["components"] = {}
    for name, m in masks.items():
        t = torch.from_numpy(m).cuda()
        e = {"voxels_set": int(m.sum()),
             "label": stats(event_ms(lambda: PP.label(t), args.calls)),
             "ccl_roots": stats(event_ms(lambda: ops_raw.ccl_roots(lib, t), args.calls)),
             "binary_fill_holes": stats(event_ms(lambda: PP.binary_fill_holes(t), args.calls)),
             "largest_connected_domain": stats(event_ms(lambda: PP.largest_connected_domain(t), args.calls)),
             "aten_propagation_roots": stats(event_ms(lambda: K.torch_roots(t), 3, warmup=1)),
             "aten_propagation_fill": stats(event_ms(lambda: K.torch_fill(t), 3, warmup=1))}
        if not args.no_scipy:
            try:
                from scipy import ndimage
                t0 = time.perf_counter()
                ndimage.label(m)
                t1 = time.perf_counter()
                ndimage.binary_fill_holes(m)
                t2 = time.perf_counter()
                e["scipy_label_s"], e["scipy_binary_fill_holes_s"], e["host_cpus_used"] = t1 - t0, t2 - t1, 1
            except ImportError:
                e["scipy_label_s"] = None
        rec["components"][name] = e
    rec["postprocess_labels_three_regions"] = stats(event_ms(lambda: PP.postprocess_labels(torch.from_numpy(pred).cuda()), args.calls))

    # (c) per kernel
    t = torch.from_numpy(masks["pred_WT"]).cuda()
    nbytes = {"roots_tile_kernel": n + 4 * n, "roots_merge_kernel": n, "roots_flatten_kernel": 4 * n + 4 * n, "ccl_sizes_kernel": 4 * n,
              "ccl_best_kernel": 4 * n, "ccl_select_kernel": 4 * n + n, "resample_argmax_kernel": 4 * 4 * n + n}
    logits = logits_for(pred, SHAPE)
    calls_of = {"largest_connected_domain": lambda: PP.largest_connected_domain(t), "labels_from_logits": lambda: PP.labels_from_logits(logits)}
    rec["kernels"] = {}
    for what, fn in calls_of.items():
        try:
            split = kernel_split(fn)
        except Exception as exc:          # the split is a record, not a result: say why it is missing
            rec["kernels"][what] = f"unavailable: {type(exc).__name__}: {exc}"
            continue
        out = {"launches": int(sum(c for c, _ in split.values())), "readbacks": 0, "by_kernel": {}}
        for kname, (cnt, us) in split.items():
            row = {"calls": cnt, "us_per_call": us / cnt}
            for key, b in nbytes.items():
                if key in kname:
                    row["bytes_per_call_by_count"] = b
                    row["TB_per_s"] = b / (us / cnt * 1e-6) / 1e12
            out["by_kernel"][kname] = row
        rec["kernels"][what] = out
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
