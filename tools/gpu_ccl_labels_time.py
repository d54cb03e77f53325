"""Time `keep_largest_per_class` (one labelled connected-components pass, csrc/ccl_roots.hip and ccl_labels.hip) against the per-class
loop over the binary entries that gives the same label map, on a synthetic 10-class 200 x 256 x 256 volume.

    python tools/gpu_ccl_labels_time.py [--calls 30] [--shape 200 256 256] [--out profiles/ccl_labels_time.json]

The volume (tests/ccl_labels_ref.ten_class): nine blobs, labels 1 .. 9, each with two islands, plus speckle of a few thousand
one-voxel components.  The loop is what the parent commit offers: per class `labels == c` -> ccl_roots -> ccl_sizes -> ccl_select
(LARGEST), recombined.  The two outputs must be equal, or the tool fails.
HIP events around whole calls, the two routes alternating, the median over `--calls` calls after warm-up; launches and the per-kernel
split of one call of each route from the profiler in passes of their own; bytes by the algorithm's count."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                # noqa: E402

from segmamba_amd import lib as L                       # noqa: E402
from segmamba_amd import ops_raw                        # noqa: E402
from segmamba_amd import postprocess as PP              # noqa: E402
from tests import ccl_labels_ref as LR                  # noqa: E402
from tools.gpu_metrics_time import kernel_split         # noqa: E402


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def alternating_ms(fns, calls, warmup=3):
    """one timed call of every function per round, in turn: drift of the shared machine hits all of them alike"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(calls):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--shape", type=int, nargs=3, default=(200, 256, 256))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccl_labels_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("a GPU is required: times are measured, never estimated")
    lib = L.get_lib()
    shape = tuple(args.shape)
    lab = LR.ten_class(shape, seed=0)
    t = torch.from_numpy(lab).cuda()
    n = t.numel()
    classes = list(range(1, 10))

    def one_pass():
        return PP.keep_largest_per_class(t)

    def loop():
        out = torch.zeros_like(t)
        for c in classes:
            roots = ops_raw.ccl_roots(lib, (t == c).to(torch.uint8))
            sizes, _ = ops_raw.ccl_sizes(lib, roots)
            out[ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST)[0] != 0] = c
        return out

    got, want = one_pass(), loop()
    if not torch.equal(got, want):
        raise RuntimeError(f"the two routes differ in {int((got != want).sum().item())} voxels")
    summary = PP.class_component_summary(t)
    rec = {"case": f"tests/ccl_labels_ref.ten_class{shape}, seed 0", "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "voxels": n, "voxels_labelled": int((t != 0).sum().item()), "voxels_removed": int((got != t).sum().item()),
           "components_per_class": {str(c): v[0] for c, v in summary.items()}, "outputs_equal": True}
    ms_one, ms_loop = alternating_ms([one_pass, loop], args.calls)
    rec["keep_largest_per_class"] = stats(ms_one)
    rec["per_class_loop"] = stats(ms_loop)
    rec["loop_over_one_pass"] = rec["per_class_loop"]["ms_median"] / rec["keep_largest_per_class"]["ms_median"]

    # bytes the algorithm needs per launch, from the shapes: label bytes, int32 labels / roots / sizes, the byte output
    nbytes = {"roots_tile_kernel": n + 4 * n, "roots_merge_kernel": n, "roots_flatten_kernel": 4 * n + 4 * n, "ccl_sizes_kernel": 4 * n,
              "label_best_kernel": 4 * n, "label_select_kernel": n + 4 * n + n, "ccl_best_kernel": 4 * n, "ccl_select_kernel": 4 * n + n}
    rec["kernels"] = {}
    for what, fn in (("keep_largest_per_class", one_pass), ("per_class_loop", loop)):
        try:
            split = kernel_split(fn)
        except Exception as exc:          # the split is a record, not a result: say why it is missing
            rec["kernels"][what] = f"unavailable: {type(exc).__name__}: {exc}"
            continue
        out = {"launches": int(sum(c for c, _ in split.values())), "readbacks": 0, "device_us_total": sum(us for _, us in split.values()),
               "by_kernel": {}}
        for kname, (cnt, us) in sorted(split.items(), key=lambda kv: -kv[1][1]):
            row = {"calls": cnt, "us_per_call": us / cnt}
            for key, b in nbytes.items():
                if "::" + key in kname or kname.startswith(key):
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
