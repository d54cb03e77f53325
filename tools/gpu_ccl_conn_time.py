"""Time the connected components at connectivity 1, 2 and 3 (csrc/ccl_roots.hip) on the synthetic 10-class 200 x 256 x 256 label map of
tools/gpu_ccl_labels_time.py.

    python tools/gpu_ccl_conn_time.py [--calls 30] [--shape 200 256 256] [--no-scipy] [--out profiles/ccl_conn_time.json]

Timed: `keep_largest_per_class` (all classes, one labelled pass) and `largest_connected_domain` of one organ's mask (label 5), each at
connectivity 1, 2 and 3.  HIP events around whole calls, the six variants alternating, the median over `--calls` calls after warm-up.
Yardsticks: the connectivity-1 calls (README records 0.270 ms for `keep_largest_per_class` there) and, once, `scipy.ndimage.label` with the full structure on the host - the only route to the
connectivity-3 result without these kernels.
Asserted before anything is timed (the tool fails otherwise, and the JSON records them): at every connectivity the label map of
`keep_largest_per_class` equals the per-class loop over the binary entries, its roots per class equal the binary entry's, two calls
are bit-equal, the keyword at 1 equals the call without it, and with scipy the number of components of the organ's mask equals
scipy's at every connectivity.
The per-kernel split of one call of each of the six variants comes from the profiler in passes of their own; bytes by the
algorithm's count."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch                # noqa: E402

from segmamba_amd import lib as L                       # noqa: E402
from segmamba_amd import ops_raw                        # noqa: E402
from segmamba_amd import postprocess as PP              # noqa: E402
from tests import ccl_labels_ref as LR                  # noqa: E402
from tools.gpu_ccl_labels_time import alternating_ms, stats     # noqa: E402
from tools.gpu_metrics_time import kernel_split         # noqa: E402

ORGAN = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--shape", type=int, nargs=3, default=(200, 256, 256))
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ccl_conn_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("a GPU is required: times are measured, never estimated")
    lib = L.get_lib()
    shape = tuple(args.shape)
    lab = LR.ten_class(shape, seed=0)
    t = torch.from_numpy(lab).cuda()
    organ = (t == ORGAN).to(torch.uint8)
    n = t.numel()
    conns = (1, 2, 3)

    def loop(c):
        out = torch.zeros_like(t)
        for k in range(1, 10):
            roots = ops_raw.ccl_roots(lib, (t == k).to(torch.uint8), connectivity=c)
            sizes, _ = ops_raw.ccl_sizes(lib, roots)
            out[ops_raw.ccl_select(lib, roots, sizes, L.CCL_LARGEST)[0] != 0] = k
        return out

    rec = {"case": f"tests/ccl_labels_ref.ten_class{shape}, seed 0", "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "voxels": n, "voxels_labelled": int((t != 0).sum().item()), "organ_label": ORGAN, "organ_voxels": int(organ.sum().item()),
           "components_per_class": {}, "organ_components": {}, "voxels_removed": {}, "asserted": {}}
    asserted = rec["asserted"]                            # a key is written where its check has just passed, nowhere else
    for c in conns:
        got = PP.keep_largest_per_class(t, connectivity=c)
        if not torch.equal(got, loop(c)):
            raise RuntimeError(f"connectivity {c}: keep_largest_per_class differs from the per-class loop")
        asserted[f"keep_largest_per_class_equals_per_class_loop_c{c}"] = True
        if not torch.equal(got, PP.keep_largest_per_class(t, connectivity=c)):
            raise RuntimeError(f"connectivity {c}: two calls differ")
        asserted[f"two_calls_bit_equal_c{c}"] = True
        roots = PP.label_component_roots(t, connectivity=c)
        for k in range(1, 10):
            m = t == k
            if not torch.equal(roots[m], PP.component_roots(m.to(torch.uint8), connectivity=c)[m]):
                raise RuntimeError(f"connectivity {c}: the roots of class {k} differ from the binary entry's")
        asserted[f"roots_per_class_equal_binary_entry_c{c}"] = True
        rec["components_per_class"][str(c)] = {str(k): v[0] for k, v in PP.class_component_summary(t, connectivity=c).items()}
        rec["organ_components"][str(c)] = PP.component_summary(organ, connectivity=c)[0]
        rec["voxels_removed"][str(c)] = int((got != t).sum().item())
    if not torch.equal(PP.keep_largest_per_class(t, connectivity=1), PP.keep_largest_per_class(t)) \
            or not torch.equal(PP.largest_connected_domain(organ, connectivity=1), PP.largest_connected_domain(organ)):
        raise RuntimeError("connectivity=1 differs from the call without the keyword")
    asserted["keyword_at_1_equals_call_without"] = True

    if not args.no_scipy:
        try:
            from scipy import ndimage
            host = (lab == ORGAN)
            rec["scipy_label_ms"] = {}
            for c in conns:
                t0 = time.perf_counter()
                _, num = ndimage.label(host, structure=ndimage.generate_binary_structure(3, c))
                rec["scipy_label_ms"][str(c)] = (time.perf_counter() - t0) * 1e3
                if num != rec["organ_components"][str(c)]:
                    raise RuntimeError(f"connectivity {c}: {rec['organ_components'][str(c)]} components of the organ, scipy finds {num}")
                asserted[f"organ_components_equal_scipy_c{c}"] = True
        except ImportError as exc:
            rec["scipy_label_ms"] = f"unavailable: {exc}"

    fns = [lambda c=c: PP.keep_largest_per_class(t, connectivity=c) for c in conns] \
        + [lambda c=c: PP.largest_connected_domain(organ, connectivity=c) for c in conns]
    ms = alternating_ms(fns, args.calls)
    rec["keep_largest_per_class"] = {str(c): stats(ms[i]) for i, c in enumerate(conns)}
    rec["largest_connected_domain"] = {str(c): stats(ms[3 + i]) for i, c in enumerate(conns)}
    for key in ("keep_largest_per_class", "largest_connected_domain"):
        rec[key]["c3_over_c1"] = rec[key]["3"]["ms_median"] / rec[key]["1"]["ms_median"]
        rec[key]["c3_minus_c1_ms"] = rec[key]["3"]["ms_median"] - rec[key]["1"]["ms_median"]

    # bytes the algorithm needs per launch, from the shapes: the byte volume, int32 labels / roots / sizes, the byte output.  The
    # merge launch reads every voxel's byte once; the up to 13 neighbour bytes of a boundary voxel come from lines already read.
    nbytes = {"roots_tile_kernel": n + 4 * n, "roots_merge_kernel": n, "roots_flatten_kernel": 4 * n + 4 * n, "ccl_sizes_kernel": 4 * n,
              "label_best_kernel": 4 * n, "label_select_kernel": n + 4 * n + n, "ccl_best_kernel": 4 * n, "ccl_select_kernel": 4 * n + n}
    rec["kernels"] = {}
    variants = [(f"keep_largest_per_class_c{c}", fns[i]) for i, c in enumerate(conns)] \
        + [(f"largest_connected_domain_c{c}", fns[3 + i]) for i, c in enumerate(conns)]
    for what, fn in variants:
        try:
            split = kernel_split(fn)
        except Exception as exc:          # the split is a record, not a result: say why it is missing
            rec["kernels"][what] = f"unavailable: {type(exc).__name__}: {exc}"
            continue
        out = {"launches": int(sum(k for k, _ in split.values())), "readbacks": 0, "device_us_total": sum(us for _, us in split.values()),
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
