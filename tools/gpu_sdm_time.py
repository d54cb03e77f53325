"""Time the signed-distance and edge targets (segmamba_amd/sdm.py, csrc/sdm.hip) on the GPU.

    python tools/gpu_sdm_time.py [--calls 30] [--out profiles/sdm_time.json] [--no-scipy]

(a) `sdm_edge_targets` on a (2, 128, 128, 128) int64 label batch with the three BraTS regions, and on one 155 x 240 x 240 uint8 case
    (tests/metrics_ref.brats_size_case): medians over `--calls` calls after warm-up, HIP events around whole calls.
(b) in a profiler pass of its own (torch.profiler's device activity, one call): launches, the per-kernel split, and for the two new
    passes the bytes by the algorithm's count over their time - mask pass: the label and four bytes written per voxel; maxima: the
    inside byte and one int32 per voxel and live item; compose: three bit bytes, one int32 and two fp32 per voxel and item.  Reads of
    neighbours (caches) and packets that straddle the region's surface (both planes) are not counted: a lower bound on the traffic.
(c) `PatchLoader.next_with_targets()` against `next()` with `augment="fused"`, 128^3 patches, batch 2, from a resident case, the two
    alternating call by call on the same draws.
(d) once, tests/sdm_ref.py (the scipy calls of the reference) on one core for the same two inputs."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmamba_amd import preprocess as P                # noqa: E402
from segmamba_amd import sdm as T                       # noqa: E402
from segmamba_amd.dataloading import PatchLoader        # noqa: E402
from tests import metrics_ref as MR                     # noqa: E402
from tests import preprocess_ref as PR                  # noqa: E402
from tools.gpu_intensity_time import alternate_ms, stats          # noqa: E402
from tools.gpu_metrics_time import kernel_split         # noqa: E402


def patch_labels():
    """(2, 128, 128, 128) int64: nested rippled balls of the labels 2 > 1 > 3, the second sample shifted, -1 never (the loader maps it to 0)"""
    z, y, x = np.meshgrid(*[np.arange(128, dtype=np.float32)] * 3, indexing="ij")
    out = []
    for cz, cy, cx in ((60, 64, 66), (70, 58, 62)):
        r = np.sqrt((z - cz) ** 2 + (y - cy) ** 2 * 1.3 + (x - cx) ** 2 * 0.8) + 2.0 * np.sin(0.3 * x) * np.cos(0.25 * y)
        out.append(np.where(r < 14, 3, np.where(r < 26, 1, np.where(r < 40, 2, 0))).astype(np.int64))
    return np.stack(out)


def split_record(fn, n_vol, voxels, esize, live_items, items):
    try:
        split = kernel_split(fn)
    except Exception as exc:                  # the split is a record, not a result: say why it is missing
        return {"unavailable": f"{type(exc).__name__}: {exc}"}
    kernels = {}
    for key, (count, us) in sorted(split.items(), key=lambda kv: -kv[1][1]):
        row = {"calls": count, "us_total": us}
        nbytes = None
        if "sdm_masks_kernel" in key:
            nbytes = (esize + 4) * n_vol * voxels
        elif "sdm_max_kernel" in key:
            nbytes = 5 * live_items * voxels
        elif "sdm_compose_kernel" in key:
            nbytes = 15 * items * voxels
        if nbytes is not None:
            row["bytes_by_count"] = nbytes
            row["TB_per_s_by_count"] = nbytes / (us * 1e-6) / 1e12
        kernels[key] = row
    return {"launches": sum(r["calls"] for r in kernels.values()), "device_us": sum(r["us_total"] for r in kernels.values()), "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdm_time.json"))
    ap.add_argument("--no-scipy", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/gpu_sdm_time.py needs a GPU: nothing is measured without one")
    rec = {"device": torch.cuda.get_device_name(0), "calls": args.calls,
           "timing": "HIP events around whole calls, medians; the kernel split from a torch.profiler pass of its own",
           "bytes": "by the algorithm's count from the shapes, not by a hardware counter"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)

    def save():
        with open(args.out, "w") as f:        # what has been measured so far survives a later failure
            json.dump(rec, f, indent=1)
    batch = patch_labels()
    case = MR.brats_size_case()[1]
    for name, host in (("batch_2x128^3_int64", batch), ("case_155x240x240_uint8", case[None])):
        t = torch.from_numpy(host).cuda()
        ms, = alternate_ms([lambda: T.sdm_edge_targets(t)], args.calls)
        row = stats(ms)
        n_vol, voxels = host.shape[0], int(np.prod(host.shape[1:]))
        row["split"] = split_record(lambda: T.sdm_edge_targets(t), n_vol, voxels, host.dtype.itemsize, 3 * n_vol, 3 * n_vol)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        T.sdm_edge_targets(t)
        torch.cuda.synchronize()
        row["peak_allocated_bytes"] = int(torch.cuda.max_memory_allocated() - base)
        rec[name] = row
        print(name, json.dumps({k: row[k] for k in ("ms_median", "ms_min", "ms_max", "peak_allocated_bytes")}), flush=True)
        save()

    data, seg, _ = PR.brats_case()
    props = {"spacing": (1.0, 1.0, 1.0)}
    out, sout = P.preprocess_case(torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda(), props)

    class Resident:                           # one preprocessed case, as CaseDataset keeps it
        device = out.device

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"data": out, "seg": sout, "properties": props}
    loaders = [PatchLoader(Resident(), (128, 128, 128), batch_size=2, augment="fused"),
               PatchLoader(Resident(), (128, 128, 128), batch_size=2, augment="fused", targets="sdm_edge")]
    calls = [loaders[0].next, loaders[1].next_with_targets]
    states = [None, None]

    def turn(i):
        def run():                            # each loader continues its own stream of np.random draws: the same boxes for both
            if states[i] is not None:
                np.random.set_state(states[i])
            calls[i]()
            states[i] = np.random.get_state()
        return run
    np.random.seed(0)
    states[0] = states[1] = np.random.get_state()
    ms_next, ms_targets = alternate_ms([turn(0), turn(1)], args.calls)
    rec["patch_loader"] = {"patch": [128, 128, 128], "batch": 2, "augment": "fused", "next": stats(ms_next),
                           "next_with_targets": stats(ms_targets)}
    print(json.dumps(rec["patch_loader"]), flush=True)
    save()

    if not args.no_scipy:
        from tests import sdm_ref as S
        torch.set_num_threads(1)
        rec["scipy_one_core_s"] = {}
        for name, host in (("batch_2x128^3_int64", batch), ("case_155x240x240_uint8", case[None])):
            t0 = time.perf_counter()
            S.targets(host)
            rec["scipy_one_core_s"][name] = time.perf_counter() - t0
            print("scipy", name, rec["scipy_one_core_s"][name], flush=True)
            save()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
