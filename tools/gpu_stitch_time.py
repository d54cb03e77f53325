"""What stitching a prediction costs, on both routes (`stitch="aten"` and `stitch="hip"` of segmamba_amd/predictor.py), on the case of
tools/gpu_predict_time.py: 1 x 4 x 138 x 176 x 144, 128^3 windows, overlap 0.5, gaussian, mirror [0, 1, 2], sw_batch_size 2 and 8.

  (a) stitching alone: the predictor returns a preallocated (n, 4, 128^3) bf16 tensor, so a call is gather / blend / finish (or
      their ATen counterparts) and nothing else.  Medians of 30 calls, HIP events around whole calls; the kernels one by one with the
      bytes the algorithm has to move held against the copy rate; launches per call; the peak of the allocator on both routes.
  (b) the whole case through SegMamba on both routes, median of 5, and the largest absolute difference between the two results.

    python tools/gpu_stitch_time.py            ->  profiles/stitch_time.json
"""
import json
import os
import statistics
import sys

for _k in ("FWD", "BWD", "WRW"):
    os.environ.setdefault("MIOPEN_DEBUG_CONV_DIRECT_NAIVE_CONV_" + _k, "0")
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd import predictor as P

SHAPE, ROI, COUT, AXES = (1, 4, 138, 176, 144), (128, 128, 128), 4, [0, 1, 2]
COPY_RATE_TBS = 5.5                                   # what the library's other byte-work kernels reach (5 - 6 TB/s)


class Canned(torch.nn.Module):
    """a predictor that costs nothing: the first n windows of a preallocated bf16 tensor"""

    def __init__(self, buf):
        super().__init__()
        self.buf = buf

    def forward(self, win):
        return self.buf[:win.shape[0]]


def timed(fn, reps):
    """-> the median of `reps` calls in ms, HIP events around each whole call"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def peak_of(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def kernel_row(ms, nbytes):
    tbs = nbytes / (ms * 1e-3) / 1e12
    return {"ms": round(ms, 4), "bytes": int(nbytes), "TB_per_s": round(tbs, 3), "of_copy_rate": round(tbs / COPY_RATE_TBS, 3)}


def kernels_alone(lib, x, swb, dev):
    """every entry on the case's shapes, one launch each: median ms, the bytes by the algorithm's count, the rate"""
    size = SHAPE[2:]
    starts = P.dense_patch_starts(size, ROI, (64, 64, 64))
    jobs = [(0,) + tuple(st) for st in starts][:swb]
    rv, V, C = ROI[0] * ROI[1] * ROI[2], size[0] * size[1] * size[2], SHAPE[1]
    weight = P.importance_map(ROI, "gaussian", 0.125, dev, torch.float32)
    axis_starts = [sorted(set(st[d] for st in starts)) for d in range(3)]
    count = ops_raw.window_count(lib, weight, size, axis_starts)
    pred = torch.randn((swb, COUT) + ROI, device=dev).to(torch.bfloat16)
    acc = torch.zeros((1, COUT) + size, device=dev)
    total = torch.zeros((1, COUT) + size, device=dev)
    covered = np.zeros(size, dtype=bool)
    for _, z, y, xx in jobs:
        covered[z:z + ROI[0], y:y + ROI[1], xx:xx + ROI[2]] = True
    union = int(covered.sum())
    out = {}
    for mask in (0, 7):
        out[f"gather_mask{mask}"] = kernel_row(timed(lambda: ops_raw.window_gather(lib, x, ROI, jobs, mask), 30), 2 * swb * C * rv * 4)
    out["count"] = kernel_row(timed(lambda: ops_raw.window_count(lib, weight, size, axis_starts), 30), V * 4 + rv * 4)
    out["blend_bf16"] = kernel_row(timed(lambda: ops_raw.window_blend(lib, acc, pred, weight, jobs), 30),
                                   swb * COUT * rv * 2 + rv * 4 + 2 * union * COUT * 4)
    for mask, index in ((0, 0), (7, 1)):              # pass 0 writes total, a later pass reads it as well; both zero acc
        out[f"finish_mask{mask}_pass{index}"] = kernel_row(
            timed(lambda: ops_raw.window_finish(lib, acc, count, total, ROI, mask, index, 8), 30),
            COUT * V * 4 * (2 + (1 if index else 0)) + V * 4 + COUT * V * 4)
    return out


def main():
    dev = torch.device("cuda")
    lib = L.get_lib()
    torch.manual_seed(0)
    x = torch.rand(SHAPE, device=dev)
    result = {"case": {"shape": SHAPE, "roi": ROI, "overlap": 0.5, "mode": "gaussian", "mirror_axes": AXES, "out_channels": COUT},
              "device": torch.cuda.get_device_name(0), "copy_rate_TB_per_s_assumed": COPY_RATE_TBS, "stitching_alone": {}, "whole_case": {}}
    windows, passes = 8, 8
    for swb in (2, 8):
        canned = Canned(torch.randn((swb, COUT) + ROI, device=dev).to(torch.bfloat16)).to(dev)
        row = {}
        outs = {}
        for route in ("aten", "hip"):
            inferer = P.SlidingWindowInferer(roi_size=ROI, sw_batch_size=swb, overlap=0.5, mode="gaussian", stitch=route)
            pred = P.Predictor(inferer, AXES)

            def call():
                outs[route] = pred.maybe_mirror_and_predict(x, canned, device=dev)
            row[route + "_ms"] = round(timed(call, 30), 3)
            row[route + "_peak_bytes"] = peak_of(call)
        chunks = -(-windows // swb)
        row["equal"] = bool(torch.equal(outs["aten"], outs["hip"]))
        memsets = passes if any(s < r for s, r in zip(SHAPE[2:], ROI)) else 0      # only a padded image needs one
        row["hip_launches_per_call"] = {"count": 1, "gather": passes * chunks, "blend": passes * chunks, "finish": passes,
                                        "memset": memsets, "total": 1 + passes * (2 * chunks + 1) + memsets}
        row["kernels"] = kernels_alone(lib, x, swb, dev)
        result["stitching_alone"][f"sw_batch_{swb}"] = row
        print(json.dumps({f"stitching_alone sw_batch {swb}": row}), flush=True)
        del canned, outs
        torch.cuda.empty_cache()

    from segmamba_amd.segmamba import SegMamba
    model = SegMamba(in_chans=4, out_chans=COUT, depths=[2, 2, 2, 2], feat_size=[48, 96, 192, 384]).to(dev).eval()
    for swb in (2, 8):
        row = {}
        outs = {}
        for route in ("aten", "hip"):
            inferer = P.SlidingWindowInferer(roi_size=ROI, sw_batch_size=swb, overlap=0.5, mode="gaussian", stitch=route)
            pred = P.Predictor(inferer, AXES)

            def call():
                outs[route] = pred.maybe_mirror_and_predict(x, model, device=dev)
            row[route + "_ms"] = round(timed(call, 5), 2)
        row["max_abs_difference"] = float((outs["aten"] - outs["hip"]).abs().max())
        row["max_abs_value"] = float(outs["aten"].abs().max())
        result["whole_case"][f"sw_batch_{swb}"] = row
        print(json.dumps({f"whole_case sw_batch {swb}": row}), flush=True)
    path = os.path.join(ROOT, "profiles", "stitch_time.json")
    with open(path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
