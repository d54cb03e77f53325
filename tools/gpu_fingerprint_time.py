"""Time the CT fingerprint (segmamba_amd/preprocess.py on csrc/fingerprint.hip) at CT size, 1 x 400 x 512 x 512, and the CT normalisation.

    python tools/gpu_fingerprint_time.py [--calls 30] [--no-host] [--shape 400 512 512] [--out profiles/fingerprint_time.json]

A synthetic CT-like case (HU-like integers, seg uint8) with an organ of about 2 % of the voxels, and the same case with 50 % foreground.
Per case:
(a) `collect_foreground_intensities` as a whole, its two readbacks included;
(b) the entries on their own - count + scan, the three selection passes with their select kernels, the gather of 10 000 ranks - each
    with the bytes it moves by the algorithm's count (not a hardware counter) and the resulting TB/s.  A pass reads the seg of every
    voxel of a segment that holds foreground, and 4 bytes of data per voxel of it; segments without foreground cost their two offsets;
(c) the ATen route on the device: `images[c][mask]`, `torch.sort`, indexing the sorted array and the compaction;
(d) numpy on one core, once (unless --no-host).
Then `segm_crop_clip_normalize` against `segm_crop_normalize` on the 155 x 240 x 240 x 4 crop of tools/gpu_preprocess_time.py.
HIP events around whole calls, the median over `--calls` calls after warm-up; the host by the wall clock."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np          # noqa: E402
import torch                # noqa: E402

from segmamba_amd import lib as L                       # noqa: E402
from segmamba_amd import ops_raw                        # noqa: E402
from segmamba_amd import postprocess as PP              # noqa: E402
from segmamba_amd import preprocess as P                # noqa: E402
from tests import preprocess_ref as R                   # noqa: E402
from tools.gpu_metrics_time import event_ms, kernel_split      # noqa: E402
from tools.gpu_preprocess_time import stats, with_rate         # noqa: E402


def ct_like(shape, share, seed=0):
    """-> (data (1, D, H, W) fp32 of HU-like integers, seg (1, D, H, W) uint8: an ellipsoid of `share` of the voxels), on the device"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    data = torch.round(300.0 * torch.randn((1,) + tuple(shape), generator=g, device="cuda") - 200.0)
    r = [n * (share * 6.0 / np.pi) ** (1.0 / 3.0) / 2.0 for n in shape]         # (4 / 3) pi r0 r1 r2 = share * D H W
    axes = [((torch.arange(n, device="cuda", dtype=torch.float32) - n / 2.0) / ri) ** 2 for n, ri in zip(shape, r)]
    inside = (axes[0][:, None, None] + axes[1][None, :, None] + axes[2][None, None, :]) <= 1.0
    return data, inside.to(torch.uint8)[None]


def one_case(lib, shape, share, calls, host):
    data, seg = ct_like(shape, share)
    nvox = int(np.prod(shape))
    count, sums, state = ops_raw.fg_count(lib, data, seg[0])
    n = int(count)
    ranks, _ = P._fingerprint_ranks(n)
    idx = torch.from_numpy(np.random.RandomState(1234).randint(0, n, 10000)).cuda()
    nseg = (nvox + L.FG_SEGMENT - 1) // L.FG_SEGMENT
    flat = torch.zeros(nseg * L.FG_SEGMENT, dtype=torch.uint8, device="cuda")
    flat[:nvox] = seg.reshape(-1)
    live = int((flat.view(nseg, L.FG_SEGMENT).sum(1, dtype=torch.int64) > 0).sum())
    pass_bytes = live * L.FG_SEGMENT * 5 + nseg * 16
    rec = {"shape": list(shape), "voxels": nvox, "foreground": n, "share": n / nvox, "segments": nseg, "segments_with_foreground": live,
           "workspace_bytes": int(lib.dll.segm_fg_workspace_bytes(1, nvox))}
    rec["collect_foreground_intensities"] = stats(event_ms(lambda: P.collect_foreground_intensities(seg, data), calls))
    rec["parts"] = {
        "count_and_scan": with_rate(event_ms(lambda: ops_raw.fg_count(lib, data, seg[0]), calls), nvox + 4 * n),
        "order_stats_three_passes": with_rate(event_ms(lambda: ops_raw.fg_order_stats(lib, state, n, ranks), calls), 3 * pass_bytes),
        "gather_10000": with_rate(event_ms(lambda: ops_raw.fg_gather(lib, state, n, idx), calls), 10000 * (L.FG_SEGMENT + 4 + 8 * 20)),
    }
    try:
        split = kernel_split(lambda: P.collect_foreground_intensities(seg, data))
        rec["kernels"] = {k: {"calls": c, "us_per_call": us / c} for k, (c, us) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"

    def aten():
        fg = data[0][seg[0] > 0]
        s = torch.sort(fg).values
        return s[torch.tensor(ranks, device="cuda")], fg[idx]
    want = aten()
    got = ops_raw.fg_order_stats(lib, state, n, ranks)[0], ops_raw.fg_gather(lib, state, n, idx)[0]
    rec["equal_to_aten"] = bool(torch.equal(want[0], got[0]) and torch.equal(want[1], got[1]))
    rec["aten_mask_sort_index"] = stats(event_ms(aten, max(3, calls // 3)))
    del want, got
    if host:
        d, s = data.cpu().numpy(), seg.cpu().numpy()
        t0 = time.perf_counter()
        fg = d[0][s[0] > 0]
        t1 = time.perf_counter()
        np.random.RandomState(1234).choice(fg, 10000, replace=True)
        np.mean(fg), np.median(fg), np.min(fg), np.max(fg), np.percentile(fg, 99.5), np.percentile(fg, 0.5)
        t2 = time.perf_counter()
        rec["numpy_one_core"] = {"compaction_s": t1 - t0, "samples_and_statistics_s": t2 - t1, "host_cpus_used": 1}
    return rec


def normalise(lib, calls):
    data, seg, _ = R.brats_case()
    td, ts = torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda()
    C = data.shape[0]
    mask, bbox = ops_raw.nonzero_mask_bbox(lib, td)
    filled = PP._fill(lib, mask)
    z0, y0, x0, z1, y1, x1 = (int(v) for v in bbox.tolist())
    start, shape = [z0, y0, x0], [z1 - z0, y1 - y0, x1 - x0]
    nb = int(np.prod(shape))
    nbp = shape[0] * shape[1] * 4 * ((x1 + 3) // 4 - x0 // 4)
    nbytes = (4 * C + 4 + 1) * nbp + (4 * C + 2) * nb
    _, s32 = ops_raw.crop_stats(lib, td, start, shape)
    s64 = torch.cat([s32, torch.full((8,), -1.5, device="cuda"), torch.full((8,), 2.5, device="cuda")])
    return {"case": "tests/preprocess_ref.brats_case: 4 x 155 x 240 x 240 fp32, seg fp32", "box": [start, shape],
            "crop_normalize": with_rate(event_ms(lambda: ops_raw.crop_normalize(lib, td, s32, start, shape, mask=filled, seg=ts[0]), calls), nbytes),
            "crop_clip_normalize": with_rate(event_ms(lambda: ops_raw.crop_clip_normalize(lib, td, s64, start, shape, mask=filled, seg=ts[0]),
                                                      calls), nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--shape", nargs=3, type=int, default=[400, 512, 512])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fingerprint_time.json"))
    args = ap.parse_args()
    lib = L.get_lib()
    rec = {"device": torch.cuda.get_device_name(0), "calls": args.calls,
           "case": "HU-like integers round(300 randn - 200), seg uint8: an ellipsoid of the stated share of the voxels"}
    for name, share in (("organ_2_percent", 0.02), ("half_foreground", 0.5)):
        rec[name] = one_case(lib, tuple(args.shape), share, args.calls, not args.no_host)
        torch.cuda.empty_cache()
    rec["ct_normalisation"] = normalise(lib, args.calls)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
