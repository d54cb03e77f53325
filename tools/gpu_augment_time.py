"""Time the augmentation at the reference's interpolation orders (segmamba_amd/augment.py `SplineAugmenter` on csrc/augment.hip) at
the training shape 2 x 4 x 128^3.

    python tools/gpu_augment_time.py [--calls 30] [--draws 200] [--out profiles/augment_time.json]

(a) every kernel entry stand-alone, (b) the spatial transform with both samples on (coefficients, warp, labels), blur with all 8
volumes on, low resolution with one (sample, channel) pair on at zoom 0.75 - HIP events around whole calls, the median over `--calls`
calls after warm-up, with the bytes each entry moves BY THE ALGORITHM'S COUNT (every array it must read or write, once; not a
hardware counter) - and (c) `PatchLoader.next()` from a resident case with `augment="spline"` and with `augment=True` over the same
`--draws` draws of the loader: median, minimum and maximum."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from segmamba_amd import lib as L                       # noqa: E402
from segmamba_amd import ops_raw                        # noqa: E402
from segmamba_amd import preprocess as P                # noqa: E402
from segmamba_amd.augment import SplineAugmenter        # noqa: E402
from segmamba_amd.dataloading import PatchLoader        # noqa: E402
from tests import preprocess_ref as R                   # noqa: E402
from tools.gpu_metrics_time import event_ms, kernel_split      # noqa: E402

B, C, SIDE = 2, 4, 128


def stats(ms, nbytes=None):
    out = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    if nbytes is not None:
        out["bytes_by_count"] = int(nbytes)
        out["TB_per_s_by_count"] = nbytes / (out["ms_median"] * 1e-3) / 1e12
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augment_time.json"))
    args = ap.parse_args()
    lib = L.get_lib()
    dev = "cuda"
    shape = (SIDE, SIDE, SIDE)
    nvox = SIDE ** 3
    n = B * C * nvox
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C, *shape, device=dev, generator=g)
    y = torch.randint(0, 4, (B, *shape), device=dev, generator=g)
    mats = np.stack([SplineAugmenter.matrix((0.3, -0.2, 0.45), 0.85, shape), SplineAugmenter.matrix((-0.52, 0.52, 0.1), 1.35, shape)])
    coefs = ops_raw.spline_coefs(lib, x)
    small_shape = [int(v) for v in np.round(np.asarray(shape) * 0.75).astype(int)]
    nsmall = int(np.prod(small_shape))
    small = ops_raw.zoom_nearest(lib, x[0, :1], small_shape)
    sigma = [0.5 + 0.5 * v / 7 for v in range(B * C)]
    # per axis of the in-place line kernel: the causal sweep reads and writes a line, the anti-causal sweep again
    coef_bytes = 4 * n + 8 * n + 2 * 4 * 8 * n
    rec = {"shape": [B, C, *shape], "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "coefficient_workspace_bytes": int(lib.dll.segm_spline_coefs_workspace_bytes(B, C, *shape)),
           "bytes": "by the algorithm's count from the shapes, not by a hardware counter",
           "blur": "three separable launches per call (z, y, x), neighbours served by the caches; a tiled single kernel was not measured"}
    rec["kernels_alone"] = {
        "spline_coefs": stats(event_ms(lambda: ops_raw.spline_coefs(lib, x), args.calls), coef_bytes),
        "affine_spline3": stats(event_ms(lambda: ops_raw.affine_spline3(lib, x, coefs, mats), args.calls), 8 * n + 4 * n),
        "affine_labels_int64": stats(event_ms(lambda: ops_raw.affine_labels(lib, y, mats), args.calls), 2 * 8 * B * nvox),
        "zoom_nearest_one_channel_0p75": stats(event_ms(lambda: ops_raw.zoom_nearest(lib, x[0, :1], small_shape), args.calls), 4 * nvox + 4 * nsmall),
        "gauss_blur_8_volumes": stats(event_ms(lambda: ops_raw.gauss_blur(lib, x, sigma), args.calls), 3 * 2 * 4 * n),
    }

    def spatial():
        c = ops_raw.spline_coefs(lib, x)
        return ops_raw.affine_spline3(lib, x, c, mats), ops_raw.affine_labels(lib, y, mats)

    def low_res():
        s = ops_raw.zoom_nearest(lib, x[0, :1], small_shape)
        return ops_raw.zoom(lib, s, shape, 3, True)
    rec["transforms"] = {
        "spatial_both_samples": stats(event_ms(spatial, args.calls), coef_bytes + 12 * n + 16 * B * nvox),
        "blur_all_8_volumes": rec["kernels_alone"]["gauss_blur_8_volumes"],
        "low_res_one_pair_0p75": stats(event_ms(low_res, args.calls)),
    }
    try:
        split = kernel_split(lambda: (spatial(), ops_raw.gauss_blur(lib, x, sigma), low_res()))
        rec["kernels"] = {k: {"calls": c, "us_per_call": us / c} for k, (c, us) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"
    del coefs, small

    data, seg, _ = R.brats_case()
    props = {"spacing": (1.0, 1.0, 1.0)}
    out, sout = P.preprocess_case(torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda(), props)

    class Resident:                       # one preprocessed case, as CaseDataset keeps it
        device = out.device

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"data": out, "seg": sout, "properties": props}
    loaders = {}
    for name, augment in (("plain", False), ("augment_true", True), ("augment_spline", "spline")):
        np.random.seed(0)                 # the same boxes for the three loaders
        loader = PatchLoader(Resident(), shape, batch_size=B, augment=augment)
        loaders[name] = stats(event_ms(loader.next, args.draws))
    rec["patch_loader_next"] = {"patch": list(shape), "batch": B, "draws": args.draws, **loaders}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
