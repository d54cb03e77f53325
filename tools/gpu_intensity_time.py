"""Time the intensity transforms of the augmentation - noise, brightness, contrast, the two gammas, the mirror - on the kernels of
csrc/intensity.hip (`FusedAugmenter`) against the ATen route they replace (`SplineAugmenter`), at the training shape 2 x 4 x 128^3.

    python tools/gpu_intensity_time.py [--calls 30] [--draws 200] [--out profiles/intensity_time.json]

(a) each transform forced on alone (every other coin off), brightness plus contrast, both gammas, the mirror on all axes, the six
together and all twelve coins together: HIP events around whole augmenter calls, the two routes alternating in one loop, the median
over `--calls` calls after warm-up; (b) per configuration the kernels of one call of each route from the profiler (a separate call,
after the timing): launches, microseconds, and for the new kernels the bytes BY THE ALGORITHM'S COUNT (every array a pass must read
or write, once; not a hardware counter) over their time; (c) the peak of allocated bytes of one call above what was allocated
before it; (d) `PatchLoader.next()` from a resident case with `augment="fused"` and with `augment="spline"` over the same `--draws`
draws of the loader, alternating."""
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
from segmamba_amd import preprocess as P                # noqa: E402
from segmamba_amd.augment import FusedAugmenter, SplineAugmenter      # noqa: E402
from segmamba_amd.dataloading import PatchLoader        # noqa: E402
from tests import preprocess_ref as R                   # noqa: E402
from tools.gpu_metrics_time import kernel_split         # noqa: E402

B, C, SIDE = 2, 4, 128
SIX = ("noise", "brightness", "contrast", "gamma_inverted", "gamma", "mirror")
TWELVE = ("rotation", "scale", "blur", "blur_channel", "lowres", "lowres_channel") + SIX
CONFIGS = [("noise", ("noise",)), ("brightness", ("brightness",)), ("contrast", ("contrast",)),
           ("brightness_contrast", ("brightness", "contrast")), ("gamma_inverted", ("gamma_inverted",)), ("gamma", ("gamma",)),
           ("both_gammas", ("gamma_inverted", "gamma")), ("mirror_all_axes", ("mirror",)), ("six_together", SIX),
           ("all_twelve_coins", TWELVE)]


def forced(cls):
    class Forced(cls):
        """the coins of the named transforms always fall on, every other coin off"""

        def __init__(self, *a, force=(), **kw):
            super().__init__(*a, **kw)
            self.force = tuple(force)

        def _coin(self, name, p, *shape):
            super()._coin(name, p, *shape)
            return np.full(shape, name in self.force, dtype=bool)
    return Forced


def stats(ms):
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def alternate_ms(fns, calls, warmup=5):
    """the callables timed in turn, call by call -> one list of milliseconds each"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(calls):
        for fn, ms in zip(fns, out):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
    return out


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def split_record(fn, name):
    """the kernels of one call: launches in all, and per kernel calls and microseconds; for the kernels of csrc/intensity.hip the bytes
    by the algorithm's count over the time (all 8 planes are on in every configuration)"""
    n = B * C * SIDE ** 3
    try:
        split = kernel_split(fn)
    except Exception as exc:                  # the split is a record, not a result: say why it is missing
        return {"unavailable": f"{type(exc).__name__}: {exc}"}
    kernels = {}
    for key, (count, us) in sorted(split.items(), key=lambda kv: -kv[1][1]):
        row = {"calls": count, "us_per_call": us / count}
        nbytes = None
        if "in_stats_kernel" in key:
            nbytes = 4 * n                                               # one read of the planes
        elif "in_apply_kernel" in key and name in ("noise", "brightness", "contrast", "brightness_contrast", "gamma_inverted", "gamma",
                                                   "both_gammas", "mirror_all_axes"):
            nbytes = (12 if name == "noise" else 8) * n                  # read, write, and the noise field
        if nbytes is not None:
            row["bytes_by_count"] = nbytes
            row["TB_per_s_by_count"] = nbytes / (us / count * 1e-6) / 1e12
        kernels[key] = row
    return {"launches": sum(r["calls"] for r in kernels.values()), "device_us": sum(r["calls"] * r["us_per_call"] for r in kernels.values()),
            "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--draws", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intensity_time.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    L.get_lib()
    dev = "cuda"
    shape = (SIDE, SIDE, SIDE)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(B, C, *shape, device=dev, generator=g)
    y = torch.randint(0, 4, (B, *shape), device=dev, generator=g)
    rec = {"shape": [B, C, *shape], "device": torch.cuda.get_device_name(0), "calls": args.calls,
           "bytes": "by the algorithm's count from the shapes, not by a hardware counter; a pass over the batch reads 67 MB",
           "routes": {"aten": "SplineAugmenter", "kernels": "FusedAugmenter"},
           "timing": "HIP events around whole augmenter calls, the two routes alternating call by call; medians"}
    SplineForced, FusedForced = forced(SplineAugmenter), forced(FusedAugmenter)
    rec["transforms"] = {}
    for name, force in CONFIGS:
        aten, fused = SplineForced(dev, seed=5, force=force), FusedForced(dev, seed=5, force=force)
        ms_aten, ms_fused = alternate_ms([lambda: aten(x, y), lambda: fused(x, y)], args.calls)
        row = {"aten": stats(ms_aten), "kernels": stats(ms_fused)}
        row["aten_over_kernels"] = row["aten"]["ms_median"] / row["kernels"]["ms_median"]
        row["aten"]["peak_allocated_bytes"] = peak_bytes(lambda: aten(x, y))
        row["kernels"]["peak_allocated_bytes"] = peak_bytes(lambda: fused(x, y))
        row["aten"]["split"] = split_record(lambda: aten(x, y), name)
        row["kernels"]["split"] = split_record(lambda: fused(x, y), name)
        rec["transforms"][name] = row
        print(name, json.dumps({k: row[k]["ms_median"] for k in ("aten", "kernels")}), flush=True)
        with open(args.out, "w") as f:        # what has been measured so far survives a later failure
            json.dump(rec, f, indent=1)

    data, seg, _ = R.brats_case()
    props = {"spacing": (1.0, 1.0, 1.0)}
    out, sout = P.preprocess_case(torch.from_numpy(data).cuda(), torch.from_numpy(seg).cuda(), props)

    class Resident:                           # one preprocessed case, as CaseDataset keeps it
        device = out.device

        def __len__(self):
            return 1

        def __getitem__(self, i):
            return {"data": out, "seg": sout, "properties": props}
    loaders = []
    for augment in ("spline", "fused"):
        loaders.append(PatchLoader(Resident(), shape, batch_size=B, augment=augment))
    states = [None, None]

    def turn(i):
        def run():                            # each loader continues its own stream of np.random draws: the same boxes for both
            if states[i] is not None:
                np.random.set_state(states[i])
            loaders[i].next()
            states[i] = np.random.get_state()
        return run
    np.random.seed(0)
    states[0] = states[1] = np.random.get_state()
    ms_spline, ms_fused = alternate_ms([turn(0), turn(1)], args.draws)
    rec["patch_loader_next"] = {"patch": list(shape), "batch": B, "draws": args.draws, "augment_spline": stats(ms_spline),
                                "augment_fused": stats(ms_fused)}
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["patch_loader_next"]))


if __name__ == "__main__":
    main()
