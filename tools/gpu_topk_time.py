"""Time TopKLoss (segmamba_amd/losses.py on csrc/topk_ce.hip) at training size: logits 2 x 4 x 128^3 in bf16 and in fp32, k = 10, every
7th voxel ignored.

    python tools/gpu_topk_time.py [--calls 30] [--out profiles/topk_time.json]

Per dtype, in a process of its own under its own time limit (the parent opens no GPU and stops at the first step that fails):
(a) `TopKLoss` forward + backward as a whole;
(b) the entries on their own - the map, the selection, the backward with the top-k weight - each with the bytes it moves by the
    algorithm's count (not a hardware counter) and the resulting TB/s, to set against the 5 - 6 TB/s copy rate of the library's
    streaming kernels.  With n voxels, C classes and e bytes per logit: the map reads C e n + 8 n (labels) and writes 4 n; the selection
    reads the 4 n of the map four times (three histogram passes, one for the sum); the backward reads C e n + 8 n + 4 n and writes C e n;
(c) the kernel split of one forward + backward from the profiler;
(d) ATen's route on the device: `F.cross_entropy(logits.float(), reduction="none")`, `torch.topk`, the mean, backward.
HIP events around whole calls, the median over `--calls` calls after warm-up."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, CLASSES, K = (2, 128, 128, 128), 4, 10
STEP_LIMIT_S = 240


def step(dtype_name, calls):
    import torch
    import torch.nn.functional as F

    from segmamba_amd import lib as L, losses, ops_raw
    from tools.gpu_metrics_time import event_ms, kernel_split
    from tools.gpu_preprocess_time import stats, with_rate

    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype_name]
    lib = L.get_lib()
    g = torch.Generator(device="cuda").manual_seed(31)
    logits = (2.0 * torch.randn((SHAPE[0], CLASSES) + SHAPE[1:], generator=g, device="cuda")).to(dtype)
    labels = torch.randint(0, CLASSES, SHAPE, generator=g, device="cuda")
    labels.view(-1)[::7] = CLASSES
    n, e = labels.numel(), logits.element_size()
    kk = int(n * K / 100)
    fn = losses.TopKLoss(k=K, ignore_index=CLASSES)
    target = labels.unsqueeze(1).float()

    def whole():
        x = logits.detach().requires_grad_(True)
        loss = fn(x, target)
        loss.backward()
        return loss.detach(), x.grad

    def aten():
        x = logits.detach().requires_grad_(True)
        res = F.cross_entropy(x.float(), labels, ignore_index=CLASSES, reduction="none")
        loss = torch.topk(res.view(-1), kk, sorted=False)[0].mean()
        loss.backward()
        return loss.detach(), x.grad

    lmap = ops_raw.cross_entropy_map(lib, logits, labels, CLASSES)
    sel = ops_raw.topk_select(lib, lmap.view(-1), kk)
    ws = torch.empty(lib.dll.segm_topk_select_workspace_bytes(n) // 8 + 1, dtype=torch.int64, device="cuda")
    one = torch.ones(1, device="cuda")
    rec = {"dtype": dtype_name, "shape": list(SHAPE), "classes": CLASSES, "k": K, "voxels": n, "kk": kk,
           "device": torch.cuda.get_device_name(0)}
    (l1, g1), (l2, g2) = whole(), aten()
    rec["loss"], rec["loss_aten"] = float(l1), float(l2)
    rec["max_gradient_difference_to_aten"] = float((g1.float() - g2.float()).abs().max())
    rec["topk_loss_forward_backward"] = stats(event_ms(whole, calls))
    rec["parts"] = {
        "cross_entropy_map": with_rate(event_ms(lambda: ops_raw.cross_entropy_map(lib, logits, labels, CLASSES), calls),
                                       n * (CLASSES * e + 8 + 4)),
        "topk_select": with_rate(event_ms(lambda: ops_raw.topk_select(lib, lmap.view(-1), kk, ws), calls), 4 * 4 * n),
        "cross_entropy_map_bwd": with_rate(event_ms(lambda: ops_raw.cross_entropy_map_bwd(lib, logits, labels, CLASSES, scale=one, loss_map=lmap,
                                                                                          select=sel, kk=kk), calls),
                                           n * (2 * CLASSES * e + 8 + 4)),
    }
    try:
        split = kernel_split(whole)
        rec["kernels"] = {k: {"calls": c, "us_per_call": us / c} for k, (c, us) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"
    rec["aten_cross_entropy_topk_backward"] = stats(event_ms(aten, max(3, calls // 3)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_time.json"))
    ap.add_argument("--step", choices=("bf16", "fp32"), help="run one step in this process and print its record")
    args = ap.parse_args()
    if args.step:
        print("RECORD " + json.dumps(step(args.step, args.calls)))
        return 0
    out = {"tool": "tools/gpu_topk_time.py", "calls": args.calls, "steps": []}
    for name in ("bf16", "fp32"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(args.calls)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"step {name}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            print(f"step {name}: exit status {r.returncode}; stopping\n{r.stderr[-3000:]}", file=sys.stderr)
            return 1
        out["steps"].append(json.loads(lines[-1][len("RECORD "):]))
        print(json.dumps(out["steps"][-1], indent=1), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
