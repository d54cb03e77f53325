"""Time DC_and_CE_loss(device_sums=True) (segmamba_amd/losses.py on csrc/dice_ce.hip) at training size: logits 2 x 4 x 128^3 in bf16
and in fp32, int64 labels, every 7th voxel ignored.

    python tools/gpu_dice_ce_time.py [--calls 30] [--out profiles/dice_ce_time.json]

Per dtype, in a process of its own under its own time limit (the parent opens no GPU and stops at the first step that fails):
(a) `DC_and_CE_loss(..., ignore_label=4, device_sums=True)` forward + backward as a whole, with its peak allocated bytes;
(b) the two entries on their own, each with the bytes it moves by the algorithm's count (not a hardware counter) and the resulting
    TB/s, to set against the 5 - 6 TB/s copy rate of the library's streaming kernels.  With n voxels, C classes and e bytes per
    logit: the forward reads C e n + 8 n (labels); the backward reads the same and writes C e n;
(c) the kernel split of one forward + backward from the profiler;
(d) the ATen formulation of the same loss on the same device - `_sums_aten`'s formulas (fp32 softmax, one-hot by comparison, the
    masked products and sums, logsumexp - x_y) followed by the same `from_sums` - forward + backward, with its peak allocated bytes.
HIP events around whole calls, the median over `--calls` calls after warm-up."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE, CLASSES, IGNORE = (2, 128, 128, 128), 4, 4
STEP_LIMIT_S = 240


def step(dtype_name, calls):
    import torch

    from segmamba_amd import lib as L, losses, ops_raw
    from tools.gpu_metrics_time import event_ms, kernel_split
    from tools.gpu_preprocess_time import stats, with_rate

    dtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype_name]
    lib = L.get_lib()
    g = torch.Generator(device="cuda").manual_seed(35)
    logits = (2.0 * torch.randn((SHAPE[0], CLASSES) + SHAPE[1:], generator=g, device="cuda")).to(dtype)
    labels = torch.randint(0, CLASSES, SHAPE, generator=g, device="cuda")
    labels.view(-1)[::7] = IGNORE
    n, e = labels.numel(), logits.element_size()
    dice_kw = dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False)
    fn = losses.DC_and_CE_loss(dice_kw, {}, ignore_label=IGNORE, device_sums=True)
    host = losses.DC_and_CE_loss(dice_kw, {}, ignore_label=IGNORE)             # for from_sums and the weights only

    def whole():
        x = logits.detach().requires_grad_(True)
        loss = fn(x, labels)
        loss.backward()
        return loss.detach(), x.grad

    def aten():
        x = logits.detach().requires_grad_(True)
        inter, pred, gt, ce_sum, count = losses._sums_aten(x, labels, None, IGNORE, losses.softmax_helper_dim1)
        loss = ce_sum.sum() / count.sum().clamp(min=1) + host.dc.from_sums(inter, pred, gt)
        loss.backward()
        return loss.detach(), x.grad

    def peak(f):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = f()
        torch.cuda.synchronize()
        del out
        return int(torch.cuda.max_memory_allocated() - base)

    ws = torch.empty(lib.dll.segm_softmax_dice_workspace_bytes(SHAPE[0], CLASSES, n // SHAPE[0]) // 8, dtype=torch.float64, device="cuda")
    coef = [torch.full((SHAPE[0], CLASSES), v, device="cuda") for v in (1e-6, -1e-6)] + [torch.full((SHAPE[0],), 1e-7, device="cuda")]
    rec = {"dtype": dtype_name, "shape": list(SHAPE), "classes": CLASSES, "voxels": n, "ignored_every": 7,
           "device": torch.cuda.get_device_name(0)}
    (l1, g1), (l2, g2) = whole(), aten()
    rec["loss"], rec["loss_aten"] = float(l1), float(l2)
    rec["max_gradient_difference_to_aten"] = float((g1.float() - g2.float()).abs().max())
    rec["max_gradient_aten"] = float(g2.float().abs().max())
    del g1, g2
    rec["peak_bytes"] = peak(whole)
    rec["peak_bytes_aten"] = peak(aten)
    rec["logits_bytes"] = logits.numel() * e
    rec["dc_and_ce_forward_backward"] = stats(event_ms(whole, calls))
    rec["parts"] = {
        "softmax_dice_fwd": with_rate(event_ms(lambda: ops_raw.softmax_dice_fwd(lib, logits, labels, None, IGNORE, workspace=ws), calls),
                                      n * (CLASSES * e + 8)),
        "softmax_dice_bwd": with_rate(event_ms(lambda: ops_raw.softmax_dice_bwd(lib, logits, labels, *coef, ignore_label=IGNORE), calls),
                                      n * (2 * CLASSES * e + 8)),
    }
    try:
        split = kernel_split(whole)
        rec["kernels"] = {k: {"calls": c, "us_per_call": us / c} for k, (c, us) in sorted(split.items(), key=lambda kv: -kv[1][1])}
    except Exception as exc:              # the split is a record, not a result: say why it is missing
        rec["kernels"] = f"unavailable: {type(exc).__name__}: {exc}"
    rec["aten_forward_backward"] = stats(event_ms(aten, max(3, calls // 3)))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dice_ce_time.json"))
    ap.add_argument("--step", choices=("bf16", "fp32"), help="run one step in this process and print its record")
    args = ap.parse_args()
    if args.step:
        print("RECORD " + json.dumps(step(args.step, args.calls)))
        return 0
    out = {"tool": "tools/gpu_dice_ce_time.py", "calls": args.calls, "steps": []}
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
