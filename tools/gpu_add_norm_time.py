"""Time the fused add + LayerNorm / RMSNorm entries (csrc/add_norm.hip through segmamba_amd.ops_raw) against the ATen composition of
the same definition on the same device.

    python tools/gpu_add_norm_time.py [--calls 30] [--out profiles/add_norm_time.json]

Shapes M x N: 524288 x 48, 65536 x 96, 8192 x 192, 1024 x 384 (SegMamba's four token shapes at 2 x 128^3) and 524288 x 768.  Per
shape, in a process of its own under its own time limit (the parent opens no GPU and stops at the first step that fails): bf16 x
with a bf16 residual and with an fp32 residual, LayerNorm and RMS, forward and backward.  HIP events around whole calls, the library
and ATen alternating call by call, the median over `--calls` calls after warm-up.
  * library forward   ops_raw.add_norm_fwd: reads x and the residual, writes y and residual_out
  * library backward  ops_raw.add_norm_bwd: reads residual_out, dy and dresidual, writes dx (and dresidual_in for an fp32 stream)
  * ATen forward      s = x.float() + residual.float(); residual_out = s.to(.); F.layer_norm(s, ...) or s * rsqrt(mean(s^2) + eps)
                      * w; .to(x.dtype)
  * ATen backward     torch.autograd.grad of that graph for the same dy and dresidual
Bytes are the algorithm's count for the library's entry (not a hardware counter), e and r the element sizes of x and of the residual
stream: forward M N (2 e + 2 r), backward M N (2 e + 2 r) with a stream in x's dtype (dresidual_in is dx) and M N (2 e + 3 r) with
an fp32 one; the resulting TB/s stand against the 5 - 6 TB/s copy rate of the library's streaming kernels."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((524288, 48), (65536, 96), (8192, 192), (1024, 384), (524288, 768))
STEP_LIMIT_S = 240
EPS = 1e-5


def alternate(fa, fb, calls, warmup=3):
    """event times of fa and fb in milliseconds, the two alternating call by call"""
    import torch
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(calls):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b))
    return out


def step(index, calls):
    import torch
    import torch.nn.functional as F

    from segmamba_amd import lib as L, ops_raw
    from tools.gpu_preprocess_time import stats, with_rate

    lib = L.get_lib()
    M, N = SHAPES[index]
    g = torch.Generator(device="cuda").manual_seed(17)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")      # noqa: E731
    x, dy = rnd(M, N).to(torch.bfloat16), rnd(M, N).to(torch.bfloat16)
    w, b = 1 + 0.1 * rnd(N), 0.1 * rnd(N)
    rec = {"rows": M, "cols": N, "dtype": "bf16", "device": torch.cuda.get_device_name(0), "cases": []}
    for rdt_name, rdt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        res, dres = rnd(M, N).to(rdt), rnd(M, N).to(rdt)
        e, r = 2, res.element_size()
        for rms in (False, True):
            bias = None if rms else b

            def aten_graph():
                xg, rg = x.detach().requires_grad_(), res.detach().requires_grad_()
                s = xg.float() + rg.float()
                if rms:
                    y = (s * torch.rsqrt(s.square().mean(-1, keepdim=True) + EPS) * w).to(x.dtype)
                else:
                    y = F.layer_norm(s, (N,), w, b, EPS).to(x.dtype)
                return xg, rg, y, s.to(rdt)

            y, mean, rstd, res_out = ops_raw.add_norm_fwd(lib, x, w, bias, res, EPS, rms)
            xg, rg, y_aten, out_aten = aten_graph()
            case = {"residual": rdt_name, "norm": "rms" if rms else "layernorm",
                    "max_y_difference_to_aten": float((y.float() - y_aten.float()).abs().max())}
            ours, aten = alternate(lambda: ops_raw.add_norm_fwd(lib, x, w, bias, res, EPS, rms), aten_graph, calls)
            case["forward"] = with_rate(ours, M * N * (2 * e + 2 * r))
            case["forward_aten"] = stats(aten)
            ours, aten = alternate(
                lambda: ops_raw.add_norm_bwd(lib, dy, res_out, w, mean, rstd, dres, True, bias is not None, rms),
                lambda: torch.autograd.grad((y_aten, out_aten), (xg, rg), (dy, dres), retain_graph=True), calls)
            case["backward"] = with_rate(ours, M * N * (2 * e + (3 if r == 4 else 2) * r))
            case["backward_aten"] = stats(aten)
            rec["cases"].append(case)
            del y, mean, rstd, res_out, xg, rg, y_aten, out_aten
        del res, dres
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "add_norm_time.json"))
    ap.add_argument("--step", type=int, help="run the shape of this index in this process and print its record")
    args = ap.parse_args()
    if args.step is not None:
        print("RECORD " + json.dumps(step(args.step, args.calls)))
        return 0
    out = {"tool": "tools/gpu_add_norm_time.py", "calls": args.calls, "steps": []}
    for i, shape in enumerate(SHAPES):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(i), "--calls", str(args.calls)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print(f"step {shape}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
            return 1
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RECORD ")]
        if r.returncode != 0 or not lines:
            print(f"step {shape}: exit status {r.returncode}; stopping\n{r.stderr[-3000:]}", file=sys.stderr)
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
