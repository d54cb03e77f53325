"""Golden fixture of the fused add + LayerNorm / RMSNorm, generated from the REFERENCE's own code (build container only: needs
/root/reference).

    python tests/golden/make_golden_add_norm.py

add_norm.npz:
  * the reference's `layer_norm_ref` / `rms_norm_ref` (mamba_ssm/ops/triton/layernorm.py:19-48) on float64 CPU tensors with
    upcast=False, so every step is float64: M x N in {3 x 7, 5 x 48, 4 x 100} x {LayerNorm, RMS} x with / without residual x
    prenorm x with / without bias.  The inputs of a shape (s<i>.x, .residual, .w, .b, .dy, .dres) are shared by its cases; a case
    s<i>.<ln|rms>.r<0|1>.p<0|1>.b<0|1> records y, res_out (prenorm), and the gradients dx, dres_in (residual), dw, db (bias) that
    torch.autograd.grad gives for the recorded dy and (prenorm) dres.
  * the reference's `Block(fused_add_norm=False, norm_cls=nn.LayerNorm)` (mamba_simple.py:445-501) with residual_in_fp32 both ways,
    float64 on the CPU, two blocks chained around the stub mixer below: blk.h0, blk.dh, blk.dr and the parameters blk<j>.*; per
    flag blk.f<0|1>.h, .r (the outputs of the second block) and the gradients .dh0, .dnw<j>, .dnb<j>, .dW<j>.
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402

SHAPES = ((3, 7), (5, 48), (4, 100))
EPS = 1e-5
BLOCK_DIM, BLOCK_BATCH, BLOCK_LEN = 48, 2, 5


class StubMixer(nn.Module):
    """tanh(x W^T + b): the stand-in for a Mamba mixer (tests/add_norm_checks.py holds the same definition)"""

    def __init__(self, dim):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(dim, dim))
        self.b = nn.Parameter(torch.zeros(dim))

    def forward(self, x, inference_params=None):
        return torch.tanh(x @ self.W.to(x.dtype).t() + self.b.to(x.dtype))


def main():
    _, _, ms = load_reference()
    from mamba_ssm.ops.triton.layernorm import layer_norm_ref, rms_norm_ref
    g = torch.Generator().manual_seed(11)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)   # noqa: E731
    arrs = {"shapes": np.array(SHAPES, dtype=np.int64), "eps": np.float64(EPS)}
    for i, (M, N) in enumerate(SHAPES):
        base = {"x": rnd(M, N), "residual": rnd(M, N), "w": 1.0 + 0.3 * rnd(N), "b": 0.5 * rnd(N), "dy": rnd(M, N), "dres": rnd(M, N)}
        for k, v in base.items():
            arrs[f"s{i}.{k}"] = v
        for norm, fn in (("ln", layer_norm_ref), ("rms", rms_norm_ref)):
            for has_res in (0, 1):
                for prenorm in (0, 1):
                    for has_b in (0, 1):
                        x, w = base["x"].clone().requires_grad_(), base["w"].clone().requires_grad_()
                        r = base["residual"].clone().requires_grad_() if has_res else None
                        b = base["b"].clone().requires_grad_() if has_b else None
                        out = fn(x, w, b, residual=r, eps=EPS, prenorm=bool(prenorm), upcast=False)
                        outs, grads = ((out[0], out[1]), (base["dy"], base["dres"])) if prenorm else ((out,), (base["dy"],))
                        if prenorm and not has_res:
                            outs = (out[0], out[1] * 1.0)     # the reference hands x itself back: a node of its own for autograd.grad
                        wrt = [t for t in (x, w, r, b) if t is not None]
                        got = dict(zip([n for n, t in zip(("dx", "dw", "dres_in", "db"), (x, w, r, b)) if t is not None],
                                       torch.autograd.grad(outs, wrt, grads)))
                        key = f"s{i}.{norm}.r{has_res}.p{prenorm}.b{has_b}."
                        arrs[key + "y"] = outs[0]
                        if prenorm:
                            arrs[key + "res_out"] = outs[1]
                        for n, t in got.items():
                            arrs[key + n] = t

    # two chained reference Blocks, non-fused, LayerNorm
    D = BLOCK_DIM
    params = []
    for j in range(2):
        params.append({"norm.weight": 1.0 + 0.2 * rnd(D), "norm.bias": 0.3 * rnd(D), "mix.W": rnd(D, D) / np.sqrt(D), "mix.b": 0.1 * rnd(D)})
        for k, v in params[j].items():
            arrs[f"blk{j}.{k}"] = v
    h0, dh, dr = rnd(BLOCK_BATCH, BLOCK_LEN, D), rnd(BLOCK_BATCH, BLOCK_LEN, D), rnd(BLOCK_BATCH, BLOCK_LEN, D)
    arrs.update({"blk.h0": h0, "blk.dh": dh, "blk.dr": dr})
    for f32 in (0, 1):
        blocks = []
        for j in range(2):
            blk = ms.Block(D, StubMixer, norm_cls=lambda d: nn.LayerNorm(d, eps=EPS), fused_add_norm=False,
                           residual_in_fp32=bool(f32)).double()
            with torch.no_grad():
                blk.norm.weight.copy_(params[j]["norm.weight"])
                blk.norm.bias.copy_(params[j]["norm.bias"])
                blk.mixer.W.copy_(params[j]["mix.W"])
                blk.mixer.b.copy_(params[j]["mix.b"])
            blocks.append(blk)
        x = h0.clone().requires_grad_()
        h, r = blocks[0](x)
        h, r = blocks[1](h, r)
        wrt = [x] + [p for blk in blocks for p in (blk.norm.weight, blk.norm.bias, blk.mixer.W)]
        grads = torch.autograd.grad((h, r), wrt, (dh, dr.to(r.dtype)))
        key = f"blk.f{f32}."
        arrs[key + "h"], arrs[key + "r"], arrs[key + "dh0"] = h, r, grads[0]
        for j in range(2):
            arrs[key + f"dnw{j}"], arrs[key + f"dnb{j}"], arrs[key + f"dW{j}"] = grads[1 + 3 * j: 4 + 3 * j]
    out = os.path.join(HERE, "add_norm.npz")
    np.savez_compressed(out, **{k: (v.detach().numpy() if torch.is_tensor(v) else v) for k, v in arrs.items()})
    print("wrote add_norm.npz:", len(arrs), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
