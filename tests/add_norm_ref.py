"""Float64 restatement of the fused add + LayerNorm / RMSNorm contract (include/segmamba_hip.h, csrc/add_norm.hip), forward and
backward in closed form, on torch tensors of any device.  TEST INFRASTRUCTURE ONLY: tests/test_add_norm_cpu.py holds it to the
recorded reference results (tests/golden/add_norm.npz) at 1e-12 relative, so it is tied to the reference and not to the kernels.

The inputs are taken as they are stored (already rounded to their dtype).  The one fp32 step of the contract is the sum
s = float(x) + float(residual): it is formed in `sum_dtype` (fp32 for the kernels, float64 against the float64 fixture) and
everything after it is float64."""
import torch


def forward(x, weight, bias=None, residual=None, eps=1e-6, rms=False, sum_dtype=torch.float32):
    """-> (y, s, mean, rstd) in float64: y (M, N) before its rounding, s the sum that residual_out rounds, mean (zeros for rms)
    and rstd (M,)"""
    s = x.to(sum_dtype)
    if residual is not None:
        s = s + residual.to(sum_dtype)
    s = s.double()
    if rms:
        mean = torch.zeros(s.shape[0], dtype=torch.float64, device=s.device)
        var = (s * s).mean(dim=-1)
    else:
        mean = s.mean(dim=-1)
        var = ((s - mean[:, None]) ** 2).mean(dim=-1)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (s - mean[:, None]) * rstd[:, None] * weight.double()
    if bias is not None:
        y = y + bias.double()
    return y, s, mean, rstd


def backward(dy, x_saved, weight, mean, rstd, dresidual=None, rms=False):
    """-> (dx, dweight, dbias) in float64; x_saved is the row the forward kept (residual_out as it was rounded, or x), dx the value
    that both dx and dresidual_in round"""
    g, xs, w = dy.double(), x_saved.double(), weight.double()
    xhat = (xs - mean.double()[:, None]) * rstd.double()[:, None]
    wdy = g * w
    inner = xhat * (xhat * wdy).mean(dim=-1, keepdim=True)
    if not rms:
        inner = inner + wdy.mean(dim=-1, keepdim=True)
    dx = (wdy - inner) * rstd.double()[:, None]
    if dresidual is not None:
        dx = dx + dresidual.double()
    return dx, (g * xhat).sum(dim=0), g.sum(dim=0)
