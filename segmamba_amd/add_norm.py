"""Fused residual add + LayerNorm / RMSNorm: `layer_norm_fn`, `rms_norm_fn`, `RMSNorm` - the names of the reference's
mamba_ssm/ops/triton/layernorm.py (Triton kernels there, csrc/add_norm.hip here; layernorm.py:380-503 for the signatures, the return
forms and the dtype rules).

    s = x + residual (fp32)  ->  residual_out = s in the residual stream's dtype,  y = norm(s) * weight + bias in x's dtype

The input is taken as (M, N) rows.  residual_out has the residual's dtype when there is a residual; without one it is fp32 when
`residual_in_fp32` and x is not fp32, and x itself otherwise.  `prenorm` returns (y, residual_out) in x's shape.  The statistics
come from the unrounded fp32 sum, as in the reference's kernel (its `layer_norm_ref` / `rms_norm_ref` round the sum first).  The
backward returns dx, dweight in the weight's dtype, dbias, and the residual's gradient only where there was a residual.  A weight
or bias that is not fp32 is cast for the kernel (N elements) and its gradient cast back.  The residual stream is in x's dtype or in
fp32; any other pair is refused.

Tensors on the CPU take an ATen composition of the same definition (the same dtype rules, the same unrounded sum), as the losses do
for CPU tensors; tensors on the device take the HIP kernels and nothing else.

Deviations from the reference, and what is not provided:
  * the reference's `RMSNorm.forward` hands `is_rms_norm=True` to `rms_norm_fn`, which has no such parameter, and raises TypeError;
    so does its `Block` on the non-fused path with an RMSNorm.  Both work here.
  * `LayerNormLinearFn` / `layer_norm_linear_fn`, `layer_norm_ref` / `rms_norm_ref` and the language-model stack (`models/`,
    `utils/`) are not provided.
"""
from __future__ import annotations

import torch

from . import lib as L
from . import ops_raw


def _rows(t: torch.Tensor) -> torch.Tensor:
    """(..., N) -> (M, N) with a unit stride along the rows (a copy only where the view cannot be had)"""
    t = t.reshape(-1, t.shape[-1])
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t


def _compute_dtype(t: torch.Tensor) -> torch.dtype:
    return torch.float64 if t.dtype == torch.float64 else torch.float32


def _fwd_aten(x, weight, bias, residual, eps, rms, residual_dtype):
    """the ATen composition of add_norm_fwd for CPU tensors -> (y, mean, rstd, residual_out)"""
    ct = _compute_dtype(x)
    s = x.to(ct)
    if residual is not None:
        s = s + residual.to(ct)
        residual_dtype = residual.dtype
    residual_out = None
    if residual is not None or (residual_dtype is not None and residual_dtype != x.dtype):
        residual_out = s.to(residual_dtype)
    mean = None
    centred = s
    if not rms:
        mean = s.mean(dim=-1)
        centred = s - mean[:, None]
    rstd = 1.0 / torch.sqrt(centred.square().mean(dim=-1) + eps)
    y = centred * rstd[:, None] * weight.to(ct)
    if bias is not None:
        y = y + bias.to(ct)
    return y.to(x.dtype), mean, rstd, residual_out


def _bwd_aten(dy, saved, weight, mean, rstd, dresidual, has_residual, has_bias, rms):
    """the ATen composition of add_norm_bwd for CPU tensors -> (dx, dweight, dbias, dresidual_in)"""
    ct = _compute_dtype(dy)
    xs, g = saved.to(ct), dy.to(ct)
    xhat = xs * rstd[:, None] if rms else (xs - mean[:, None]) * rstd[:, None]
    wdy = g * weight.to(ct)
    inner = xhat * (xhat * wdy).mean(dim=-1, keepdim=True)
    if not rms:
        inner = inner + wdy.mean(dim=-1, keepdim=True)
    dx = (wdy - inner) * rstd[:, None]
    if dresidual is not None:
        dx = dx + dresidual.to(ct)
    dweight = (g * xhat).sum(dim=0)
    dbias = g.sum(dim=0) if has_bias else None
    out = dx.to(dy.dtype)
    dresidual_in = None
    if has_residual:
        dresidual_in = out if saved.dtype == dy.dtype else dx.to(saved.dtype)
    return out, dweight, dbias, dresidual_in


class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
        shape = x.shape
        x2 = _rows(x)
        r2 = None
        if residual is not None:
            if residual.shape != shape:
                raise RuntimeError(f"layer_norm_fn: the residual has shape {tuple(residual.shape)}, x {tuple(shape)}")
            r2 = _rows(residual)
        residual_dtype = r2.dtype if r2 is not None else (torch.float32 if residual_in_fp32 else None)
        if residual_dtype is not None and residual_dtype not in (x2.dtype, torch.float32):
            raise RuntimeError(f"layer_norm_fn: a residual stream in {x2.dtype} or fp32 is supported, got {residual_dtype}")
        if L.on_device(x2):
            w32 = weight.detach().float().contiguous()
            b32 = bias.detach().float().contiguous() if bias is not None else None
            y, mean, rstd, residual_out = ops_raw.add_norm_fwd(L.get_lib(), x2, w32, b32, r2, eps, is_rms_norm, residual_dtype)
        else:
            y, mean, rstd, residual_out = _fwd_aten(x2, weight.detach(), None if bias is None else bias.detach(), r2, eps,
                                                   is_rms_norm, residual_dtype)
        if residual_out is None:
            residual_out = x2
        ctx.save_for_backward(residual_out, weight, bias, mean, rstd)
        ctx.shape, ctx.rms, ctx.has_residual, ctx.prenorm = shape, is_rms_norm, residual is not None, prenorm
        y = y.reshape(shape)
        return y if not prenorm else (y, residual_out.reshape(shape))

    @staticmethod
    def backward(ctx, dy, *more):
        saved, weight, bias, mean, rstd = ctx.saved_tensors
        dy2 = _rows(dy)
        dresidual = _rows(more[0]) if ctx.prenorm else None
        if L.on_device(dy2):
            dx, dweight, dbias, dresidual_in = ops_raw.add_norm_bwd(
                L.get_lib(), dy2, saved, weight.detach().float().contiguous(), mean, rstd, dresidual, ctx.has_residual,
                bias is not None, ctx.rms)
        else:
            dx, dweight, dbias, dresidual_in = _bwd_aten(dy2, saved, weight.detach(), mean, rstd, dresidual, ctx.has_residual,
                                                         bias is not None, ctx.rms)
        return (dx.reshape(ctx.shape), dweight.to(weight.dtype), None if dbias is None else dbias.to(bias.dtype),
                dresidual_in.reshape(ctx.shape) if ctx.has_residual else None, None, None, None, None)


def layer_norm_fn(x, weight, bias, residual=None, eps=1e-6, prenorm=False, residual_in_fp32=False, is_rms_norm=False):
    return LayerNormFn.apply(x, weight, bias, residual, eps, prenorm, residual_in_fp32, is_rms_norm)


def rms_norm_fn(x, weight, bias, residual=None, prenorm=False, residual_in_fp32=False, eps=1e-6):
    return LayerNormFn.apply(x, weight, bias, residual, eps, prenorm, residual_in_fp32, True)


class RMSNorm(torch.nn.Module):
    def __init__(self, hidden_size, eps=1e-5, device=None, dtype=None):
        super().__init__()
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.empty(hidden_size, device=device, dtype=dtype))
        self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        torch.nn.init.ones_(self.weight)

    def forward(self, x, residual=None, prenorm=False, residual_in_fp32=False):
        return rms_norm_fn(x, self.weight, self.bias, residual=residual, prenorm=prenorm, residual_in_fp32=residual_in_fp32,
                           eps=self.eps)
