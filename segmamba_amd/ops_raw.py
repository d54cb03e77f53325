"""Thin, allocation-owning wrappers around the C ABI: tensors in, tensors out, no autograd.

Every function takes the loaded library first so that the *same* marshalling code is exercised by
the product (`lib.get_lib()`, the HIP build) and by the CPU-emulation build the tests use to check
kernel logic without a GPU.  Layout is chosen per call:

  channel_last=True   u, delta, z, out ... are (B, L, D); B / C are (B, L, N) or (B, L, G, N)
  channel_last=False  the reference's layout: (B, D, L); B / C are (B, N, L) or (B, G, N, L)
                      (mamba/mamba_ssm/ops/selective_scan_interface.py:31-36)

Error behaviour mirrors the reference's TORCH_CHECKs (selective_scan.cpp:233-303,
causal_conv1d.cpp:136-170): shape / dtype / stride problems raise RuntimeError.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import os

import numpy as np

import torch

from . import lib as L


def _shape_bld(t: torch.Tensor, channel_last: bool):
    b, x, y = t.shape
    return (b, x, y) if channel_last else (b, y, x)        # -> (batch, seqlen, dim)


def _bc4(t: torch.Tensor, channel_last: bool) -> torch.Tensor:
    if t.dim() == 3:
        return t.unsqueeze(2) if channel_last else t.unsqueeze(1)
    if t.dim() != 4:
        raise RuntimeError("B / C must have 3 or 4 dimensions (input-dependent B and C only)")
    return t


def _check_seq(name, t, ref, dtype):
    if t is None:
        return
    if t.shape != ref.shape:
        raise RuntimeError(f"{name} must have shape {tuple(ref.shape)}, got {tuple(t.shape)}")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if t.device != ref.device:
        raise RuntimeError(f"{name} must be on {ref.device}")


def _check_vec(name, t, n, dev):
    if t is None:
        return
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32")
    if t.numel() != n or not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous with {n} elements")
    if t.device != dev:
        raise RuntimeError(f"{name} must be on {dev}")


def _fill_scan_args(a: L.ScanFwdArgs, u, delta, A, B, C, D, z, delta_bias, delta_softplus, channel_last,
                    time_order, nslices, chunk):
    batch, seqlen, dim = _shape_bld(u, channel_last)
    if A.dim() != 2 or A.shape[0] != dim:
        raise RuntimeError(f"A must be (dim={dim}, dstate)")
    if A.is_complex():
        raise RuntimeError("complex A is not supported (not on the SegMamba path)")
    dstate = A.shape[1]
    if dstate > 16:
        raise RuntimeError("selective_scan only supports state dimension <= 16 on this backend")
    B4, C4 = _bc4(B, channel_last), _bc4(C, channel_last)
    groups = B4.shape[2] if channel_last else B4.shape[1]
    exp_shape = (batch, seqlen, groups, dstate) if channel_last else (batch, groups, dstate, seqlen)
    for name, t in (("B", B4), ("C", C4)):
        if tuple(t.shape) != exp_shape:
            raise RuntimeError(f"{name} must have shape {exp_shape}, got {tuple(t.shape)}")
        if t.dtype != u.dtype:
            raise RuntimeError(f"{name} must have the dtype of u")
    if dim % groups != 0:
        raise RuntimeError("dim must be divisible by the number of B/C groups")
    _check_seq("delta", delta, u, u.dtype)
    _check_seq("z", z, u, u.dtype)
    _check_vec("A", A.reshape(-1), dim * dstate, u.device)
    _check_vec("D", D, dim, u.device)
    _check_vec("delta_bias", delta_bias, dim, u.device)
    if time_order == L.TIME_INTERLEAVED and (nslices <= 0 or seqlen % nslices != 0):
        raise RuntimeError(f"seqlen {seqlen} must be divisible by nslices {nslices}")
    a.batch, a.dim, a.dstate, a.n_groups, a.seqlen = batch, dim, dstate, groups, seqlen
    a.dtype = L.dtype_code(u)
    a.delta_softplus = int(bool(delta_softplus))
    a.time_order, a.nslices, a.chunk = int(time_order), int(nslices), int(chunk)
    a.u, a.delta, a.z = L.seq_view(u, channel_last), L.seq_view(delta, channel_last), L.seq_view(z, channel_last)
    a.B, a.C = L.bc_view(B4, channel_last), L.bc_view(C4, channel_last)
    a.A, a.D, a.delta_bias = A.data_ptr(), L.fptr(D), L.fptr(delta_bias)
    a.stream = L.stream_handle(u)
    return batch, seqlen, dim, dstate, groups, B4, C4


def scan_fwd(lib: L.SegmLib, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, *,
             channel_last=False, time_order=L.TIME_FORWARD, nslices=1, chunk=0, need_out=True,
             need_ckpt=False, need_last_state=False, ckpt_buf=None, conv_weight=None, conv_bias=None, dt_x=None, dt_weight=None):
    """-> dict(out, out_z, ckpt, last_state, chunk).  `out` is the un-gated y (None unless need_out or z is None).
    `dt_x` (batch, seqlen, R) rows of R <= 8 consecutive elements [a column window of x_dbl] + `dt_weight` (dim, R) fp32:
    delta = dt_weight . dt_x is formed inside the scan launches (reference selective_scan_interface.py:181-182 without its
    launch) and `delta` is an OUTPUT the apply pass fills, rounded to its dtype, for the backward (regular shapes, one group).
    `ckpt_buf`: a caller-owned fp32 buffer of segm_selective_scan_ckpt_bytes() for the checkpoints.
    `conv_weight` (dim, width) [+ `conv_bias` (dim)]: the causal depthwise conv1d + SiLU in front of the scan is computed inside the
    scan launches and `u` is its INPUT x (regular shapes with softplus and a gate only; results equal conv1d_fwd followed by the scan)."""
    a = L.ScanFwdArgs()
    r = _scan_fwd_prepare(lib, a, u, delta, A, B, C, D, z, delta_bias, delta_softplus, channel_last=channel_last,
                          time_order=time_order, nslices=nslices, chunk=chunk, need_out=need_out, need_ckpt=need_ckpt,
                          need_last_state=need_last_state, ckpt_buf=ckpt_buf, conv_weight=conv_weight, conv_bias=conv_bias,
                          dt_x=dt_x, dt_weight=dt_weight)
    lib.check(lib.dll.segm_selective_scan_fwd(a), "selective_scan_fwd")
    r.pop("_ws")
    return r


def scan_fused_conv_supported(lib: L.SegmLib, batch: int, dim: int, seqlen: int, nslices: int, time_order: int, chunk: int = 0,
                              dstate: int = 16) -> bool:
    """whether scan_fwd(..., conv_weight=) can run: the library's regular-shape condition"""
    return bool(lib.dll.segm_selective_scan_regular_shape(batch, dim, dstate, seqlen, chunk, int(time_order), int(nslices)))


def scan_fwd_multi(lib: L.SegmLib, calls):
    """Several forward scans of ONE geometry (the three directions of a Mamba v3 layer) as one C call: `calls` is a list of
    keyword dicts for `scan_fwd`; the library runs them as one grid with a direction axis when they are regular-shaped and share
    batch / dim / dstate / seqlen / dtype / chunk, else one after the other.  -> list of scan_fwd result dicts."""
    n = len(calls)
    arr = (L.ScanFwdArgs * n)()
    rs = [_scan_fwd_prepare(lib, arr[i], **c) for i, c in enumerate(calls)]
    lib.check(lib.dll.segm_selective_scan_fwd_multi(arr, n), "selective_scan_fwd_multi")
    for r in rs:
        r.pop("_ws")
    return rs


def _scan_fwd_prepare(lib, a, u, delta, A, B, C, D=None, z=None, delta_bias=None, delta_softplus=False, *,
                      channel_last=False, time_order=L.TIME_FORWARD, nslices=1, chunk=0, need_out=True,
                      need_ckpt=False, need_last_state=False, ckpt_buf=None, conv_weight=None, conv_bias=None,
                      dt_x=None, dt_weight=None):
    """fills the argument block `a` and allocates outputs / workspace; -> result dict (+ `_ws`, alive until the launch)"""
    batch, seqlen, dim, dstate, groups, B4, C4 = _fill_scan_args(
        a, u, delta, A, B, C, D, z, delta_bias, delta_softplus, channel_last, time_order, nslices, chunk)
    if chunk == 0:
        chunk = lib.dll.segm_selective_scan_default_chunk(batch, dim, seqlen)
        a.chunk = chunk
    dev = u.device
    out = torch.empty_like(u, memory_format=torch.contiguous_format) if (need_out or z is None) else None
    out_z = torch.empty_like(u, memory_format=torch.contiguous_format) if z is not None else None
    ckpt = None
    if need_ckpt:
        nbytes = lib.dll.segm_selective_scan_ckpt_bytes(batch, dim, dstate, seqlen)
        if ckpt_buf is not None:
            if ckpt_buf.dtype != torch.float32 or not ckpt_buf.is_contiguous() or ckpt_buf.numel() < nbytes // 4 or \
                    ckpt_buf.device != dev:
                raise RuntimeError("scan_fwd: ckpt_buf must be a contiguous fp32 tensor of segm_selective_scan_ckpt_bytes()")
            ckpt = ckpt_buf
        else:
            ckpt = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    last_state = torch.empty(batch, dim, dstate, dtype=torch.float32, device=dev) if need_last_state else None
    ws_bytes = lib.dll.segm_selective_scan_fwd_workspace_bytes(batch, dim, dstate, seqlen, chunk)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a.out, a.out_z = L.seq_view(out, channel_last), L.seq_view(out_z, channel_last)
    a.last_state, a.ckpt = L.fptr(last_state), L.fptr(ckpt)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    keep = [ws]
    if conv_weight is not None:
        if conv_weight.dim() != 2 or conv_weight.shape[0] != dim or not 2 <= conv_weight.shape[1] <= 4:
            raise RuntimeError("scan_fwd: conv_weight must be (dim, width) with width in [2, 4]")
        cw = conv_weight.detach().to(torch.float32).contiguous()
        cb = conv_bias.detach().to(torch.float32).contiguous() if conv_bias is not None else None
        a.conv_weight, a.conv_bias, a.conv_width = cw.data_ptr(), L.fptr(cb), cw.shape[1]
        keep += [cw, cb]
    if dt_x is not None:
        R = dt_x.shape[-1]
        if dt_x.dim() != 3 or tuple(dt_x.shape[:2]) != (batch, seqlen) or not 1 <= R <= 8 or dt_x.stride(2) != 1 or \
                dt_x.dtype != u.dtype or dt_x.device != dev:
            raise RuntimeError("scan_fwd: dt_x must be (batch, seqlen, R <= 8) of u's dtype with unit stride along R")
        if dt_weight is None or tuple(dt_weight.shape) != (dim, R) or dt_weight.dtype != torch.float32 or \
                not dt_weight.is_contiguous() or dt_weight.device != dev:
            raise RuntimeError("scan_fwd: dt_weight must be a contiguous fp32 (dim, R) tensor")
        a.dt_x, a.dt_stride_b, a.dt_stride_t = dt_x.data_ptr(), dt_x.stride(0), dt_x.stride(1)
        a.dt_weight, a.dt_rank = dt_weight.data_ptr(), R
        keep += [dt_x, dt_weight]
    return dict(out=out, out_z=out_z, ckpt=ckpt, last_state=last_state, chunk=chunk, _ws=keep)


def scan_bwd(lib: L.SegmLib, u, delta, A, B, C, D, z, delta_bias, dout, out, ckpt, delta_softplus, *,
             channel_last=False, time_order=L.TIME_FORWARD, nslices=1, chunk=0, du=None, ddelta=None, dz=None, dB=None, dC=None):
    """-> dict(du, ddelta, dA, dB, dC, dD, ddelta_bias, dz, dbc_native).  du / ddelta / dz may be pre-allocated views
    (e.g. halves of one dxz buffer, reference selective_scan_interface.py:244-245); dB / dC have the layout and rank of
    B / C and are fp32 (the reference's accumulation buffers) unless the caller offers destinations of u's own 16-bit type
    AND the launch takes the deterministic kernel (`dbc_native` in the result says which happened: see _scan_bwd_prepare)."""
    a = L.ScanBwdArgs()
    r = _scan_bwd_prepare(lib, a, u, delta, A, B, C, D, z, delta_bias, dout, out, ckpt, delta_softplus, channel_last=channel_last,
                          time_order=time_order, nslices=nslices, chunk=chunk, du=du, ddelta=ddelta, dz=dz, dB=dB, dC=dC)
    lib.check(lib.dll.segm_selective_scan_bwd(a), "selective_scan_bwd")
    r.pop("_ws")
    return r


def scan_bwd_multi(lib: L.SegmLib, calls):
    """the backward counterpart of scan_fwd_multi: `calls` = keyword dicts for `scan_bwd`"""
    n = len(calls)
    arr = (L.ScanBwdArgs * n)()
    rs = [_scan_bwd_prepare(lib, arr[i], **c) for i, c in enumerate(calls)]
    lib.check(lib.dll.segm_selective_scan_bwd_multi(arr, n), "selective_scan_bwd_multi")
    for r in rs:
        r.pop("_ws")
    return rs


def _scan_bwd_prepare(lib, a, u, delta, A, B, C, D, z, delta_bias, dout, out, ckpt, delta_softplus, *,
                      channel_last=False, time_order=L.TIME_FORWARD, nslices=1, chunk=0, du=None, ddelta=None, dz=None,
                      dB=None, dC=None):
    """`dB` / `dC`: optional caller-owned tensors shaped like B / C.  fp32: always honoured.  u's 16-bit dtype (e.g. column
    windows of the x_proj gradient operand): honoured when the launch takes the kernel that sums dB / dC over the d-tiles in a
    fixed order and writes the finished values once (segm_selective_scan_bwd_deterministic) - the result then has
    `dbc_native` True and dB / dC ARE the caller's tensors; otherwise fp32 tensors are allocated and `dbc_native` is False (the
    caller copies, as the reference's final cast does, selective_scan.cpp:488)."""
    if chunk and os.environ.get("SEGM_BWD_CHUNK"):        # experiments only: the backward's own chunking (the checkpoints are per 8 steps, not per chunk)
        chunk = int(os.environ["SEGM_BWD_CHUNK"])
    batch, seqlen, dim, dstate, groups, B4, C4 = _fill_scan_args(
        a.f, u, delta, A, B, C, D, z, delta_bias, delta_softplus, channel_last, time_order, nslices, chunk)
    if chunk == 0:
        raise RuntimeError("scan_bwd needs a chunk length (the forward's, or segm_selective_scan_bwd_default_chunk)")
    if ckpt is None:
        raise RuntimeError("scan_bwd needs the forward checkpoints (run the forward with need_ckpt=True)")
    if z is not None and out is None:
        raise RuntimeError("scan_bwd needs the forward's un-gated output when z is given")
    _check_seq("dout", dout, u, u.dtype)
    _check_seq("out", out, u, u.dtype)
    dev = u.device
    du = torch.empty_like(u, memory_format=torch.contiguous_format) if du is None else du
    ddelta = torch.empty_like(u, memory_format=torch.contiguous_format) if ddelta is None else ddelta
    if z is not None and dz is None:
        dz = torch.empty_like(u, memory_format=torch.contiguous_format)
    for name, t in (("du", du), ("ddelta", ddelta), ("dz", dz)):
        _check_seq(name, t, u, u.dtype)
    dA = torch.empty(dim, dstate, dtype=torch.float32, device=dev)
    a.f.out = L.seq_view(out, channel_last)
    a.f.ckpt = ckpt.data_ptr()
    native = False
    if dB is not None:
        dB, dC = _bc4(dB, channel_last), _bc4(dC, channel_last)
        native = dB.dtype == u.dtype and u.dtype != torch.float32
        for name, t in (("dB", dB), ("dC", dC)):
            if tuple(t.shape) != tuple(B4.shape) or t.dtype != (u.dtype if native else torch.float32) or t.device != dev:
                raise RuntimeError(f"{name} must be an fp32 (or, both, {u.dtype}) tensor of B's shape {tuple(B4.shape)} on the same device")
        if native and not lib.dll.segm_selective_scan_bwd_deterministic(a):
            dB, native = None, False                        # the atomically accumulating kernels need zeroed fp32 buffers
    if dB is None:
        dB = torch.empty(B4.shape, dtype=torch.float32, device=dev)
        dC = torch.empty(C4.shape, dtype=torch.float32, device=dev)
    a.dbc_native = int(native)
    dD = torch.empty(dim, dtype=torch.float32, device=dev) if D is not None else None
    ddb = torch.empty(dim, dtype=torch.float32, device=dev) if delta_bias is not None else None
    ws_bytes = lib.dll.segm_selective_scan_bwd_workspace_bytes(batch, dim, dstate, seqlen, chunk)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a.dout, a.du, a.ddelta, a.dz = (L.seq_view(t, channel_last) for t in (dout, du, ddelta, dz))
    a.dB, a.dC = L.bc_view(dB, channel_last), L.bc_view(dC, channel_last)
    a.dA, a.dD, a.ddelta_bias = dA.data_ptr(), L.fptr(dD), L.fptr(ddb)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    if B.dim() == 3:
        dB = dB.squeeze(2 if channel_last else 1)
    if C.dim() == 3:
        dC = dC.squeeze(2 if channel_last else 1)
    return dict(du=du, ddelta=ddelta, dA=dA, dB=dB, dC=dC, dD=dD, ddelta_bias=ddb, dz=dz, dbc_native=native, _ws=ws)


# ---------------------------------------------------------------------------------------------------------
# causal depthwise conv1d
# ---------------------------------------------------------------------------------------------------------
def _fill_conv_args(a: L.Conv1dArgs, x, weight, bias, silu, channel_last, time_order, nslices):
    batch, seqlen, dim = _shape_bld(x, channel_last)
    if weight.dim() != 2 or weight.shape[0] != dim:
        raise RuntimeError(f"weight must be (dim={dim}, width)")
    width = weight.shape[1]
    if not 2 <= width <= 4:
        raise RuntimeError("causal_conv1d only supports width between 2 and 4")
    _check_vec("weight", weight.reshape(-1) if weight.is_contiguous() else weight, dim * width, x.device)
    _check_vec("bias", bias, dim, x.device)
    if time_order == L.TIME_INTERLEAVED and (nslices <= 0 or seqlen % nslices != 0):
        raise RuntimeError(f"seqlen {seqlen} must be divisible by nslices {nslices}")
    a.batch, a.dim, a.width, a.silu, a.seqlen = batch, dim, width, int(bool(silu)), seqlen
    a.dtype = L.dtype_code(x)
    a.time_order, a.nslices = int(time_order), int(nslices)
    a.x = L.seq_view(x, channel_last)
    a.weight, a.bias = weight.data_ptr(), L.fptr(bias)
    a.stream = L.stream_handle(x)
    return batch, seqlen, dim, width


def conv1d_fwd(lib: L.SegmLib, x, weight, bias=None, silu=False, *, channel_last=False,
               time_order=L.TIME_FORWARD, nslices=1, out=None):
    a = L.Conv1dArgs()
    _fill_conv_args(a, x, weight, bias, silu, channel_last, time_order, nslices)
    out = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
    _check_seq("out", out, x, x.dtype)
    a.out = L.seq_view(out, channel_last)
    lib.check(lib.dll.segm_causal_conv1d_fwd(a), "causal_conv1d_fwd")
    return out


def conv1d_fwd_multi(lib: L.SegmLib, calls):
    """several conv1d_fwd launches in one C call (`calls`: keyword dicts of conv1d_fwd with keys x, weight, bias, silu,
    channel_last, time_order, nslices, out): the three directions of a Mamba v3 layer run as one grid -> list of outputs"""
    n = len(calls)
    arr = (L.Conv1dArgs * n)()
    outs = []
    for i, c in enumerate(calls):
        x = c["x"]
        _fill_conv_args(arr[i], x, c["weight"], c.get("bias"), c.get("silu", False), c.get("channel_last", False),
                        c.get("time_order", L.TIME_FORWARD), c.get("nslices", 1))
        out = c.get("out")
        out = torch.empty_like(x, memory_format=torch.contiguous_format) if out is None else out
        _check_seq("out", out, x, x.dtype)
        arr[i].out = L.seq_view(out, c.get("channel_last", False))
        outs.append(out)
    lib.check(lib.dll.segm_causal_conv1d_fwd_multi(arr, n), "causal_conv1d_fwd_multi")
    return outs


def conv1d_bwd_multi(lib: L.SegmLib, calls):
    """the backward counterpart: keyword dicts of conv1d_bwd (x, weight, bias, dout, silu, channel_last, time_order, nslices, dx)
    -> list of (dx, dweight, dbias)"""
    n = len(calls)
    arr = (L.Conv1dArgs * n)()
    res, keep = [], []
    for i, c in enumerate(calls):
        r = _conv1d_bwd_prepare(lib, arr[i], c["x"], c["weight"], c.get("bias"), c["dout"], c.get("silu", False),
                                channel_last=c.get("channel_last", False), time_order=c.get("time_order", L.TIME_FORWARD),
                                nslices=c.get("nslices", 1), dx=c.get("dx"))
        res.append(r[:3])
        keep.append(r[3])
    lib.check(lib.dll.segm_causal_conv1d_bwd_multi(arr, n), "causal_conv1d_bwd_multi")
    return res


def conv1d_bwd(lib: L.SegmLib, x, weight, bias, dout, silu=False, *, channel_last=False,
               time_order=L.TIME_FORWARD, nslices=1, dx=None):
    """-> (dx, dweight fp32 (dim, width), dbias fp32 (dim) or None)"""
    a = L.Conv1dArgs()
    dx, dweight, dbias, _ws = _conv1d_bwd_prepare(lib, a, x, weight, bias, dout, silu, channel_last=channel_last,
                                                  time_order=time_order, nslices=nslices, dx=dx)
    lib.check(lib.dll.segm_causal_conv1d_bwd(a), "causal_conv1d_bwd")
    return dx, dweight, dbias


def _conv1d_bwd_prepare(lib, a, x, weight, bias, dout, silu=False, *, channel_last=False, time_order=L.TIME_FORWARD, nslices=1,
                        dx=None):
    batch, seqlen, dim, width = _fill_conv_args(a, x, weight, bias, silu, channel_last, time_order, nslices)
    _check_seq("dout", dout, x, x.dtype)
    dx = torch.empty_like(x, memory_format=torch.contiguous_format) if dx is None else dx
    _check_seq("dx", dx, x, x.dtype)
    dev = x.device
    dweight = torch.empty(dim, width, dtype=torch.float32, device=dev)
    dbias = torch.empty(dim, dtype=torch.float32, device=dev) if bias is not None else None
    ws_bytes = lib.dll.segm_causal_conv1d_bwd_workspace_bytes(batch, dim, width, seqlen)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    a.dout, a.dx = L.seq_view(dout, channel_last), L.seq_view(dx, channel_last)
    a.dweight, a.dbias = dweight.data_ptr(), L.fptr(dbias)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    return dx, dweight, dbias, ws


# ---------------------------------------------------------------------------------------------------------
# 3x3x3 convolution weight gradient (stem / decoder)
# ---------------------------------------------------------------------------------------------------------
def conv3d_k3_wgrad_supported(x: torch.Tensor, dy: torch.Tensor) -> bool:
    """Shapes / layouts the MFMA weight-gradient kernel takes (everything else stays on MIOpen)."""
    if x.dim() != 5 or dy.dim() != 5 or x.dtype not in (torch.bfloat16, torch.float16) or dy.dtype != x.dtype:
        return False
    if x.shape[0] != dy.shape[0] or x.shape[2:] != dy.shape[2:]:
        return False
    if (x.shape[1] % 48 and x.shape[1] > 48) or dy.shape[1] % 48 or x.shape[4] % 8:
        return False
    for t in (x, dy):
        if t.stride(4) != 1 or any(t.stride(i) % 8 for i in range(4)) or t.data_ptr() % 16:
            return False
    return conv3d_k3_wgrad_spans_fit(x, dy)


def conv3d_k3_wgrad_spans_fit(x: torch.Tensor, dy: torch.Tensor) -> bool:
    """The weight-gradient kernel addresses a (batch, plane, 48-channel block) through 32-bit byte offsets: 48 channel strides and
    a plane's rows must stay below the buffer descriptor's 0xFFFFF000 bytes - the same bound segm_conv3d_k3_wgrad checks
    (csrc/conv3d_wgrad.hip, `fits32`; volumes up to ~350^3 elements per channel).  Beyond it the routing falls back to the
    vendor route instead of raising."""
    lim = 0xFFFFF000 - 4096
    W, H = x.shape[4], x.shape[3]
    for t in (x, dy):
        if t.stride(1) * 96 + 2 * W >= lim or t.stride(3) * 2 * H >= lim:
            return False
    return True


def conv3d_k3_wgrad(lib: L.SegmLib, x: torch.Tensor, dy: torch.Tensor, out_dtype=torch.bfloat16) -> torch.Tensor:
    """dW (Cout, Cin, 3, 3, 3) of a stride-1 pad-1 3x3x3 convolution; x (B, Cin, D, H, W), dy (B, Cout, D, H, W), bf16."""
    if not conv3d_k3_wgrad_supported(x, dy):
        raise RuntimeError("conv3d_k3_wgrad: unsupported shape / dtype / layout")
    B, cin, D, H, W = x.shape
    cout = dy.shape[1]
    a = L.Conv3dWgradArgs()
    a.batch, a.cin, a.cout, a.depth, a.height, a.width = B, cin, cout, D, H, W
    a.dtype = L.dtype_code(x)
    a.dw_dtype = L.dtype_code(torch.empty(0, dtype=out_dtype))
    a.x, a.dy = x.data_ptr(), dy.data_ptr()
    a.x_stride_b, a.x_stride_c, a.x_stride_z, a.x_stride_y = x.stride()[:4]
    a.dy_stride_b, a.dy_stride_c, a.dy_stride_z, a.dy_stride_y = dy.stride()[:4]
    dw = torch.empty(cout, cin, 3, 3, 3, dtype=out_dtype, device=x.device)
    ws_bytes = lib.dll.segm_conv3d_k3_wgrad_workspace_bytes(B, cin, cout, D, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a.dw, a.workspace, a.workspace_bytes = dw.data_ptr(), ws.data_ptr(), ws_bytes
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_conv3d_k3_wgrad(a), "conv3d_k3_wgrad")
    return dw


# ---------------------------------------------------------------------------------------------------------
# 3x3x3 convolution forward / data gradient (48 input channels)
# ---------------------------------------------------------------------------------------------------------
def pack_conv3d_weight(weight: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """(Cout, Cin <= 48, 3, 3, 3) -> (Cout, 3, 3, 3, 48) contiguous in the activations' 16-bit dtype: the layout
    segm_conv3d_k3_fwd keeps in registers."""
    w = weight.permute(0, 2, 3, 4, 1)
    if w.shape[-1] < 48:                                   # a narrow first layer: zero input channels up to 48
        w = torch.nn.functional.pad(w, (0, 48 - w.shape[-1]))
    return w.contiguous().to(dtype)


def pack_conv3d_weight_for_dgrad(weight: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """The data gradient of a stride-1 pad-1 3x3x3 convolution is the forward convolution of dy with the spatially
    flipped, channel-transposed weights: (Cout, Cin, 3, 3, 3) -> packed (Cin, 3, 3, 3, Cout)."""
    return pack_conv3d_weight(weight.flip(2, 3, 4).transpose(0, 1), dtype)


def conv3d_k3_fwd_supported(x: torch.Tensor, cout: int) -> bool:
    if x.dim() != 5 or x.dtype not in (torch.bfloat16, torch.float16) or not 1 <= x.shape[1] <= 48 or cout % 16 or x.shape[4] % 8:
        return False
    return x.stride(4) == 1 and not any(x.stride(i) % 8 for i in range(4)) and x.data_ptr() % 16 == 0


CONV_FWD_ACCUMULATE, CONV_FWD_CHAIN, CONV_FWD_PITCH48, CONV_FWD_CHAIN32 = 1, 2, 4, 8     # segm_conv_fwd_flags


def conv3d_k3_fwd(lib: L.SegmLib, x: torch.Tensor, w_packed: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, accumulate: bool = False, chain: bool = False,
                  pitch48: bool = False, chain32: bool = False, want_stats: bool = False):
    """y (B, Cout, D, H, W) = conv3d(x, w, bias, stride 1, padding 1); x (B, <= 48, D, H, W) bf16 / fp16, w_packed from
    pack_conv3d_weight().  `out` + `accumulate`: add to an existing result (the next 48-channel block of a wider
    layer; Cout % 48 == 0).  `chain`: the pipelined-K-parts kernel (Cout % 48 == 0); `pitch48`: its unpadded LDS layout; `chain32`: the
    same pipeline on 32-wide x blocks, two workgroups per CU (exclusive with `chain`).
    want_stats (chain + pitch48, or chain32): -> (y, stats), stats = fp32 (B, Cout, nparts, 4) partial {count, sum, sum of squares, -}
    of what this launch stored, for instnorm_fwd(..., stats=stats); (y, None) when the launch has no statistics epilogue."""
    cout = w_packed.shape[0]
    if not conv3d_k3_fwd_supported(x, cout):
        raise RuntimeError("conv3d_k3_fwd: unsupported shape / dtype / layout")
    if tuple(w_packed.shape[1:]) != (3, 3, 3, 48) or w_packed.dtype != x.dtype or not w_packed.is_contiguous():
        raise RuntimeError("conv3d_k3_fwd: w_packed must be a contiguous (Cout, 3, 3, 3, 48) tensor of x's dtype")
    if (accumulate or chain or chain32) and cout % 48:
        raise RuntimeError("conv3d_k3_fwd: accumulate / chain need Cout % 48 == 0")
    if chain32 and (chain or pitch48):
        raise RuntimeError("conv3d_k3_fwd: chain32 excludes chain / pitch48")
    B, _, D, H, W = x.shape
    if out is None:
        if accumulate:
            raise RuntimeError("conv3d_k3_fwd: accumulate needs `out`")
        y = volume_empty(B, cout, (D, H, W), x.dtype, x.device)
    else:
        y = out
        if tuple(y.shape) != (B, cout, D, H, W) or y.dtype != x.dtype or y.device != x.device or y.stride(4) != 1 or \
                any(y.stride(i) % 8 for i in range(4)) or y.data_ptr() % 16:
            raise RuntimeError("conv3d_k3_fwd: `out` must be a (B, Cout, D, H, W) tensor of x's dtype, W contiguous, 16-byte rows")
    if bias is not None:
        bias = bias.float().contiguous()
    a = L.Conv3dFwdArgs()
    a.batch, a.cin, a.cout, a.depth, a.height, a.width = B, x.shape[1], cout, D, H, W
    a.dtype = L.dtype_code(x)
    if pitch48 and not chain:
        raise RuntimeError("conv3d_k3_fwd: pitch48 is a variant of the chained kernel")
    a.flags = (CONV_FWD_ACCUMULATE if accumulate else 0) | (CONV_FWD_CHAIN if chain else 0) | (CONV_FWD_PITCH48 if pitch48 else 0) | \
        (CONV_FWD_CHAIN32 if chain32 else 0)
    a.x, a.y, a.w_packed = x.data_ptr(), y.data_ptr(), w_packed.data_ptr()
    a.x_stride_b, a.x_stride_c, a.x_stride_z, a.x_stride_y = x.stride()[:4]
    a.y_stride_b, a.y_stride_c, a.y_stride_z, a.y_stride_y = y.stride()[:4]
    a.bias = bias.data_ptr() if bias is not None else None
    a.stream = L.stream_handle(x)
    stats = None
    if want_stats and ((chain and pitch48) or chain32):
        nparts = lib.dll.segm_conv3d_k3_fwd_stats_parts(D, H, W, B, cout, a.flags)
        if nparts > 0:
            # (a workgroup whose y part is empty - ysplit >= 16 with H not a multiple of it - writes a zero-count slot: ADVICE r05)
            stats = torch.empty(B, cout, nparts, 4, dtype=torch.float32, device=x.device)
            a.stats_partials, a.stats_nparts = stats.data_ptr(), nparts
    lib.check(lib.dll.segm_conv3d_k3_fwd(a), "conv3d_k3_fwd")
    return (y, stats) if want_stats else y


# ---------------------------------------------------------------------------------------------------------
# channel-last 3x3x3 convolution (round 6 prototype, csrc/conv3d_cl.hip)
CONV_CL_ACCUMULATE, CONV_CL_WAVES8 = 1, 2
_cl_index_cache = {}


def conv3d_cl_weight_image(lib: L.SegmLib, w: torch.Tensor, dtype=None) -> torch.Tensor:
    """(48, 48, 3, 3, 3) weights -> the (14, 9, 64, 8) image of MFMA operand fragments segm_conv3d_k3_fwd_cl keeps in LDS (one
    gather through the index map the library exports).  For the data gradient pass flip(w, (2, 3, 4)).transpose(0, 1)."""
    if tuple(w.shape) != (48, 48, 3, 3, 3):
        raise RuntimeError("conv3d_cl_weight_image: weights must be (48, 48, 3, 3, 3)")
    key = str(w.device)
    idx = _cl_index_cache.get(key)
    if idx is None:
        n = 14 * 9 * 64 * 8
        host = torch.empty(n, dtype=torch.int32)
        lib.check(lib.dll.segm_conv3d_k3_cl_pack_index(host.data_ptr(), n), "conv3d_k3_cl_pack_index")
        idx = host.to(w.device).long()
        _cl_index_cache[key] = idx
    flat = torch.cat([w.reshape(-1), w.new_zeros(1)])       # index -1 -> the appended zero
    return flat[idx].view(14, 9, 64, 8).to(dtype or w.dtype).contiguous()


def _check_out(name: str, out: torch.Tensor, x: torch.Tensor, shape) -> None:
    """`out` of a kernel that takes it as a raw pointer + four strides: the shape the launch writes, x's dtype and device, unit
    stride along the last dimension, 16-byte rows"""
    if tuple(out.shape) != tuple(shape) or out.dtype != x.dtype or out.device != x.device or out.stride(4) != 1 or \
            any(out.stride(i) % 8 or out.stride(i) <= 0 for i in range(4)) or out.data_ptr() % 16:
        raise RuntimeError(f"{name}: `out` must be a {tuple(shape)} tensor of x's dtype on x's device, last dimension contiguous, 16-byte rows")


def _check_w_image(name: str, w_image: torch.Tensor, x: torch.Tensor, numel: int) -> None:
    if w_image.dtype != x.dtype or w_image.device != x.device or not w_image.is_contiguous() or w_image.numel() != numel:
        raise RuntimeError(f"{name}: `w_image` must be a contiguous image of {numel} elements of x's dtype on x's device")


def conv3d_k3_fwd_cl(lib: L.SegmLib, x: torch.Tensor, w_image: torch.Tensor, bias=None, out=None, accumulate=False, waves8=False):
    """y (B, D, H, W, 48) = conv3d(x (B, D, H, W, 48) channel-last, 3x3x3, stride 1, pad 1); bf16 / fp16."""
    if x.dim() != 5 or x.shape[4] != 48 or x.stride(4) != 1 or x.dtype not in (torch.bfloat16, torch.float16):
        raise RuntimeError("conv3d_k3_fwd_cl: x must be a (B, D, H, W, 48) 16-bit tensor with contiguous channels")
    B, D, H, W, _ = x.shape
    if accumulate and out is None:
        raise RuntimeError("conv3d_k3_fwd_cl: accumulate needs `out`")
    _check_w_image("conv3d_k3_fwd_cl", w_image, x, 14 * 9 * 64 * 8)
    if out is not None:
        _check_out("conv3d_k3_fwd_cl", out, x, (B, D, H, W, 48))
    y = out if out is not None else torch.empty(B, D, H, W, 48, dtype=x.dtype, device=x.device)
    a = L.Conv3dClArgs()
    a.batch, a.channels, a.depth, a.height, a.width = B, 48, D, H, W
    a.dtype = L.dtype_code(x)
    a.flags = (CONV_CL_ACCUMULATE if accumulate else 0) | (CONV_CL_WAVES8 if waves8 else 0)
    a.x, a.y, a.w_image = x.data_ptr(), y.data_ptr(), w_image.data_ptr()
    a.x_stride_b, a.x_stride_z, a.x_stride_y, a.x_stride_x = x.stride()[:4]
    a.y_stride_b, a.y_stride_z, a.y_stride_y, a.y_stride_x = y.stride()[:4]
    if bias is not None:
        bias = bias.float().contiguous()
    a.bias = bias.data_ptr() if bias is not None else None
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_conv3d_k3_fwd_cl(a), "conv3d_k3_fwd_cl")
    return y


# ---------------------------------------------------------------------------------------------------------
# 3x3x3 convolution of wide layers on small volumes (csrc/conv3d_cube.hip, ABI 10)
# ---------------------------------------------------------------------------------------------------------
CONV_CUBE_ACCUMULATE = 1
_cube_index_cache = {}


def conv3d_cube_supported(x: torch.Tensor, cout: int) -> bool:
    """does segm_conv3d_k3_cube_fwd take this input (B, Cin, D, H, W) for `cout` output channels"""
    if x.dim() != 5 or x.dtype not in (torch.bfloat16, torch.float16) or x.stride(4) != 1:
        return False
    B, C, D, H, W = x.shape
    if C % 32 != 0 or (cout % 64 != 0 and cout % 96 != 0) or D % 8 or H % 8 or W % 8 or min(B, C, D, H, W) <= 0:
        return False
    return all(s % 8 == 0 and s > 0 for s in x.stride()[:4]) and x.data_ptr() % 16 == 0


def conv3d_cube_index(lib: L.SegmLib, cout_w: int, cin_w: int, flipped: bool, device) -> torch.Tensor:
    """int32 map: element i of the kernel's weight image <- flat index into the (cout_w, cin_w, 3, 3, 3) weight"""
    key = (cout_w, cin_w, bool(flipped), str(device))
    idx = _cube_index_cache.get(key)
    if idx is None:
        n = cout_w * cin_w * 27
        host = torch.empty(n, dtype=torch.int32)
        lib.check(lib.dll.segm_conv3d_k3_cube_pack_index(host.data_ptr(), n, cout_w, cin_w, 1 if flipped else 0), "conv3d_k3_cube_pack_index")
        idx = host.to(device)
        _cube_index_cache[key] = idx
    return idx


_cube_desc_cache = {}


def conv3d_cube_weight_image(lib: L.SegmLib, w: torch.Tensor, flipped: bool = False, dtype=None, by_index: bool = False) -> torch.Tensor:
    """(Cout, Cin, 3, 3, 3) weights (or a channel slice of a wider weight) -> the fragment image segm_conv3d_k3_cube_fwd streams
    (`flipped`: the image of the data gradient, a convolution of dy with flip(w)^T).  On the device one launch of the pack kernel
    (segm_conv3d_k3_cube_pack_multi with a single cached descriptor); `by_index` (and layouts the kernel does not take): a gather
    through the index map the library exports - the definition the pack kernel is tested against."""
    direct = (not by_index and L.on_device(w) and w.dim() == 5 and tuple(w.shape[2:]) == (3, 3, 3) and tuple(w.stride()[1:]) == (27, 9, 3, 1) and
              w.dtype in (torch.bfloat16, torch.float16) and w.shape[0] % 32 == 0 and w.shape[1] % 32 == 0 and 0 < w.stride(0) < (1 << 31) and
              (dtype is None or dtype == w.dtype))
    if direct:
        key = (w.shape[0], w.shape[1], w.stride(0), bool(flipped), str(w.device))
        hit = _cube_desc_cache.get(key)
        if hit is None:
            hit = cube_pack_descs([(0, 0, w.shape[0], w.shape[1], w.stride(0), flipped)], w.device)
            _cube_desc_cache[key] = hit
        out = torch.empty(w.shape[0] * w.shape[1] * 27, dtype=w.dtype, device=w.device)
        lib.check(lib.dll.segm_conv3d_k3_cube_pack_multi(w.data_ptr(), out.data_ptr(), hit[0].data_ptr(), 1, hit[1], L.stream_handle(out)),
                  "conv3d_k3_cube_pack_multi")
        return out
    idx = conv3d_cube_index(lib, w.shape[0], w.shape[1], flipped, w.device)
    img = torch.index_select(w.reshape(-1), 0, idx)
    return img if dtype is None or dtype == img.dtype else img.to(dtype)


def cube_pack_descs(items, device) -> tuple:
    """items: [(src_off, out_off, cout_w, cin_w, co_stride, flipped)] -> (int32 (n, 10) device tensor laid out as the 40-byte
    segm_cube_pack_desc {src_off lo, src_off hi, out_off lo, out_off hi, cout_w, cin_w, co_stride, flipped, first_block, reserved},
    total blocks) for conv3d_cube_pack_multi"""
    rows, first = [], 0
    for src_off, out_off, cout_w, cin_w, co_stride, flipped in items:
        rows.append([src_off & 0xffffffff, src_off >> 32, out_off & 0xffffffff, out_off >> 32, cout_w, cin_w, co_stride, int(bool(flipped)), first, 0])
        first += (cin_w // 16) * (cout_w // 32) if flipped else (cout_w // 16) * (cin_w // 32)
    t = torch.tensor(rows, dtype=torch.int64).to(torch.int32).to(device).contiguous()
    return t, first


def conv3d_cube_pack_multi(lib: L.SegmLib, src: torch.Tensor, out: torch.Tensor, descs: torch.Tensor, nblocks: int) -> torch.Tensor:
    """every weight image described by `descs` (cube_pack_descs) from the 16-bit weight buffer `src` into `out`, one launch"""
    if src.dtype not in (torch.bfloat16, torch.float16) or out.dtype != src.dtype or descs.dtype != torch.int32 or descs.dim() != 2 or \
            descs.shape[1] != 10 or not (src.is_contiguous() and out.is_contiguous() and descs.is_contiguous()) or out.data_ptr() & 15:
        raise RuntimeError("conv3d_cube_pack_multi: 16-bit src / out, int32 (n, 10) descriptors")
    lib.check(lib.dll.segm_conv3d_k3_cube_pack_multi(src.data_ptr(), out.data_ptr(), descs.data_ptr(), descs.shape[0], nblocks,
                                                     L.stream_handle(out)), "conv3d_k3_cube_pack_multi")
    return out


def conv3d_cube_plan(lib: L.SegmLib, B, cin, cout, D, H, W, nt=0, splits=0):
    c_nt, c_s, c_ws = C.c_int32(nt), C.c_int32(splits), C.c_int64(0)
    lib.check(lib.dll.segm_conv3d_k3_cube_plan(B, cin, cout, D, H, W, C.byref(c_nt), C.byref(c_s), C.byref(c_ws)), "conv3d_k3_cube_plan")
    return c_nt.value, c_s.value, c_ws.value


def conv3d_k3_cube_fwd(lib: L.SegmLib, x: torch.Tensor, w_image: torch.Tensor, cout: int, bias=None, out=None, accumulate=False,
                       nt=0, splits=0, want_stats=False):
    """y (B, cout, D, H, W) = conv3d(x (B, Cin, D, H, W), 3x3x3, stride 1, pad 1) through the cube kernel; bf16 / fp16.  The
    fp32 partial sums of a split contraction live in a workspace allocated per call (none with one split).  `out` and `w_image`
    reach the kernel as raw pointers: both are checked here (RuntimeError).
    want_stats: -> (y, stats), stats = fp32 (B, cout, nparts, 4) partial {count, sum, sum of squares, -} of what the launch stored
    (per wave of the storing launch: 128 or 512 voxels), for instnorm_fwd(..., stats=stats)."""
    if not conv3d_cube_supported(x, cout):
        raise RuntimeError("conv3d_k3_cube_fwd: unsupported input")
    B, cin, D, H, W = x.shape
    if accumulate and out is None:
        raise RuntimeError("conv3d_k3_cube_fwd: accumulate needs `out`")
    _check_w_image("conv3d_k3_cube_fwd", w_image, x, cout * cin * 27)
    if out is not None:
        _check_out("conv3d_k3_cube_fwd", out, x, (B, cout, D, H, W))
    y = out if out is not None else torch.empty(B, cout, D, H, W, dtype=x.dtype, device=x.device)
    nt, splits, need = conv3d_cube_plan(lib, B, cin, cout, D, H, W, nt, splits)
    # the partial sums of this call (none with one split): a fresh tensor per call - the caching allocator hands the same block back
    # call after call on one stream, and a buffer shared between calls would be a race as soon as two streams convolve
    ws = torch.empty(need, dtype=torch.float32, device=x.device) if need > 0 else None
    a = L.Conv3dCubeArgs()
    a.batch, a.cin, a.cout, a.depth, a.height, a.width = B, cin, cout, D, H, W
    a.dtype = L.dtype_code(x)
    a.flags = CONV_CUBE_ACCUMULATE if accumulate else 0
    a.nt, a.splits = nt, splits
    a.x, a.y, a.w_image = x.data_ptr(), y.data_ptr(), w_image.data_ptr()
    a.x_stride_b, a.x_stride_c, a.x_stride_z, a.x_stride_y = x.stride()[:4]
    a.y_stride_b, a.y_stride_c, a.y_stride_z, a.y_stride_y = y.stride()[:4]
    if bias is not None:
        bias = bias.float().contiguous()
    a.bias = bias.data_ptr() if bias is not None else None
    a.workspace, a.workspace_elems = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    a.stream = L.stream_handle(x)
    stats = None
    if want_stats:
        stats = torch.empty(B, cout, lib.dll.segm_conv3d_k3_cube_stats_parts(D, H, W, splits), 4, dtype=torch.float32, device=x.device)
        a.stats_partials, a.stats_nparts = stats.data_ptr(), stats.shape[2]
    lib.check(lib.dll.segm_conv3d_k3_cube_fwd(a), "conv3d_k3_cube_fwd")
    return (y, stats) if want_stats else y


def conv3d_cube_wgrad_supported(x: torch.Tensor, dy: torch.Tensor) -> bool:
    if x.dim() != 5 or dy.dim() != 5 or x.dtype not in (torch.bfloat16, torch.float16) or dy.dtype != x.dtype:
        return False
    if x.shape[0] != dy.shape[0] or x.shape[2:] != dy.shape[2:] or x.shape[1] % 32 or dy.shape[1] % 64 or x.shape[2] % 8 or x.shape[3] % 8 or x.shape[4] % 8:
        return False
    for t in (x, dy):
        if t.stride(4) != 1 or any(t.stride(i) % 8 or t.stride(i) <= 0 for i in range(4)) or t.data_ptr() % 16:
            return False
    return True


def conv3d_k3_cube_wgrad(lib: L.SegmLib, x: torch.Tensor, dy: torch.Tensor, out_dtype=torch.float32) -> torch.Tensor:
    """dW (Cout, Cin, 3, 3, 3) of a stride-1 pad-1 3x3x3 convolution through segm_conv3d_k3_cube_wgrad; x (B, Cin, D, H, W),
    dy (B, Cout, D, H, W), bf16 / fp16"""
    if not conv3d_cube_wgrad_supported(x, dy):
        raise RuntimeError("conv3d_k3_cube_wgrad: unsupported shape / dtype / layout")
    B, cin, D, H, W = x.shape
    cout = dy.shape[1]
    a = L.Conv3dWgradArgs()
    a.batch, a.cin, a.cout, a.depth, a.height, a.width = B, cin, cout, D, H, W
    a.dtype = L.dtype_code(x)
    a.dw_dtype = L.dtype_code(torch.empty(0, dtype=out_dtype))
    a.x, a.dy = x.data_ptr(), dy.data_ptr()
    a.x_stride_b, a.x_stride_c, a.x_stride_z, a.x_stride_y = x.stride()[:4]
    a.dy_stride_b, a.dy_stride_c, a.dy_stride_z, a.dy_stride_y = dy.stride()[:4]
    dw = torch.empty(cout, cin, 3, 3, 3, dtype=out_dtype, device=x.device)
    ws_bytes = lib.dll.segm_conv3d_k3_cube_wgrad_workspace_bytes(B, cin, cout, D, H, W)
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=x.device)
    a.dw, a.workspace, a.workspace_bytes = dw.data_ptr(), ws.data_ptr(), ws.numel() * 4
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_conv3d_k3_cube_wgrad(a), "conv3d_k3_cube_wgrad")
    return dw


# ---------------------------------------------------------------------------------------------------------
# InstanceNorm3d (+ residual) (+ activation)
# ---------------------------------------------------------------------------------------------------------
ACT_CODES = {"none": 0, "relu": 1, "leaky_relu": 2}


# ---------------------------------------------------------------------------------------------------------
# volumes with a padded channel stride
# ---------------------------------------------------------------------------------------------------------
# A dense (B, C, 128, 128, 128) 16-bit volume has a channel stride of exactly 4 MiB: the C lines a convolution writes for one
# output row (one per channel, same z / y / x) all fall into the same L2 set and the same memory channel.  Measured on MI355X
# (profiles/r02_conv_stride_pad.log): the 48 -> 48 3x3x3 kernel takes 0.669 ms on dense tensors, 0.586 ms with 64 elements of
# padding per channel of the OUTPUT and 0.530 ms with input and output padded; the 1x1x1 kernel 0.284 -> 0.247 ms; 64^3 volumes
# (0.5 MiB) do not care.  The convolution kernels therefore allocate such outputs with `volume_empty`; their consumers take the
# strides (convolutions, the instance-norm kernels) or see an ordinary strided tensor (ATen).
_VOLUME_PAD = 192                 # elements: 384 bytes = three 128-byte lines
_VOLUME_PAD_ON = os.environ.get("SEGM_VOLUME_PAD", "1") == "1"
_VOLUME_PAD_QUANTUM = 1 << 20     # channel sizes (bytes) that are multiples of this get the padding (tests lower it)


def volume_empty(B: int, C: int, spatial, dtype: torch.dtype, device) -> torch.Tensor:
    """(B, C, *spatial) tensor, dense inside a channel; the channel stride is padded by _VOLUME_PAD elements when the dense one
    would be a multiple of 1 MiB (C >= 16: with a handful of channels nothing aliases; 16-bit dtypes only: fp32 volumes go to
    vendor kernels that would copy a strided input)."""
    S = 1
    for d in spatial:
        S *= int(d)
    nbytes = S * torch.empty(0, dtype=dtype).element_size()
    if not (_VOLUME_PAD_ON and C >= 16 and dtype in (torch.bfloat16, torch.float16) and nbytes >= _VOLUME_PAD_QUANTUM
            and nbytes % _VOLUME_PAD_QUANTUM == 0):
        return torch.empty(B, C, *spatial, dtype=dtype, device=device)
    buf = torch.empty(B, C, S + _VOLUME_PAD, dtype=dtype, device=device)
    return buf[:, :, :S].view(B, C, *spatial)


def channel_dense(x: torch.Tensor) -> bool:
    """(B, C, *spatial) with dense channels (contiguous spatial dims) and batch stride = C * channel stride: what the kernels
    that take a channel / instance stride accept (a contiguous tensor, or one from volume_empty)."""
    if x.dim() < 3:
        return False
    s = 1
    for i in range(x.dim() - 1, 1, -1):
        if x.shape[i] != 1 and x.stride(i) != s:
            return False
        s *= x.shape[i]
    if x.shape[1] == 1:                                   # one channel: the batch stride is the instance stride
        return x.shape[0] == 1 or x.stride(0) >= s
    return x.stride(1) >= s and (x.shape[0] == 1 or x.stride(0) == x.shape[1] * x.stride(1))


def instance_stride(x: torch.Tensor) -> int:
    """elements between consecutive (b, c) instances of a channel_dense tensor (strides of size-1 dimensions mean nothing)"""
    if x.shape[1] > 1:
        return x.stride(1)
    if x.shape[0] > 1:
        return x.stride(0)
    return x[0, 0].numel()


def _norm_geom(x):
    if x.dim() < 3 or not channel_dense(x):
        raise RuntimeError("instnorm: x must be a (B, C, *spatial) tensor with dense channels (contiguous, or a padded channel stride)")
    inst = x.shape[0] * x.shape[1]
    return inst, x.numel() // inst


class NormStats:
    """The statistics pass of one tensor, waiting for the apply pass of a residual tail: `partials` as segm_instnorm_stats wrote them;
    `mean` / `rstd` (fp32, B * C) are filled in by the tail's forward."""

    def __init__(self, partials, mean, rstd):
        self.partials, self.mean, self.rstd = partials, mean, rstd


def instnorm_fwd(lib: L.SegmLib, x, residual=None, act="none", slope=0.01, eps=1e-5, stats=None, *, stats_only=False, skip=None,
                 skip_stats=None):
    """-> (y, mean, rstd): y = act(IN(x) + residual); mean / rstd fp32 (B * C).
    stats: fp32 (B, C, nparts, 4) of {count, sum, sum of squares, -} partials summed by the producer of x (conv3d_k3_fwd's `stats`):
    the statistics pass over x is skipped.
    The residual tail y = act(IN(x) + IN(skip)) in one apply pass (segm_instnorm_tail_fwd) takes two calls:
      stats_only=True -> NormStats: the statistics pass over x alone (the skip), nothing applied;
      skip=<the skip tensor>, skip_stats=<its NormStats> in place of a materialised residual -> (y, mean, rstd), and skip_stats.mean /
      .rstd are filled in."""
    inst, S = _norm_geom(x)
    if stats_only:
        if residual is not None or stats is not None or skip is not None or skip_stats is not None:
            raise RuntimeError("instnorm: stats_only takes x alone")
        a = L.InstNormStatsArgs()
        a.instances, a.dtype, a.spatial = inst, L.dtype_code(x), S
        nbytes = lib.dll.segm_instnorm_workspace_bytes(inst, S)
        part = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        a.x, a.x_instance_stride, a.partials, a.partials_bytes, a.stream = x.data_ptr(), instance_stride(x), part.data_ptr(), nbytes, L.stream_handle(x)
        lib.check(lib.dll.segm_instnorm_stats(a), "instnorm_stats")
        return NormStats(part, torch.empty(inst, dtype=torch.float32, device=x.device), torch.empty(inst, dtype=torch.float32, device=x.device))
    if stats is not None and (stats.dtype != torch.float32 or stats.dim() != 4 or stats.shape[0] * stats.shape[1] != inst or
                              stats.shape[3] != 4 or not stats.is_contiguous() or stats.device != x.device):
        raise RuntimeError("instnorm: stats must be a contiguous fp32 (B, C, nparts, 4) tensor on x's device")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype or not channel_dense(residual)):
        raise RuntimeError("instnorm: residual must match x (shape, dtype, dense channels)")
    if (skip is None) != (skip_stats is None) or (skip is not None and residual is not None):
        raise RuntimeError("instnorm: a tail takes skip and skip_stats together, and no residual")
    if skip is not None and (skip.shape != x.shape or skip.dtype != x.dtype or not channel_dense(skip) or skip.device != x.device
                             or skip_stats.mean.numel() != inst):
        raise RuntimeError("instnorm: skip must match x (shape, dtype, dense channels) and skip_stats must be its statistics")
    a = L.InstNormFwdArgs() if skip is None else L.InstNormTailFwdArgs()
    a.instances, a.dtype, a.act, a.spatial = inst, L.dtype_code(x), ACT_CODES[act], S
    a.slope, a.eps = float(slope), float(eps)
    y = volume_empty(x.shape[0], x.shape[1], x.shape[2:], x.dtype, x.device)
    a.x_instance_stride, a.y_instance_stride = instance_stride(x), instance_stride(y)
    mean = torch.empty(inst, dtype=torch.float32, device=x.device)
    rstd = torch.empty(inst, dtype=torch.float32, device=x.device)
    ws_bytes = lib.dll.segm_instnorm_workspace_bytes(inst, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a.x, a.y = x.data_ptr(), y.data_ptr()
    a.mean, a.rstd = mean.data_ptr(), rstd.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws_bytes, L.stream_handle(x)
    if stats is not None:
        a.stats_partials, a.stats_nparts = stats.data_ptr(), stats.shape[2]
    if skip is not None:
        a.skip, a.skip_instance_stride = skip.data_ptr(), instance_stride(skip)
        a.skip_mean, a.skip_rstd = skip_stats.mean.data_ptr(), skip_stats.rstd.data_ptr()
        a.skip_partials, a.skip_partials_bytes = skip_stats.partials.data_ptr(), skip_stats.partials.numel()
        lib.check(lib.dll.segm_instnorm_tail_fwd(a), "instnorm_tail_fwd")
        return y, mean, rstd
    a.residual = residual.data_ptr() if residual is not None else None
    a.residual_instance_stride = instance_stride(residual) if residual is not None else 0
    lib.check(lib.dll.segm_instnorm_fwd(a), "instnorm_fwd")
    return y, mean, rstd


def instnorm_bwd(lib: L.SegmLib, x, dy, mean, rstd, y=None, act="none", slope=0.01, want_dresidual=False):
    """-> (dx, dresidual or None).  `y` is needed iff act != none and the forward added a residual."""
    inst, S = _norm_geom(x)
    if dy.shape != x.shape or dy.dtype != x.dtype:
        raise RuntimeError("instnorm: dy must match x")
    if not channel_dense(dy):
        dy = dy.contiguous()
    a = L.InstNormBwdArgs()
    a.instances, a.dtype, a.act, a.spatial = inst, L.dtype_code(x), ACT_CODES[act], S
    a.slope = float(slope)
    if y is not None and (y.shape != x.shape or y.dtype != x.dtype or not channel_dense(y)):
        raise RuntimeError("instnorm: y must match x (shape, dtype, dense channels)")
    dx = volume_empty(x.shape[0], x.shape[1], x.shape[2:], x.dtype, x.device)
    dres = volume_empty(x.shape[0], x.shape[1], x.shape[2:], x.dtype, x.device) if want_dresidual else None
    a.x_instance_stride, a.dy_instance_stride, a.dx_instance_stride = instance_stride(x), instance_stride(dy), instance_stride(dx)
    a.y_instance_stride = instance_stride(y) if y is not None else 0
    a.dresidual_instance_stride = instance_stride(dres) if dres is not None else 0
    ws_bytes = lib.dll.segm_instnorm_workspace_bytes(inst, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a.x, a.dy, a.y = x.data_ptr(), dy.data_ptr(), (y.data_ptr() if y is not None else None)
    a.mean, a.rstd, a.dx = mean.data_ptr(), rstd.data_ptr(), dx.data_ptr()
    a.dresidual = dres.data_ptr() if dres is not None else None
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws_bytes, L.stream_handle(x)
    lib.check(lib.dll.segm_instnorm_bwd(a), "instnorm_bwd")
    return dx, dres


def instnorm_tail_bwd(lib: L.SegmLib, x, skip, dy, mean, rstd, skip_mean, skip_rstd, y, act="leaky_relu", slope=0.01):
    """-> (dx, dskip) of y = act(IN(x) + IN(skip)) in one statistics and one apply pass (segm_instnorm_tail_bwd); `y` is needed iff
    act != none."""
    inst, S = _norm_geom(x)
    if dy.shape != x.shape or dy.dtype != x.dtype:
        raise RuntimeError("instnorm: dy must match x")
    if not channel_dense(dy):
        dy = dy.contiguous()
    for t in (skip, y):
        if t is not None and (t.shape != x.shape or t.dtype != x.dtype or not channel_dense(t)):
            raise RuntimeError("instnorm: skip and y must match x (shape, dtype, dense channels)")
    a = L.InstNormTailBwdArgs()
    a.instances, a.dtype, a.act, a.spatial = inst, L.dtype_code(x), ACT_CODES[act], S
    a.slope = float(slope)
    dx = volume_empty(x.shape[0], x.shape[1], x.shape[2:], x.dtype, x.device)
    dskip = volume_empty(x.shape[0], x.shape[1], x.shape[2:], x.dtype, x.device)
    a.x_instance_stride, a.skip_instance_stride, a.dy_instance_stride = instance_stride(x), instance_stride(skip), instance_stride(dy)
    a.dx_instance_stride, a.dskip_instance_stride = instance_stride(dx), instance_stride(dskip)
    a.y_instance_stride = instance_stride(y) if y is not None else 0
    ws_bytes = lib.dll.segm_instnorm_tail_workspace_bytes(inst, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a.x, a.skip, a.dy, a.y = x.data_ptr(), skip.data_ptr(), dy.data_ptr(), (y.data_ptr() if y is not None else None)
    a.mean, a.rstd, a.skip_mean, a.skip_rstd = mean.data_ptr(), rstd.data_ptr(), skip_mean.data_ptr(), skip_rstd.data_ptr()
    a.dx, a.dskip = dx.data_ptr(), dskip.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws_bytes, L.stream_handle(x)
    lib.check(lib.dll.segm_instnorm_tail_bwd(a), "instnorm_tail_bwd")
    return dx, dskip


# ---------------------------------------------------------------------------------------------------------
# depth-to-space / space-to-depth by 2 x 2 x 2 (the permute behind a kernel-2 stride-2 transposed convolution)
# ---------------------------------------------------------------------------------------------------------
def _d2s_shape_ok(t: torch.Tensor) -> bool:
    return t.dtype in (torch.bfloat16, torch.float16) and t.dim() == 5 and t.shape[4] % 8 == 0 and t.shape[1] % 8 == 0 and t.is_contiguous()


def depth_to_space2_supported(t: torch.Tensor) -> bool:
    return L.on_device(t) and _d2s_shape_ok(t)


def depth_to_space2(lib: L.SegmLib, blk: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """blk (B, C * 8, D, H, W) contiguous [channel index = ((c * 2 + i) * 2 + j) * 2 + k] -> vol (B, C, 2D, 2H, 2W) with
    vol[b, c, 2z+i, 2y+j, 2x+k] = blk[b, c, i, j, k, z, y, x]; `out`: a volume with unit x stride (e.g. ops_raw.volume_empty)."""
    B, C8, D, H, W = blk.shape
    if not _d2s_shape_ok(blk):
        raise RuntimeError("depth_to_space2: blk must be a contiguous 16-bit (B, C * 8, D, H, W) tensor with W % 8 == 0")
    Cc = C8 // 8
    if out is None:
        out = torch.empty(B, Cc, 2 * D, 2 * H, 2 * W, dtype=blk.dtype, device=blk.device)
    _d2s_call(lib, blk, out, 0)
    return out


def space_to_depth2(lib: L.SegmLib, vol: torch.Tensor) -> torch.Tensor:
    """the inverse gather: vol (B, C, 2D, 2H, 2W), unit x stride -> blk (B, C * 8, D, H, W) contiguous"""
    B, Cc, D2, H2, W2 = vol.shape
    if D2 % 2 or H2 % 2 or W2 % 16 or vol.dtype not in (torch.bfloat16, torch.float16) or vol.stride(4) != 1:
        raise RuntimeError("space_to_depth2: vol must be a 16-bit (B, C, 2D, 2H, 2W) tensor with unit x stride and 2W % 16 == 0")
    blk = torch.empty(B, Cc * 8, D2 // 2, H2 // 2, W2 // 2, dtype=vol.dtype, device=vol.device)
    _d2s_call(lib, blk, vol, 1)
    return blk


def _d2s_call(lib, blk, vol, direction):
    B, C8, D, H, W = blk.shape
    if tuple(vol.shape) != (B, C8 // 8, 2 * D, 2 * H, 2 * W) or vol.dtype != blk.dtype or vol.stride(4) != 1 or vol.device != blk.device:
        raise RuntimeError("depth_to_space2: vol must be (B, C, 2D, 2H, 2W) of blk's dtype with unit x stride")
    a = L.D2sArgs()
    a.batch, a.channels, a.depth, a.height, a.width = B, C8 // 8, D, H, W
    a.dtype, a.direction = L.dtype_code(blk), direction
    a.blk, a.vol = blk.data_ptr(), vol.data_ptr()
    a.vol_stride_b, a.vol_stride_c, a.vol_stride_z, a.vol_stride_y = vol.stride(0), vol.stride(1), vol.stride(2), vol.stride(3)
    a.stream = L.stream_handle(blk)
    lib.check(lib.dll.segm_depth_to_space2(a), "depth_to_space2")


# ---------------------------------------------------------------------------------------------------------
# channel-first <-> channel-last
# ---------------------------------------------------------------------------------------------------------
def add3_supported(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> bool:
    n = 4 if a.dtype == torch.float32 else 8
    return a.dtype in (torch.float32, torch.float16, torch.bfloat16) and a.shape == b.shape == c.shape and a.dtype == b.dtype == c.dtype \
        and a.is_contiguous() and b.is_contiguous() and c.is_contiguous() and a.numel() > 0 and a.numel() % n == 0 \
        and not ((a.data_ptr() | b.data_ptr() | c.data_ptr()) & 15)


def add3(lib: L.SegmLib, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a + b + c in one pass (fp32 sum, one rounding); `out` may be `a`."""
    if not add3_supported(a, b, c):
        raise RuntimeError("add3: three dense 16-byte aligned tensors of one shape and dtype")
    out = torch.empty_like(a) if out is None else out
    if out.shape != a.shape or out.dtype != a.dtype or not out.is_contiguous() or out.data_ptr() & 15:
        raise RuntimeError("add3: `out` must match the operands")
    p = L.Add3Args()
    p.count, p.dtype = a.numel(), L.dtype_code(a)
    p.a, p.b, p.c, p.out = a.data_ptr(), b.data_ptr(), c.data_ptr(), out.data_ptr()
    p.stream = L.stream_handle(a)
    lib.check(lib.dll.segm_add3(p), "add3")
    return out


def gather16_compact_map(idx: torch.Tensor) -> Optional[torch.Tensor]:
    """int32 (n,) source indices, n % 8 == 0 -> int32 (n / 8, 2) (first index, step) when every group of eight consecutive indices
    is an arithmetic progression (the packed weight layouts are: eight input channels of one (output channel, tap)), else None"""
    if idx.numel() == 0 or idx.numel() % 8:
        return None
    m = idx.view(-1, 8)
    step = m[:, 1] - m[:, 0]
    ar = torch.arange(8, dtype=idx.dtype, device=idx.device)
    if not bool((m == m[:, :1] + step[:, None] * ar).all()):
        return None
    return torch.stack([m[:, 0], step], 1).contiguous()


def gather16(lib: L.SegmLib, src: torch.Tensor, idx: torch.Tensor, out: torch.Tensor, compact: bool = False) -> torch.Tensor:
    """out[i] = src[idx[i]] (16-bit elements, one launch); `compact`: idx is gather16_compact_map's (n / 8, 2) form"""
    n = out.numel()
    if src.dtype not in (torch.bfloat16, torch.float16) or out.dtype != src.dtype or idx.dtype != torch.int32 or n % 8 or \
            not (src.is_contiguous() and out.is_contiguous() and idx.is_contiguous()) or idx.numel() != (n // 4 if compact else n) or \
            (out.data_ptr() | idx.data_ptr()) & 15:
        raise RuntimeError("gather16: 16-bit src / out, int32 map, whole 16-byte groups")
    p = L.Gather16Args()
    p.count, p.mode = n, 1 if compact else 0
    p.src, p.map, p.out = src.data_ptr(), idx.data_ptr(), out.data_ptr()
    p.stream = L.stream_handle(out)
    lib.check(lib.dll.segm_gather16(p), "gather16")
    return out


def transpose_add(lib: L.SegmLib, x: torch.Tensor, add: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, R, C) contiguous -> (B, C, R) contiguous (+ add, which already has the output layout)."""
    if x.dim() != 3 or not x.is_contiguous():
        raise RuntimeError("transpose_add: x must be a contiguous (B, R, C) tensor")
    B, R, Cc = x.shape
    out = torch.empty(B, Cc, R, dtype=x.dtype, device=x.device)
    if add is not None and (add.shape != out.shape or add.dtype != x.dtype or not add.is_contiguous()):
        raise RuntimeError("transpose_add: add must be a contiguous (B, C, R) tensor of x's dtype")
    a = L.TransposeArgs()
    a.batch, a.rows, a.cols, a.dtype = B, R, Cc, L.dtype_code(x)
    a.in_, a.add, a.out = x.data_ptr(), (add.data_ptr() if add is not None else None), out.data_ptr()
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_transpose_add(a), "transpose_add")
    return out


# ---------------------------------------------------------------------------------------------------------
# volume -> tokens with LayerNorm
# ---------------------------------------------------------------------------------------------------------
def layernorm_tokens_supported(x: torch.Tensor) -> bool:
    if x.dim() != 3 or not x.is_contiguous() or x.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        return False
    n = 4 if x.dtype == torch.float32 else 8
    return x.shape[1] % n == 0 and x.shape[2] % n == 0 and x.shape[1] <= (192 if x.dtype == torch.float32 else 384)


def _ln_args(x, gamma, eps):
    B, Cc, S = x.shape
    a = L.LayerNormArgs()
    a.batch, a.channels, a.dtype, a.spatial, a.eps = B, Cc, L.dtype_code(x), S, float(eps)
    a.x, a.gamma, a.stream = x.data_ptr(), gamma.data_ptr(), L.stream_handle(x)
    return a


def layernorm_tokens_fwd(lib: L.SegmLib, x, gamma, beta, eps=1e-5):
    """x (B, C, S) contiguous -> (y (B, S, C), mean (B, S), rstd (B, S)); gamma / beta fp32 (C)."""
    if not layernorm_tokens_supported(x):
        raise RuntimeError("layernorm_tokens: unsupported shape / dtype / layout")
    B, Cc, S = x.shape
    gamma, beta = gamma.float().contiguous(), beta.float().contiguous()
    y = torch.empty(B, S, Cc, dtype=x.dtype, device=x.device)
    mean = torch.empty(B, S, dtype=torch.float32, device=x.device)
    rstd = torch.empty(B, S, dtype=torch.float32, device=x.device)
    a = _ln_args(x, gamma, eps)
    a.y, a.beta, a.mean, a.rstd = y.data_ptr(), beta.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    lib.check(lib.dll.segm_layernorm_tokens_fwd(a), "layernorm_tokens_fwd")
    return y, mean, rstd


def layernorm_tokens_bwd(lib: L.SegmLib, x, dy, mean, rstd, gamma):
    """-> (dx (B, C, S), dgamma (C) fp32, dbeta (C) fp32)."""
    B, Cc, S = x.shape
    if dy.shape != (B, S, Cc) or dy.dtype != x.dtype:
        raise RuntimeError("layernorm_tokens: dy must be (B, S, C) of x's dtype")
    dy = dy.contiguous()
    gamma = gamma.float().contiguous()
    dx = torch.empty_like(x)
    dgamma = torch.empty(Cc, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(Cc, dtype=torch.float32, device=x.device)
    ws_bytes = lib.dll.segm_layernorm_tokens_workspace_bytes(B, Cc, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a = _ln_args(x, gamma, 0.0)
    a.mean, a.rstd, a.dy, a.dx = mean.data_ptr(), rstd.data_ptr(), dy.data_ptr(), dx.data_ptr()
    a.dgamma, a.dbeta = dgamma.data_ptr(), dbeta.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    lib.check(lib.dll.segm_layernorm_tokens_bwd(a), "layernorm_tokens_bwd")
    return dx, dgamma, dbeta


# ---------------------------------------------------------------------------------------------------------
# training-step glue: gradient clipping + SGD over a tensor list, cross entropy with its gradient
# ---------------------------------------------------------------------------------------------------------
def sgd_clip_step(lib: L.SegmLib, params, grads, momenta, lr: float, momentum: float, weight_decay: float,
                  nesterov: bool, max_norm: float, loss_scale: Optional[torch.Tensor] = None,
                  found_inf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """In place: clip_grad_norm_(max_norm) + SGD step over lists of contiguous fp32 tensors (params / momenta updated,
    grads only read).  Returns the 4-float workspace head {update coefficient, gradient norm, skipped, -} (device tensor).
    loss_scale (1-element fp32 device tensor): the gradients carry that factor (GradScaler) - the norm and the clip are those of
    the unscaled gradients, and a non-finite norm skips the step and writes 1 to `found_inf` (1-element fp32), else 0."""
    n = len(params)
    if not (len(grads) == len(momenta) == n):
        raise RuntimeError("sgd_clip_step: params, grads and momenta must have the same length")
    if n == 0:
        return torch.ones(4)
    for p, g, m in zip(params, grads, momenta):
        if not (p.dtype == g.dtype == m.dtype == torch.float32) or not (p.is_contiguous() and g.is_contiguous() and m.is_contiguous()) \
                or not (p.numel() == g.numel() == m.numel()) or not (p.device == g.device == m.device == params[0].device):
            raise RuntimeError("sgd_clip_step: tensors must be contiguous fp32, same size per entry, one device")
    ptr_t, i64_t = C.c_void_p * n, C.c_int64 * n
    pp, gp, mp = ptr_t(*[p.data_ptr() for p in params]), ptr_t(*[g.data_ptr() for g in grads]), ptr_t(*[m.data_ptr() for m in momenta])
    ne = i64_t(*[p.numel() for p in params])
    ws_bytes = lib.dll.segm_sgd_clip_step_workspace_bytes(n, C.cast(ne, C.c_void_p))
    ws = torch.empty((ws_bytes + 3) // 4, dtype=torch.float32, device=params[0].device)
    a = L.SgdArgs()
    a.ntensors, a.nesterov = n, int(bool(nesterov))
    a.params, a.grads, a.momenta, a.numel = C.cast(pp, C.c_void_p), C.cast(gp, C.c_void_p), C.cast(mp, C.c_void_p), C.cast(ne, C.c_void_p)
    a.lr, a.momentum, a.weight_decay, a.max_norm = lr, momentum, weight_decay, max_norm
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws_bytes
    a.stream = L.stream_handle(params[0])
    for t in (loss_scale, found_inf):
        if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != params[0].device):
            raise RuntimeError("sgd_clip_step: loss_scale / found_inf must be 1-element fp32 tensors on the parameters' device")
    a.loss_scale = loss_scale.data_ptr() if loss_scale is not None else None
    a.found_inf = found_inf.data_ptr() if found_inf is not None else None
    lib.check(lib.dll.segm_sgd_clip_step(a), "sgd_clip_step")
    return ws[:4]


def cross_entropy_supported(logits: torch.Tensor, labels: torch.Tensor) -> bool:
    return logits.dim() >= 2 and 1 <= logits.shape[1] <= 16 and labels.dtype == torch.int64 and \
        logits.dtype in (torch.float32, torch.float16, torch.bfloat16) and \
        tuple(labels.shape) == (logits.shape[0],) + tuple(logits.shape[2:]) and logits.numel() > 0


def cross_entropy(lib: L.SegmLib, logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100):
    """-> (loss_sum fp32 scalar, count fp32 scalar, dlogits): sum over counted voxels of the cross entropy, the number of
    counted voxels, and d(loss_sum)/d(logits) (logits' dtype and shape)."""
    if not cross_entropy_supported(logits, labels):
        raise RuntimeError("cross_entropy: logits (B, C <= 16, *spatial) fp32 / fp16 / bf16 and int64 labels (B, *spatial)")
    logits, labels = logits.contiguous(), labels.contiguous()
    B, Cc = logits.shape[:2]
    S = logits.numel() // (B * Cc)
    nparts = lib.dll.segm_cross_entropy_partials(B, S)
    parts = torch.empty(2, nparts, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits)
    a = L.CrossEntropyArgs()
    a.batch, a.classes, a.dtype = B, Cc, L.dtype_code(logits)
    a.spatial, a.ignore_index = S, ignore_index
    a.logits, a.labels, a.dlogits = logits.data_ptr(), labels.data_ptr(), dlogits.data_ptr()
    a.loss_partial, a.count_partial = parts[0].data_ptr(), parts[1].data_ptr()
    a.stream = L.stream_handle(logits)
    lib.check(lib.dll.segm_cross_entropy(a), "cross_entropy")
    tot = parts.sum(1)
    return tot[0], tot[1], dlogits


def _ce_map_args(logits: torch.Tensor, labels: torch.Tensor, ignore_index: int, what: str):
    if not cross_entropy_supported(logits, labels):
        raise RuntimeError(f"{what}: logits (B, C <= 16, *spatial) fp32 / fp16 / bf16 and int64 labels (B, *spatial)")
    if labels.device != logits.device:
        raise RuntimeError(f"{what}: the labels lie on {labels.device}, the logits on {logits.device}")
    logits, labels = logits.contiguous(), labels.contiguous()
    B, Cc = logits.shape[:2]
    S = logits.numel() // (B * Cc)
    if B * S >= 1 << 31:
        raise RuntimeError(f"{what}: {B * S} voxels, fewer than 2^31 are supported")
    a = L.CrossEntropyMapArgs()
    a.batch, a.classes, a.dtype = B, Cc, L.dtype_code(logits)
    a.spatial, a.ignore_index = S, ignore_index
    a.logits, a.labels = logits.data_ptr(), labels.data_ptr()
    a.stream = L.stream_handle(logits)
    return a, logits, labels


def cross_entropy_map(lib: L.SegmLib, logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100) -> torch.Tensor:
    """-> the per-voxel cross entropy, fp32 (B, *spatial): logsumexp - x[label]; 0 where the label is ignored; NaN where it is outside
    [0, C) and not ignored.  `F.cross_entropy(reduction="none")` without the fp32 copy of the logits."""
    a, logits, labels = _ce_map_args(logits, labels, ignore_index, "cross_entropy_map")
    out = torch.empty(labels.shape, dtype=torch.float32, device=logits.device)
    a.loss_map = out.data_ptr()
    lib.check(lib.dll.segm_cross_entropy_map(a), "cross_entropy_map")
    return out


def topk_select(lib: L.SegmLib, values: torch.Tensor, kk: int, workspace: torch.Tensor = None) -> torch.Tensor:
    """values: contiguous fp32, n < 2^31 elements; kk in [1, n].  -> 32 bytes on the device as int64 (4,): view(float32)[0] the kk-th
    largest value (a positive NaN sorts above +inf), [1] n_gt and [2] n_eq, the number of values above / equal to it, view(float64)[3]
    the fp64 sum of the values above.  Exact: radix selection, three histogram passes and one for the sum, nothing is read back."""
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or not values.is_contiguous():
        raise RuntimeError("topk_select: values must be a contiguous fp32 tensor")
    n, kk = values.numel(), int(kk)
    if not 1 <= n < 1 << 31:
        raise RuntimeError(f"topk_select: 1 .. 2^31 - 1 values, got {n}")
    if not 1 <= kk <= n:
        raise RuntimeError(f"topk_select: kk must lie in [1, {n}], got {kk}")
    nbytes = lib.dll.segm_topk_select_workspace_bytes(n)
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=values.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != values.device or not workspace.is_contiguous():
        raise RuntimeError("topk_select: the workspace must be a contiguous tensor on the values' device")
    result = torch.empty(L.TOPK_RESULT_BYTES // 8, dtype=torch.int64, device=values.device)
    a = L.TopkSelectArgs()
    a.values, a.n, a.kk, a.result = values.data_ptr(), n, kk, result.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    a.stream = L.stream_handle(values)
    lib.check(lib.dll.segm_topk_select(a), "topk_select")
    return result


def cross_entropy_map_bwd(lib: L.SegmLib, logits: torch.Tensor, labels: torch.Tensor, ignore_index: int = -100,
                          coef: torch.Tensor = None, scale: torch.Tensor = None, loss_map: torch.Tensor = None,
                          select: torch.Tensor = None, kk: int = 0) -> torch.Tensor:
    """-> dlogits = g (softmax - onehot) in the logits' dtype and shape; 0 where the label is ignored, NaN where it is wrong.  g is the
    product of whichever are given: `coef` fp32 (B, *spatial); `scale`, a 1-element fp32 tensor; the top-k weight formed from
    `loss_map` (what `cross_entropy_map` returned), `select` (what `topk_select` returned for it) and `kk`."""
    a, logits, labels = _ce_map_args(logits, labels, ignore_index, "cross_entropy_map_bwd")
    dev = logits.device
    if coef is not None:
        if coef.dtype != torch.float32 or tuple(coef.shape) != tuple(labels.shape) or coef.device != dev:
            raise RuntimeError("cross_entropy_map_bwd: coef must be fp32 of the labels' shape on the logits' device")
        coef = coef.contiguous()
        a.coef = coef.data_ptr()
    if scale is not None:
        if scale.dtype != torch.float32 or scale.numel() != 1 or scale.device != dev:
            raise RuntimeError("cross_entropy_map_bwd: scale must be a 1-element fp32 tensor on the logits' device")
        a.scale = scale.data_ptr()
    if (loss_map is None) != (select is None):
        raise RuntimeError("cross_entropy_map_bwd: the top-k weight needs both loss_map and select")
    if select is not None:
        if loss_map.dtype != torch.float32 or tuple(loss_map.shape) != tuple(labels.shape) or loss_map.device != dev or \
                not loss_map.is_contiguous():
            raise RuntimeError("cross_entropy_map_bwd: loss_map must be contiguous fp32 of the labels' shape on the logits' device")
        if select.dtype != torch.int64 or select.numel() != L.TOPK_RESULT_BYTES // 8 or select.device != dev or not select.is_contiguous():
            raise RuntimeError("cross_entropy_map_bwd: select must be the int64 (4,) tensor topk_select returned")
        if not 1 <= int(kk) <= labels.numel():
            raise RuntimeError(f"cross_entropy_map_bwd: kk must lie in [1, {labels.numel()}], got {kk}")
        a.loss_map, a.select, a.kk = loss_map.data_ptr(), select.data_ptr(), int(kk)
    dlogits = torch.empty_like(logits)
    a.dlogits = dlogits.data_ptr()
    lib.check(lib.dll.segm_cross_entropy_map_bwd(a), "cross_entropy_map_bwd")
    return dlogits


def _loss_layout(logits: torch.Tensor):
    """the spatial axes of (B, n, *spatial) logits as (z, y, x) - x the last axis, y the one before, z whatever lies in front, which
    one stride must serve -> (Z, Y, X, stride_z, stride_y), or None where the strides do not allow it"""
    sp, st = tuple(logits.shape[2:]), logits.stride()
    X = sp[-1]
    Y = sp[-2] if len(sp) >= 2 else 1
    Z = 1
    for s in sp[:-2]:
        Z *= s
    if X != 1 and st[-1] != 1:
        return None
    sy = st[-2] if len(sp) >= 2 and Y != 1 else X
    lead = [(sp[i], st[2 + i]) for i in range(len(sp) - 2) if sp[i] != 1]
    sz = X * Y
    if lead:
        sz = lead[-1][1]
        for (_, s_out), (n_in, s_in) in zip(lead[:-1], lead[1:]):
            if s_out != s_in * n_in:
                return None
    return Z, Y, X, sz, sy


def region_loss_layout_supported(logits: torch.Tensor) -> bool:
    """whether the region-loss entries take these logits as they lie in memory (a caller may pass a dense copy otherwise)"""
    return logits.dim() >= 3 and logits.numel() > 0 and _loss_layout(logits) is not None


def softmax_dice_layout_supported(logits: torch.Tensor) -> bool:
    """whether the softmax-Dice entries take these logits as they lie in memory (a caller may pass a dense copy otherwise)"""
    return region_loss_layout_supported(logits)


def _loss_logits_args(a, logits: torch.Tensor, other: torch.Tensor, other_name: str, planes: str, limit: int, what: str) -> None:
    """the checks of the logits (B, n, *spatial) that the region-loss and the softmax-Dice entries share, and the fields of their
    argument structs that describe them.  `planes` is "regions" or "classes": the struct's field for n, and the stride field by its
    first letter; `other` is the target / the labels, which must be a tensor on the logits' device."""
    if not isinstance(logits, torch.Tensor) or not isinstance(other, torch.Tensor):
        raise RuntimeError(f"{what}: logits and {other_name} must be tensors")
    if logits.dim() < 3 or logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise RuntimeError(f"{what}: logits (B, {planes[0].upper()}, *spatial) fp32 / fp16 / bf16")
    B, n = logits.shape[:2]
    if not 1 <= n <= limit:
        raise RuntimeError(f"{what}: 1 .. {limit} {planes}, got {n}")
    if logits.numel() == 0:
        raise RuntimeError(f"{what}: empty logits {tuple(logits.shape)}")
    if other.device != logits.device:
        raise RuntimeError(f"{what}: {other_name} on {other.device}, the logits on {logits.device}")
    V = 1
    for s in logits.shape[2:]:
        V *= s
    if V >= 1 << 31:
        raise RuntimeError(f"{what}: {V} voxels per sample, fewer than 2^31 are supported")
    layout = _loss_layout(logits)
    if layout is None:
        raise RuntimeError(f"{what}: the logits need unit stride along the last axis and spatial axes in front of the last two "
                           f"that collapse into one stride, got strides {logits.stride()} for {tuple(logits.shape)}")
    st = logits.stride()
    a.batch, a.dtype = B, L.dtype_code(logits)
    setattr(a, planes, n)
    setattr(a, "stride_" + planes[0], st[1])
    a.depth, a.height, a.width, a.stride_z, a.stride_y = layout
    a.stride_b, a.stride_x = st[0], 1
    a.logits, a.stream = logits.data_ptr(), L.stream_handle(logits)


def _loss_ignore_label(a, ignore_label, what: str) -> None:
    if ignore_label is not None:
        if not -(1 << 63) <= int(ignore_label) < 1 << 63:
            raise RuntimeError(f"{what}: ignore_label {ignore_label} is no 64-bit integer")
        a.has_ignore, a.ignore_label = 1, int(ignore_label)


def _loss_workspace(a, nbytes: int, workspace, logits: torch.Tensor, what: str) -> torch.Tensor:
    """the forward's workspace of `nbytes` (what the entry's *_workspace_bytes answered), allocated unless the caller brings one"""
    if nbytes == 0:
        raise RuntimeError(f"{what}: the shape {tuple(logits.shape)} is out of range")
    if workspace is None:
        workspace = torch.empty(nbytes // 8, dtype=torch.float64, device=logits.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != logits.device or not workspace.is_contiguous():
        raise RuntimeError(f"{what}: the workspace must be a contiguous tensor on the logits' device")
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return workspace


def _loss_coefs(coefs, logits: torch.Tensor, what: str):
    """the backward's coefficients, (name, tensor, shape) each: fp32 of that shape on the logits' device -> them, contiguous"""
    out = []
    for name, g, shape in coefs:
        if not isinstance(g, torch.Tensor) or g.dtype != torch.float32 or tuple(g.shape) != shape or g.device != logits.device:
            raise RuntimeError(f"{what}: {name} must be fp32 {shape} on the logits' device")
        out.append(g.contiguous())
    return out


def _region_args(logits: torch.Tensor, target: torch.Tensor, masks, ignore_label, ignore_plane: bool, what: str):
    """the checks and the argument struct the two region-loss entries share -> (args, target kept alive)"""
    a = L.RegionLossArgs()
    _loss_logits_args(a, logits, target, "target", "regions", L.REGION_MAX_REGIONS, what)
    B, R = logits.shape[:2]
    sp = tuple(logits.shape[2:])
    if masks is not None:
        if ignore_plane:
            raise RuntimeError(f"{what}: an ignore plane belongs to a plane target, not to a label map")
        masks = [int(m) for m in masks]
        if len(masks) != R or any(not 0 <= m < 1 << 32 for m in masks):
            raise RuntimeError(f"{what}: {R} membership masks of 32 bits, got {masks}")
        if tuple(target.shape) != (B,) + sp or target.dtype not in L.REGION_LABELS:
            raise RuntimeError(f"{what}: a label map {(B,) + sp} of int64 / int16 / uint8 / float32, got {tuple(target.shape)} "
                               f"{target.dtype}")
        a.target_kind = L.REGION_LABELS[target.dtype]
        for r, m in enumerate(masks):
            a.masks[r] = m
        _loss_ignore_label(a, ignore_label, what)
    else:
        if ignore_label is not None:
            raise RuntimeError(f"{what}: ignore_label belongs to a label map (pass masks), a plane target takes ignore_plane")
        if target.dtype == torch.bool:
            target = target.contiguous().view(torch.uint8)
        planes = R + (1 if ignore_plane else 0)
        if tuple(target.shape) != (B, planes) + sp or target.dtype not in L.REGION_PLANES:
            raise RuntimeError(f"{what}: a plane target {(B, planes) + sp} of uint8 / bool / float32, got {tuple(target.shape)} "
                               f"{target.dtype}")
        a.target_kind, a.ignore_plane = L.REGION_PLANES[target.dtype], int(bool(ignore_plane))
    target = target.contiguous()
    a.target = target.data_ptr()
    return a, target


def region_loss_fwd(lib: L.SegmLib, logits: torch.Tensor, target: torch.Tensor, masks=None, ignore_label: int = None,
                    ignore_plane: bool = False, workspace: torch.Tensor = None):
    """The sums of the region-based loss, float64 on the device: -> (I, P, G, E) of shape (B, R) and N of shape (B).  With
    p = sigmoid(logits): I = sum m p t, P = sum m p, G = sum m t, E = sum m (max(x, 0) - x t + log1p(exp(-|x|))), N = sum m.
    logits (B, R <= 8, *spatial) fp32 / fp16 / bf16, unit stride along the last axis, any batch / region / row strides.
    `masks` given: target is a label map (B, *spatial) int64 / int16 / uint8 / float32 and t = (masks[r] >> label) & 1; a label equal
    to `ignore_label` has m = 0; any other label outside [0, 32) gives NaN in its sample's I, P, E.  `masks` None: target holds the
    planes (B, R, *spatial) - or (B, R + 1, *spatial) with `ignore_plane`, m = ((1 - last) != 0) - of uint8 / bool / float32."""
    a, target = _region_args(logits, target, masks, ignore_label, ignore_plane, "region_loss_fwd")
    B, R = logits.shape[:2]
    nbytes = lib.dll.segm_region_loss_workspace_bytes(B, R, a.depth * a.height * a.width)
    workspace = _loss_workspace(a, nbytes, workspace, logits, "region_loss_fwd")
    sums = torch.empty(4 * B * R + B, dtype=torch.float64, device=logits.device)
    a.sums = sums.data_ptr()
    lib.check(lib.dll.segm_region_loss_fwd(a), "region_loss_fwd")
    four = sums[:4 * B * R].view(4, B, R)
    return four[0], four[1], four[2], four[3], sums[4 * B * R:]


def region_loss_bwd(lib: L.SegmLib, logits: torch.Tensor, target: torch.Tensor, g_i: torch.Tensor, g_p: torch.Tensor,
                    g_e: torch.Tensor, masks=None, ignore_label: int = None, ignore_plane: bool = False) -> torch.Tensor:
    """-> dlogits = m (p (1 - p) (g_i t + g_p) + g_e (p - t)), dense, in the logits' dtype and shape; exactly 0 where m = 0, NaN at a
    wrong label.  g_i, g_p, g_e: fp32 (B, R) on the logits' device, the gradients of the loss by I, P and E of `region_loss_fwd`;
    the other arguments as there."""
    a, target = _region_args(logits, target, masks, ignore_label, ignore_plane, "region_loss_bwd")
    BR = tuple(logits.shape[:2])
    coefs = _loss_coefs((("g_i", g_i, BR), ("g_p", g_p, BR), ("g_e", g_e, BR)), logits, "region_loss_bwd")
    a.g_i, a.g_p, a.g_e = (g.data_ptr() for g in coefs)
    dlogits = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    a.dlogits = dlogits.data_ptr()
    lib.check(lib.dll.segm_region_loss_bwd(a), "region_loss_bwd")
    return dlogits


def _softmax_dice_args(logits: torch.Tensor, labels: torch.Tensor, mask, ignore_label, what: str):
    """the checks and the argument struct the two softmax-Dice entries share -> (args, the tensors kept alive)"""
    a = L.SoftmaxDiceArgs()
    _loss_logits_args(a, logits, labels, "labels", "classes", L.SOFTMAX_DICE_MAX_CLASSES, what)
    shape = (logits.shape[0],) + tuple(logits.shape[2:])
    if tuple(labels.shape) != shape or labels.dtype not in L.REGION_LABELS:
        raise RuntimeError(f"{what}: a label map {shape} of int64 / int16 / uint8 / float32, got {tuple(labels.shape)} {labels.dtype}")
    a.label_kind = L.REGION_LABELS[labels.dtype]
    _loss_ignore_label(a, ignore_label, what)
    labels = labels.contiguous()
    keep = [labels]
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or tuple(mask.shape) != shape or mask.device != logits.device:
            raise RuntimeError(f"{what}: the mask must be uint8 {shape} on the logits' device")
        mask = mask.contiguous()
        keep.append(mask)
        a.mask = mask.data_ptr()
    a.labels = labels.data_ptr()
    return a, keep


def softmax_dice_fwd(lib: L.SegmLib, logits: torch.Tensor, labels: torch.Tensor, mask: torch.Tensor = None, ignore_label: int = None,
                     workspace: torch.Tensor = None):
    """The sums of softmax Dice + cross entropy, float64 on the device: -> (I, P, G) of shape (B, C) and (CE, N) of shape (B).  With
    p = softmax(logits, 1): I = sum m p_c [y = c], P = sum m p_c, G = sum m [y = c], CE = sum m (logsumexp(x) - x_y), N = sum m.
    logits (B, C <= 16, *spatial) fp32 / fp16 / bf16, unit stride along the last axis, any batch / class / row strides; labels
    (B, *spatial) int64 / int16 / uint8 / float32; mask optional, uint8 (B, *spatial).  m = 0 where the label equals `ignore_label`
    or the mask is 0; any other label outside [0, C), or a float label that is no integer, gives NaN in its sample's I, P, CE."""
    a, keep = _softmax_dice_args(logits, labels, mask, ignore_label, "softmax_dice_fwd")
    B, Cc = logits.shape[:2]
    nbytes = lib.dll.segm_softmax_dice_workspace_bytes(B, Cc, a.depth * a.height * a.width)
    workspace = _loss_workspace(a, nbytes, workspace, logits, "softmax_dice_fwd")
    sums = torch.empty(3 * B * Cc + 2 * B, dtype=torch.float64, device=logits.device)
    a.sums = sums.data_ptr()
    lib.check(lib.dll.segm_softmax_dice_fwd(a), "softmax_dice_fwd")
    three = sums[:3 * B * Cc].view(3, B, Cc)
    two = sums[3 * B * Cc:].view(2, B)
    return three[0], three[1], three[2], two[0], two[1]


def softmax_dice_bwd(lib: L.SegmLib, logits: torch.Tensor, labels: torch.Tensor, g_i: torch.Tensor, g_p: torch.Tensor,
                     g_ce: torch.Tensor, mask: torch.Tensor = None, ignore_label: int = None) -> torch.Tensor:
    """-> dlogits_j = m (p_j (a_j - S) + g_ce (p_j - [j = y])), a_c = g_i[c] [y = c] + g_p[c], S = sum_c p_c a_c: dense, in the
    logits' dtype and shape; exactly 0 where m = 0, NaN at a wrong label.  g_i, g_p: fp32 (B, C), g_ce: fp32 (B), on the logits'
    device - the gradients of the loss by I, P and CE of `softmax_dice_fwd`; the other arguments as there."""
    a, keep = _softmax_dice_args(logits, labels, mask, ignore_label, "softmax_dice_bwd")
    BC = tuple(logits.shape[:2])
    coefs = _loss_coefs((("g_i", g_i, BC), ("g_p", g_p, BC), ("g_ce", g_ce, BC[:1])), logits, "softmax_dice_bwd")
    a.g_i, a.g_p, a.g_ce = (g.data_ptr() for g in coefs)
    dlogits = torch.empty(logits.shape, dtype=logits.dtype, device=logits.device)
    a.dlogits = dlogits.data_ptr()
    lib.check(lib.dll.segm_softmax_dice_bwd(a), "softmax_dice_bwd")
    return dlogits


# ---------------------------------------------------------------------------------------------------------
# single-token decode steps
# ---------------------------------------------------------------------------------------------------------
def conv1d_update(lib: L.SegmLib, x, conv_state, weight, bias=None, silu=False):
    """x (B, D), conv_state (B, D, W) updated in place, weight (D, W) / bias (D) fp32 -> out (B, D) of x's dtype."""
    if x.dim() != 2 or conv_state.dim() != 3 or tuple(conv_state.shape[:2]) != tuple(x.shape) or conv_state.dtype != x.dtype:
        raise RuntimeError("conv1d_update: x (B, D) and conv_state (B, D, W) of one dtype")
    B, D = x.shape
    W = conv_state.shape[2]
    if tuple(weight.shape) != (D, W) or weight.dtype != torch.float32 or not weight.is_contiguous():
        raise RuntimeError("conv1d_update: weight must be a contiguous fp32 (D, W) tensor")
    if bias is not None and (tuple(bias.shape) != (D,) or bias.dtype != torch.float32 or not bias.is_contiguous()):
        raise RuntimeError("conv1d_update: bias must be a contiguous fp32 (D) tensor")
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    a = L.Conv1dUpdateArgs()
    a.batch, a.dim, a.width, a.silu, a.dtype = B, D, W, int(bool(silu)), L.dtype_code(x)
    a.x, a.x_stride_b, a.x_stride_d = x.data_ptr(), x.stride(0), x.stride(1)
    a.conv_state = conv_state.data_ptr()
    a.state_stride_b, a.state_stride_d, a.state_stride_w = conv_state.stride()
    a.out, a.out_stride_b, a.out_stride_d = out.data_ptr(), out.stride(0), out.stride(1)
    a.weight, a.bias, a.stream = weight.data_ptr(), L.fptr(bias), L.stream_handle(x)
    lib.check(lib.dll.segm_causal_conv1d_update(a), "causal_conv1d_update")
    return out


def state_update(lib: L.SegmLib, state, x, dt, A, Bm, Cm, D=None, z=None, dt_bias=None, dt_softplus=False):
    """state (B, D, N) updated in place; x, dt, z (B, D); Bm, Cm (B, N); A (D, N), D, dt_bias (D) fp32 -> out (B, D)."""
    if state.dim() != 3 or x.dim() != 2 or tuple(state.shape[:2]) != tuple(x.shape):
        raise RuntimeError("state_update: state (B, D, N), x (B, D)")
    B, Dm, N = state.shape
    for name, t, shape in (("dt", dt, (B, Dm)), ("B", Bm, (B, N)), ("C", Cm, (B, N))) + ((("z", z, (B, Dm)),) if z is not None else ()):
        if tuple(t.shape) != shape or t.dtype != x.dtype:
            raise RuntimeError(f"state_update: {name} must be {shape} of x's dtype")
    for name, t, shape in (("A", A, (Dm, N)),) + ((("D", D, (Dm,)),) if D is not None else ()) + \
            ((("dt_bias", dt_bias, (Dm,)),) if dt_bias is not None else ()):
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"state_update: {name} must be a contiguous fp32 {shape} tensor")
    out = torch.empty_like(x, memory_format=torch.contiguous_format)
    a = L.StateUpdateArgs()
    a.batch, a.dim, a.dstate, a.dt_softplus = B, Dm, N, int(bool(dt_softplus))
    a.dtype, a.state_dtype = L.dtype_code(x), L.dtype_code(state)
    a.state = state.data_ptr()
    a.state_stride_b, a.state_stride_d, a.state_stride_n = state.stride()
    for name, t in (("x", x), ("dt", dt), ("out", out)):
        setattr(a, name, t.data_ptr()); setattr(a, name + "_stride_b", t.stride(0)); setattr(a, name + "_stride_d", t.stride(1))
    if z is not None:
        a.z, a.z_stride_b, a.z_stride_d = z.data_ptr(), z.stride(0), z.stride(1)
    a.B, a.B_stride_b, a.B_stride_n = Bm.data_ptr(), Bm.stride(0), Bm.stride(1)
    a.C, a.C_stride_b, a.C_stride_n = Cm.data_ptr(), Cm.stride(0), Cm.stride(1)
    a.A, a.D, a.dt_bias, a.stream = A.data_ptr(), L.fptr(D), L.fptr(dt_bias), L.stream_handle(x)
    lib.check(lib.dll.segm_selective_state_update(a), "selective_state_update")
    return out


# ---------------------------------------------------------------------------------------------------------
# row-streaming projection (tall activations)
# ---------------------------------------------------------------------------------------------------------
def linear_rows_supported(x2: torch.Tensor, w: torch.Tensor, n_out: Optional[int] = None) -> bool:
    """x2 (rows, K) view with unit column stride, w (N, K)."""
    if x2.dim() != 2 or w.dim() != 2 or x2.dtype not in (torch.bfloat16, torch.float16) or w.dtype != x2.dtype:
        return False
    K, N = x2.shape[1], w.shape[0]
    return w.shape[1] == K and K % 8 == 0 and K <= 2048 and N % 4 == 0 and x2.stride(1) == 1 and x2.stride(0) % 8 == 0 and \
        x2.data_ptr() % 16 == 0 and x2.shape[0] > 0


def linear_rows(lib: L.SegmLib, x2: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None,
                out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """y (rows, N) = x2 (rows, K) @ w (N, K)^T + bias; `out` may be a column slice of a wider row-major tensor;
    `accumulate` adds to what `out` holds."""
    if not linear_rows_supported(x2, w):
        raise RuntimeError("linear_rows: x (rows, K <= 2048, K % 8 == 0) with unit column stride and 16-byte rows, w (N % 4 == 0, K), bf16 / fp16")
    M, K = x2.shape
    N = w.shape[0]
    w = w.contiguous()
    y = torch.empty(M, N, dtype=x2.dtype, device=x2.device) if out is None else out
    if tuple(y.shape) != (M, N) or y.dtype != x2.dtype or y.stride(1) != 1 or y.stride(0) % 4 or y.data_ptr() % 8:
        raise RuntimeError("linear_rows: `out` must be (rows, N) of x's dtype, unit column stride, 8-byte rows")
    if bias is not None:
        bias = bias.float().contiguous()
    a = L.LinearArgs()
    if accumulate and out is None:
        raise RuntimeError("linear_rows: accumulate needs `out`")
    a.rows, a.k, a.n, a.dtype, a.accumulate = M, K, N, L.dtype_code(x2), int(bool(accumulate))
    a.x, a.x_stride_row = x2.data_ptr(), x2.stride(0)
    a.w, a.bias = w.data_ptr(), L.fptr(bias)
    a.y, a.y_stride_row = y.data_ptr(), y.stride(0)
    a.stream = L.stream_handle(x2)
    lib.check(lib.dll.segm_linear_rows(a), "linear_rows")
    return y


def skinny_tn_supported(wide: torch.Tensor, skinny: torch.Tensor) -> bool:
    return bool(wide.dim() == 2 and skinny.dim() == 2 and wide.shape[0] == skinny.shape[0] and skinny.shape[1] <= 32 and
                wide.dtype in (torch.bfloat16, torch.float16) and skinny.dtype == wide.dtype and wide.stride(1) == 1 and
                skinny.stride(1) == 1 and wide.shape[0] > 0 and
                # whole rows as 16-byte loads: eight channels per thread, at most 256 threads per row
                wide.shape[1] % 8 == 0 and wide.shape[1] <= 2048 and wide.stride(0) % 8 == 0 and wide.data_ptr() % 16 == 0)


def skinny_tn(lib: L.SegmLib, wide: torch.Tensor, skinny: torch.Tensor) -> torch.Tensor:
    """wide (k, m)^T @ skinny (k, n <= 32) -> (m, n) fp32: the dt_proj weight gradient as a streaming reduction"""
    if not skinny_tn_supported(wide, skinny):
        raise RuntimeError("skinny_tn: wide (k, m % 8 == 0, m <= 2048, 16-byte aligned rows), skinny (k, n <= 32), one 16-bit dtype, unit column strides")
    K, M = wide.shape
    N = skinny.shape[1]
    out = torch.empty(M, N, dtype=torch.float32, device=wide.device)
    ws_bytes = lib.dll.segm_skinny_tn_workspace_bytes(M, N, K)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=wide.device)
    a = L.SkinnyTnArgs()
    a.k, a.m, a.n, a.dtype = K, M, N, L.dtype_code(wide)
    a.wide, a.wide_stride_row = wide.data_ptr(), wide.stride(0)
    a.skinny, a.skinny_stride_row = skinny.data_ptr(), skinny.stride(0)
    a.out, a.workspace, a.workspace_bytes = out.data_ptr(), ws.data_ptr(), ws_bytes
    a.stream = L.stream_handle(wide)
    lib.check(lib.dll.segm_skinny_tn(a), "skinny_tn")
    return out


def channel_sum_supported(x: torch.Tensor) -> bool:
    """(B, C, *spatial) whose voxels are one unit-stride run per (b, c) row (dense or padded channel stride)"""
    if x.dim() < 3 or x.dtype not in (torch.float32, torch.float16, torch.bfloat16) or x.numel() == 0:
        return False
    if x.shape[0] > 65535 or x.shape[1] > 65535:
        return False
    run = 1
    for size, stride in zip(reversed(x.shape[2:]), reversed(x.stride()[2:])):
        if size != 1 and stride != run:
            return False
        run *= size
    return x.stride(1) >= run or x.shape[1] == 1


def channel_sum(lib: L.SegmLib, x: torch.Tensor) -> torch.Tensor:
    """sum over the batch and the voxels of x (B, C, *spatial) -> (C,) fp32: a convolution's bias gradient"""
    if not channel_sum_supported(x):
        raise RuntimeError("channel_sum: (B, C, *spatial) with unit-stride voxels per (b, c) row, fp32 / fp16 / bf16")
    Bn, Cn = x.shape[0], x.shape[1]
    S = 1
    for n in x.shape[2:]:
        S *= n
    out = torch.empty(Cn, dtype=torch.float32, device=x.device)
    ws_bytes = lib.dll.segm_channel_sum_workspace_bytes(Bn, Cn, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    a = L.ChannelSumArgs()
    a.x, a.stride_batch, a.stride_channel, a.spatial = x.data_ptr(), x.stride(0), (x.stride(1) if Cn > 1 else S), S
    a.batch, a.channels, a.dtype = Bn, Cn, L.dtype_code(x)
    a.out, a.workspace, a.workspace_bytes = out.data_ptr(), ws.data_ptr(), ws_bytes
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_channel_sum(a), "channel_sum")
    return out


def pointwise_cf_supported(x3: torch.Tensor, cout: int) -> bool:
    """x3 (B, Cin <= 96, S) 16-bit with contiguous voxels, S % 64 == 0, 16-byte aligned channel rows; Cout <= 96"""
    return bool(x3.dim() == 3 and x3.dtype in (torch.bfloat16, torch.float16) and x3.shape[1] <= 96 and cout <= 96
                and x3.shape[2] % 64 == 0 and x3.stride(2) == 1 and x3.stride(0) % 8 == 0 and x3.stride(1) % 8 == 0
                and x3.data_ptr() % 16 == 0)


def pointwise_cf(lib: L.SegmLib, x3: torch.Tensor, w2: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """y (B, Cout, S) = w2 (Cout, Cin) @ x3[b] (Cin, S) + bias, channel-first in and out (a 1x1x1 convolution on NCDHW
    activations flattened over their voxels, or on channel slices of them).  `out` + `accumulate`: y += ... ."""
    B, Cin, S = x3.shape
    Cout = w2.shape[0]
    if not pointwise_cf_supported(x3, Cout) or w2.shape[1] != Cin or w2.dtype != x3.dtype:
        raise RuntimeError("pointwise_cf: x (B, Cin <= 96, S % 64 == 0) 16-bit with contiguous 16-byte aligned voxel rows, "
                           "w (Cout <= 96, Cin) of the same dtype")
    if Cin % 8:                                            # pad the weight rows to a multiple of 8 (zero columns)
        w2 = torch.nn.functional.pad(w2, (0, 8 - Cin % 8))
    w2 = w2.contiguous()
    y = volume_empty(B, Cout, (S,), x3.dtype, x3.device) if out is None else out
    if tuple(y.shape) != (B, Cout, S) or y.dtype != x3.dtype or y.stride(2) != 1 or y.stride(0) % 4 or y.stride(1) % 4 \
            or y.data_ptr() % 8:
        raise RuntimeError("pointwise_cf: `out` must be (B, Cout, S) of x's dtype with contiguous 8-byte aligned voxel rows")
    if accumulate and out is None:
        raise RuntimeError("pointwise_cf: accumulate needs `out`")
    if bias is not None:
        bias = bias.float().contiguous()
    a = L.PointwiseArgs()
    a.batch, a.cin, a.cout, a.dtype, a.accumulate, a.spatial = B, Cin, Cout, L.dtype_code(x3), int(bool(accumulate)), S
    a.x, a.x_stride_b, a.x_stride_c = x3.data_ptr(), x3.stride(0), x3.stride(1)
    a.w, a.w_stride, a.bias = w2.data_ptr(), w2.shape[1], L.fptr(bias)
    a.y, a.y_stride_b, a.y_stride_c = y.data_ptr(), y.stride(0), y.stride(1)
    a.stream = L.stream_handle(x3)
    lib.check(lib.dll.segm_pointwise_cf(a), "pointwise_cf")
    return y


def _stem_geometry(weight: torch.Tensor):
    """(kernel size, stride) the thin-input kernels run a weight of this shape with: 7^3 -> stride 2 (the stem), 3^3 -> stride 1"""
    k = tuple(weight.shape[2:])
    return (7, 2) if k == (7, 7, 7) else ((3, 1) if k == (3, 3, 3) else (0, 0))


def stem_conv_supported(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """x (B, Cin <= 4, D, H, W); weight (Cout <= 48, Cin, 7, 7, 7) (stride 2, padding 3: D, H even, W % 32 == 0) or
    (Cout <= 48, Cin, 3, 3, 3) (stride 1, padding 1: W % 16 == 0); a wave's 8 output tiles are TX along x (the largest of 8, 4, 2, 1
    dividing Wout / 16) times 8 / TX rows, which must divide Hout"""
    if not (x.dim() == 5 and weight.dim() == 5 and weight.shape[1] == x.shape[1] and x.shape[1] <= 4 and weight.shape[0] <= 48):
        return False
    k, s = _stem_geometry(weight)
    if not k or x.shape[2] % s or x.shape[3] % s or x.shape[4] % (16 * s):
        return False
    xt, hout = x.shape[4] // (16 * s), x.shape[3] // s
    return any(xt % tx == 0 and hout % (8 // tx) == 0 for tx in (8, 4, 2, 1))


def pack_stem_weight(weight: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """(Cout, Cin <= 4, k, k, k) -> (Cout, k, k, 8, 4): [co][kz][ky][kx slot][ci], slots >= k and missing channels zero"""
    w = weight.permute(0, 2, 3, 4, 1)                                  # co, kz, ky, kx, ci
    w = torch.nn.functional.pad(w, (0, 4 - w.shape[-1], 0, 8 - w.shape[-2]))
    return w.contiguous().to(dtype)


def stem_channel_last4(x: torch.Tensor) -> torch.Tensor:
    """(B, Cin <= 4, D, H, W) -> (B, D, H, W, 4) contiguous, missing channels zero: the input layout of the thin-input kernels"""
    return torch.nn.functional.pad(x.permute(0, 2, 3, 4, 1), (0, 4 - x.shape[1])).contiguous()


def stem_conv_fwd(lib: L.SegmLib, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                  x4: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = conv3d(x, weight, bias, stride 2, padding 3) for the 7^3 stem, conv3d(x, weight, bias, stride 1, padding 1) for a 3^3
    weight (x, weight of one 16-bit dtype, at most 4 input channels) -> (B, Cout, D / s, H / s, W / s)"""
    if not stem_conv_supported(x, weight) or x.dtype not in (torch.bfloat16, torch.float16) or weight.dtype != x.dtype:
        raise RuntimeError("stem_conv_fwd: x (B, Cin <= 4, D, H, W) and weight (Cout <= 48, Cin, 7, 7, 7) [stride 2: D, H even, W % 32 == 0] "
                           "or (Cout <= 48, Cin, 3, 3, 3) [stride 1: W % 16 == 0] of one 16-bit dtype")
    B, Cin, D, H, W = x.shape
    k, s = _stem_geometry(weight)
    if x4 is None:
        x4 = stem_channel_last4(x)
    wp = pack_stem_weight(weight, x.dtype)
    y = volume_empty(B, weight.shape[0], (D // s, H // s, W // s), x.dtype, x.device)
    if bias is not None:
        bias = bias.float().contiguous()
    a = L.StemArgs()
    a.batch, a.cout, a.din, a.hin, a.win, a.dtype = B, weight.shape[0], D, H, W, L.dtype_code(x)
    a.x4, a.w_packed, a.bias, a.y = x4.data_ptr(), wp.data_ptr(), L.fptr(bias), y.data_ptr()
    a.kernel_size, a.stride, a.y_channel_stride = k, s, y.stride(1)
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_stem_conv_fwd(a), "stem_conv_fwd")
    return y


def stem_wgrad_supported(x4: torch.Tensor, cout: int, kernel_size: int = 7) -> bool:
    """x4 (B, D, H, W, 4); kernel 7 (stride 2): D, H even and W in {64, 128, 256}; kernel 3 (stride 1): W in {32, 64, 128}; cout <= 48"""
    if not (x4.dim() == 5 and x4.shape[4] == 4 and cout <= 48):
        return False
    if kernel_size == 7:
        return x4.shape[1] % 2 == 0 and x4.shape[2] % 2 == 0 and x4.shape[3] in (64, 128, 256)
    return kernel_size == 3 and x4.shape[3] in (32, 64, 128)


def stem_conv_wgrad(lib: L.SegmLib, x4: torch.Tensor, dy: torch.Tensor, cin: int, kernel_size: int = 7) -> torch.Tensor:
    """dW (Cout, cin, k, k, k) fp32 of conv3d(x, W, stride 2, padding 3) [k = 7] or conv3d(x, W, stride 1, padding 1) [k = 3] from the
    channel-last-4 input x4 (B, D, H, W, 4) and dy (B, Cout, D / s, H / s, W / s) (dense channels), one 16-bit dtype"""
    B, D, H, W, _ = x4.shape
    cout = dy.shape[1]
    s = 2 if kernel_size == 7 else 1
    if (not stem_wgrad_supported(x4, cout, kernel_size) or x4.dtype not in (torch.bfloat16, torch.float16) or dy.dtype != x4.dtype
            or tuple(dy.shape) != (B, cout, D // s, H // s, W // s) or not 1 <= cin <= 4):
        raise RuntimeError("stem_conv_wgrad: x4 (B, D, H, W, 4) and dy (B, Cout <= 48, D / s, H / s, W / s) of one 16-bit dtype; "
                           "kernel 7: D, H even, W in {64, 128, 256}; kernel 3: W in {32, 64, 128}")
    x4 = x4.contiguous()
    if not channel_dense(dy) or dy.stride(1) % 8:
        dy = dy.contiguous()
    cout16 = (cout + 15) // 16 * 16
    slots = 8 if kernel_size == 7 else 4
    dwp = torch.empty(kernel_size, kernel_size, cout16, slots, 4, dtype=torch.float32, device=x4.device)
    nbytes = lib.dll.segm_stem_conv_wgrad_workspace_bytes2(B, cout, D, H, kernel_size, s)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x4.device)
    a = L.StemWgradArgs()
    a.batch, a.cout, a.din, a.hin, a.win, a.dtype = B, cout, D, H, W, L.dtype_code(x4)
    a.x4, a.dy, a.dw_packed = x4.data_ptr(), dy.data_ptr(), dwp.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    a.kernel_size, a.stride, a.dy_channel_stride = kernel_size, s, dy.stride(1)
    a.stream = L.stream_handle(x4)
    lib.check(lib.dll.segm_stem_conv_wgrad(a), "stem_conv_wgrad")
    # [kz][ky][co][kx slot][ci] -> (co, ci, kz, ky, kx)
    return dwp[:, :, :cout, :kernel_size, :cin].permute(2, 4, 0, 1, 3).contiguous()


WGEMM_TN, WGEMM_NT = 0, 1


def wgrad_gemm_tn_supported(a: torch.Tensor, b: torch.Tensor) -> bool:
    """a (K, M), b (K, N): 16-bit, same dtype, unit column stride, M, N <= 1024"""
    return bool(a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0] and a.dtype == b.dtype
                and a.dtype in (torch.bfloat16, torch.float16) and a.stride(1) == 1 and b.stride(1) == 1
                and a.shape[1] <= 1024 and b.shape[1] <= 1024 and a.stride(0) >= a.shape[1] and b.stride(0) >= b.shape[1])


def wgrad_gemm_nt_supported(a: torch.Tensor, b: torch.Tensor) -> bool:
    """a (B, M, K), b (B, N, K): 16-bit, same dtype, unit stride along K, K % 32 == 0, M, N <= 96, 16-byte aligned rows"""
    return bool(a.dim() == 3 and b.dim() == 3 and a.shape[0] == b.shape[0] and a.shape[2] == b.shape[2] and a.dtype == b.dtype
                and a.dtype in (torch.bfloat16, torch.float16) and a.stride(2) == 1 and b.stride(2) == 1 and a.shape[2] % 32 == 0
                and a.shape[1] <= 96 and b.shape[1] <= 96 and not any(t.stride(i) % 8 for t in (a, b) for i in (0, 1))
                and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def wgrad_gemm(lib: L.SegmLib, a: torch.Tensor, b: torch.Tensor, layout: int) -> torch.Tensor:
    """fp32 (M, N): a^T b for a (K, M), b (K, N) (WGEMM_TN), or sum_i a[i] b[i]^T for a (B, M, K), b (B, N, K) (WGEMM_NT)"""
    if layout == WGEMM_TN:
        if not wgrad_gemm_tn_supported(a, b):
            raise RuntimeError("wgrad_gemm TN: a (K, M), b (K, N) 16-bit with unit column stride, M, N <= 1024")
        K, M = a.shape
        N, batch = b.shape[1], 1
        strides = (a.stride(0), 0, b.stride(0), 0)
    else:
        if not wgrad_gemm_nt_supported(a, b):
            raise RuntimeError("wgrad_gemm NT: a (B, M, K), b (B, N, K) 16-bit, unit stride along K % 32 == 0, M, N <= 96, 16-byte aligned rows")
        batch, M, K = a.shape
        N = b.shape[1]
        strides = (a.stride(1), a.stride(0), b.stride(1), b.stride(0))
    out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    nbytes = lib.dll.segm_wgrad_gemm_workspace_bytes(layout, M, N, K, batch)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    g = L.WgradGemmArgs()
    g.layout, g.dtype, g.m, g.n, g.k, g.batch = layout, L.dtype_code(a), M, N, K, batch
    g.a, g.a_stride_row, g.a_stride_batch = a.data_ptr(), strides[0], strides[1]
    g.b, g.b_stride_row, g.b_stride_batch = b.data_ptr(), strides[2], strides[3]
    g.out, g.workspace, g.workspace_bytes, g.stream = out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(a)
    lib.check(lib.dll.segm_wgrad_gemm(g), "wgrad_gemm")
    return out


# ---------------------------------------------------------------------------------------------------------
# evaluation (csrc/metrics.hip, csrc/edt_long.hip): region counts and borders, squared distance transform, boxes, border distances
# ---------------------------------------------------------------------------------------------------------
def _label_volume(t: torch.Tensor, what: str, dims=(3,)) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise RuntimeError(f"{what}: a uint8 tensor is required, got {getattr(t, 'dtype', type(t))}")
    if t.dim() not in dims:
        raise RuntimeError(f"{what}: {' or '.join(str(d) for d in dims)} dimensions required, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: must be contiguous")
    if t.numel() == 0 or t.numel() > L.METRICS_MAX_VOXELS * (t.shape[0] if t.dim() == 4 else 1):
        raise RuntimeError(f"{what}: between 1 and {L.METRICS_MAX_VOXELS} voxels per volume, got shape {tuple(t.shape)}")


def seg_regions(lib: L.SegmLib, pred: torch.Tensor, gt: torch.Tensor, table: torch.Tensor):
    """pred, gt (D, H, W) uint8 label volumes; table (256,) uint8, bit r of table[l] = label l belongs to region r.
    -> (borders, counts): borders (2, D, H, W) uint8, the border bits of pred [0] and gt [1] (bit r = region r); counts (5, 8) int64 =
    |P|, |G|, |P and G|, |border P|, |border G| per region (still on the device)."""
    _label_volume(pred, "seg_regions: pred")
    _label_volume(gt, "seg_regions: gt")
    if pred.shape != gt.shape:
        raise RuntimeError(f"seg_regions: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ in shape")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or tuple(table.shape) != (256,) or not table.is_contiguous():
        raise RuntimeError("seg_regions: table must be a contiguous uint8 tensor of 256 entries")
    if gt.device != pred.device or table.device != pred.device:
        raise RuntimeError("seg_regions: pred, gt and table must be on one device")
    D, H, W = pred.shape
    borders = torch.empty(2, D, H, W, dtype=torch.uint8, device=pred.device)
    counts = torch.empty(5, L.METRICS_MAX_REGIONS, dtype=torch.int64, device=pred.device)
    nbytes = lib.dll.segm_seg_regions_workspace_bytes(pred.numel())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=pred.device)
    a = L.SegRegionsArgs()
    a.depth, a.height, a.width = D, H, W
    a.pred, a.gt, a.table, a.border_pred, a.border_gt = pred.data_ptr(), gt.data_ptr(), table.data_ptr(), borders[0].data_ptr(), borders[1].data_ptr()
    a.counts, a.workspace, a.workspace_bytes, a.stream = counts.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(pred)
    lib.check(lib.dll.segm_seg_regions(a), "seg_regions")
    return borders, counts


def _unit_spacing(spacing) -> bool:
    return spacing is None or all(float(s) == 1.0 for s in spacing)


def _spacing3(spacing):
    if spacing is None:
        return (1.0, 1.0, 1.0)
    sp = tuple(float(s) for s in spacing)
    if len(sp) != 3 or not all(0.0 < s < 1e15 for s in sp):
        raise RuntimeError(f"spacing must be three positive numbers (z, y, x), got {spacing}")
    return sp


def _plane_list(planes, n_volumes: int, what: str):
    planes = [(int(v), int(b)) for v, b in planes]
    if not 1 <= len(planes) <= L.METRICS_MAX_PLANES:
        raise RuntimeError(f"{what}: between 1 and {L.METRICS_MAX_PLANES} planes per call, got {len(planes)}")
    for v, b in planes:
        if not (0 <= v < n_volumes and 0 <= b < 8):
            raise RuntimeError(f"{what}: plane (volume {v}, bit {b}) outside {n_volumes} volumes of 8 bits")
    return planes


def edt_sq(lib: L.SegmLib, volumes: torch.Tensor, planes, spacing=None) -> torch.Tensor:
    """Squared Euclidean distance of every voxel to the nearest voxel whose bit is set, for a batch of bit planes.
    volumes (V, D, H, W) uint8; planes: (volume, bit) pairs; spacing (z, y, x) or None.  -> (len(planes), D, H, W), int32 for unit
    spacing (INT32_MAX where a plane has no set bit), fp32 otherwise (+inf)."""
    _label_volume(volumes, "edt_sq: volumes", dims=(4,))
    V, D, H, W = volumes.shape
    if max(D, H, W) > L.EDT_MAX_LINE:
        raise RuntimeError(f"edt_sq: depth, height and width are limited to {L.EDT_MAX_LINE} (SEGM_E_SHAPE), got {(D, H, W)}")
    if V > L.METRICS_MAX_PLANES:
        raise RuntimeError(f"edt_sq: at most {L.METRICS_MAX_PLANES} volumes per call, got {V}")
    planes = _plane_list(planes, V, "edt_sq")
    sp = _spacing3(spacing)
    unit = _unit_spacing(spacing)
    out = torch.empty(len(planes), D, H, W, dtype=torch.int32 if unit else torch.float32, device=volumes.device)
    a = L.EdtSqArgs()
    a.depth, a.height, a.width, a.n_volumes, a.n_planes, a.fp32 = D, H, W, V, len(planes), 0 if unit else 1
    a.spacing_z, a.spacing_y, a.spacing_x = sp
    for i, (v, b) in enumerate(planes):
        a.plane_volume[i], a.plane_bit[i] = v, b
    a.volumes, a.out, a.stream = volumes.data_ptr(), out.data_ptr(), L.stream_handle(volumes)
    lib.check(lib.dll.segm_edt_sq(a), "edt_sq")
    return out


def edt_sq_long(lib: L.SegmLib, volumes: torch.Tensor, planes, spacing=None, max_workgroups: int = 0) -> torch.Tensor:
    """`edt_sq` for sides up to 2048 (segm_edt_sq_long: linear in the line length, stacks in a workspace sized by the grid).  Same
    arguments and result; int32 values equal `edt_sq`'s, fp32 values lie within the same 1e-6 relative bound.  max_workgroups: 0 = the
    default, a smaller positive value lowers the grid of the line passes (a workgroup then reuses its stack area more often)."""
    _label_volume(volumes, "edt_sq_long: volumes", dims=(4,))
    V, D, H, W = volumes.shape
    if max(D, H, W) > L.EDT_LONG_MAX_LINE:
        raise RuntimeError(f"edt_sq_long: depth, height and width are limited to {L.EDT_LONG_MAX_LINE} (SEGM_E_SHAPE), got {(D, H, W)}")
    if V > L.METRICS_MAX_PLANES:
        raise RuntimeError(f"edt_sq_long: at most {L.METRICS_MAX_PLANES} volumes per call, got {V}")
    planes = _plane_list(planes, V, "edt_sq_long")
    max_workgroups = int(max_workgroups)
    if max_workgroups < 0:
        raise RuntimeError(f"edt_sq_long: max_workgroups must be 0 (default) or positive, got {max_workgroups}")
    sp = _spacing3(spacing)
    unit = _unit_spacing(spacing)
    out = torch.empty(len(planes), D, H, W, dtype=torch.int32 if unit else torch.float32, device=volumes.device)
    nbytes = lib.dll.segm_edt_sq_long_workspace_bytes(D, H, W, len(planes), 0 if unit else 1)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=volumes.device)
    a = L.EdtSqLongArgs()
    a.depth, a.height, a.width, a.n_volumes, a.n_planes, a.fp32 = D, H, W, V, len(planes), 0 if unit else 1
    a.spacing_z, a.spacing_y, a.spacing_x = sp
    a.max_workgroups = max_workgroups
    for i, (v, b) in enumerate(planes):
        a.plane_volume[i], a.plane_bit[i] = v, b
    a.volumes, a.out, a.stream = volumes.data_ptr(), out.data_ptr(), L.stream_handle(volumes)
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    lib.check(lib.dll.segm_edt_sq_long(a), "edt_sq_long")
    return out


def planes_bbox(lib: L.SegmLib, volumes: torch.Tensor, items) -> torch.Tensor:
    """Bounding boxes of bit planes in one pass.  volumes (V, D, H, W) uint8; items: (volume, bit) or (volume, bit, volume2, bit2),
    the latter the OR of two planes.  -> (16, 6) int32 on the device, row i = [z0, z1, y0, y1, x0, x1] of item i, half-open;
    z1 = y1 = x1 = 0 for an item without a set voxel (and for the rows past the last item)."""
    _label_volume(volumes, "planes_bbox: volumes", dims=(4,))
    V, D, H, W = volumes.shape
    if V > L.METRICS_MAX_PLANES:
        raise RuntimeError(f"planes_bbox: at most {L.METRICS_MAX_PLANES} volumes per call, got {V}")
    if max(D, H, W) >= 1 << 20:
        raise RuntimeError(f"planes_bbox: sides are limited to 2^20 - 1, got {(D, H, W)}")
    items = [tuple(int(v) for v in it) for it in items]
    if any(len(it) not in (2, 4) for it in items):
        raise RuntimeError("planes_bbox: an item is (volume, bit) or (volume, bit, volume2, bit2)")
    _plane_list([it[:2] for it in items], V, "planes_bbox")
    _plane_list([it[2:] for it in items if len(it) == 4] or [(0, 0)], V, "planes_bbox")
    boxes = torch.empty(L.METRICS_MAX_PLANES, 6, dtype=torch.int32, device=volumes.device)
    a = L.PlanesBboxArgs()
    a.depth, a.height, a.width, a.n_volumes, a.n_items = D, H, W, V, len(items)
    for i, it in enumerate(items):
        a.item_volume[i], a.item_bit[i] = it[:2]
        a.item_volume2[i], a.item_bit2[i] = it[2:] if len(it) == 4 else (-1, 0)
    a.volumes, a.boxes, a.stream = volumes.data_ptr(), boxes.data_ptr(), L.stream_handle(volumes)
    lib.check(lib.dll.segm_planes_bbox(a), "planes_bbox")
    return boxes


def border_distances(lib: L.SegmLib, borders: torch.Tensor, edt: torch.Tensor, items, counts) -> torch.Tensor:
    """borders (V, D, H, W) uint8 bit planes; edt (P, D, H, W) int32 / fp32 squared distances; items: (volume, bit, edt plane)
    triples; counts: the number of set voxels of each item's border (as seg_regions counted them).  -> one fp32 vector: the
    items' distance lists sqrt(edt[plane][v]) over their border voxels v in memory order, one after the other."""
    _label_volume(borders, "border_distances: borders", dims=(4,))
    if not isinstance(edt, torch.Tensor) or edt.dtype not in (torch.int32, torch.float32) or edt.dim() != 4 or not edt.is_contiguous():
        raise RuntimeError("border_distances: edt must be a contiguous (P, D, H, W) int32 or fp32 tensor")
    if edt.shape[1:] != borders.shape[1:] or edt.device != borders.device:
        raise RuntimeError(f"border_distances: borders {tuple(borders.shape)} and edt {tuple(edt.shape)} must share volume shape and device")
    items = [(int(v), int(b), int(p)) for v, b, p in items]
    _plane_list([(v, b) for v, b, _ in items], borders.shape[0], "border_distances")
    counts = [int(c) for c in counts]
    if len(counts) != len(items) or any(c < 0 for c in counts) or any(not 0 <= p < edt.shape[0] for _, _, p in items):
        raise RuntimeError("border_distances: one non-negative count per item and edt planes inside `edt` are required")
    N = borders[0].numel()
    total = sum(counts)
    out = torch.empty(total, dtype=torch.float32, device=borders.device)
    if total == 0:
        return out
    nbytes = lib.dll.segm_border_distances_workspace_bytes(N, len(items))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=borders.device)
    a = L.BorderDistancesArgs()
    a.voxels, a.n_volumes, a.n_planes, a.n_items, a.fp32 = N, borders.shape[0], edt.shape[0], len(items), int(edt.dtype == torch.float32)
    off = 0
    for i, ((v, b, p), c) in enumerate(zip(items, counts)):
        a.border_volume[i], a.border_bit[i], a.edt_plane[i], a.out_offset[i], a.out_count[i] = v, b, p, off, c
        off += c
    a.out_capacity = total
    a.borders, a.edt, a.out = borders.data_ptr(), edt.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, L.stream_handle(borders)
    lib.check(lib.dll.segm_border_distances(a), "border_distances")
    return out


def border_stats(lib: L.SegmLib, borders: torch.Tensor, edt: torch.Tensor, items, groups, n_groups: int, tolerances=None,
                 ranks=None) -> torch.Tensor:
    """What the surface metrics need of `border_distances`' lists, without the lists (segm_border_stats).  borders, edt and items
    as in `border_distances`; groups: the group of each item (the items of a group form one joined list); tolerances: one per item
    (None or a negative value: count nothing); ranks: per group two 0-based ranks in the ascending joined list (a negative one: none).
    -> (96,) fp64 on the device: [4 i ..] = count, sum, max and within-tolerance count of item i; [64 + 2 g ..] = the two order
    statistics of group g, NaN for a rank outside the list."""
    _label_volume(borders, "border_stats: borders", dims=(4,))
    if not isinstance(edt, torch.Tensor) or edt.dtype not in (torch.int32, torch.float32) or edt.dim() != 4 or not edt.is_contiguous():
        raise RuntimeError("border_stats: edt must be a contiguous (P, D, H, W) int32 or fp32 tensor")
    if edt.shape[1:] != borders.shape[1:] or edt.device != borders.device:
        raise RuntimeError(f"border_stats: borders {tuple(borders.shape)} and edt {tuple(edt.shape)} must share volume shape and device")
    items = [(int(v), int(b), int(p)) for v, b, p in items]
    _plane_list([(v, b) for v, b, _ in items], borders.shape[0], "border_stats")
    groups = [int(g) for g in groups]
    n_groups = int(n_groups)
    if not 1 <= n_groups <= L.METRICS_MAX_PLANES:
        raise RuntimeError(f"border_stats: between 1 and {L.METRICS_MAX_PLANES} groups per call, got {n_groups}")
    if len(groups) != len(items) or any(not 0 <= g < n_groups for g in groups) or any(not 0 <= p < edt.shape[0] for _, _, p in items):
        raise RuntimeError("border_stats: one group in [0, n_groups) per item and edt planes inside `edt` are required")
    tolerances = [-1.0] * len(items) if tolerances is None else [-1.0 if t is None else float(t) for t in tolerances]
    ranks = [(-1, -1)] * n_groups if ranks is None else [(int(a), int(b)) for a, b in ranks]
    if len(tolerances) != len(items) or len(ranks) != n_groups:
        raise RuntimeError("border_stats: one tolerance per item and one pair of ranks per group are required")
    N = borders[0].numel()
    if max(groups.count(g) for g in range(n_groups)) * N >= 1 << 32:
        raise RuntimeError("border_stats: a group's items times the voxels must stay below 2^32")
    out = torch.empty(6 * L.METRICS_MAX_PLANES, dtype=torch.float64, device=borders.device)
    nbytes = lib.dll.segm_border_stats_workspace_bytes(N, len(items))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=borders.device)
    a = L.BorderStatsArgs()
    a.voxels, a.n_volumes, a.n_planes, a.n_items, a.n_groups = N, borders.shape[0], edt.shape[0], len(items), n_groups
    a.fp32 = int(edt.dtype == torch.float32)
    for i, ((v, b, p), g, t) in enumerate(zip(items, groups, tolerances)):
        a.border_volume[i], a.border_bit[i], a.edt_plane[i], a.item_group[i], a.tolerance[i] = v, b, p, g, t
    for g, (lo, hi) in enumerate(ranks):
        a.rank[g][0], a.rank[g][1] = lo, hi
    a.borders, a.edt, a.out = borders.data_ptr(), edt.data_ptr(), out.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), ws.numel() * 8, L.stream_handle(borders)
    lib.check(lib.dll.segm_border_stats(a), "border_stats")
    return out


# ---------------------------------------------------------------------------------------------------------
# signed-distance and edge targets (csrc/sdm.hip): region bits with edges and inner boundaries, then sdf / sdm / edge planes
# ---------------------------------------------------------------------------------------------------------
_SDM_LABEL_DTYPES = {torch.uint8: L.SDM_LABEL_U8, torch.int16: L.SDM_LABEL_I16, torch.int64: L.SDM_LABEL_I64}


def sdm_masks(lib: L.SegmLib, labels: torch.Tensor, table: torch.Tensor, n_regions: int):
    """labels (n, D, H, W) uint8, int16 or int64, contiguous (a value outside 0 .. 255 is in no region); table (256,) uint8, bit r of
    table[l] = label l belongs to region r < n_regions.  -> (bits, counts): bits (4, n, D, H, W) uint8 = the inside, outside, edge
    and boundary bits of every volume (bit r = region r); counts (n, 8) int64 = the region sizes (still on the device)."""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in _SDM_LABEL_DTYPES:
        raise RuntimeError(f"sdm_masks: labels must be a uint8, int16 or int64 tensor, got {getattr(labels, 'dtype', type(labels))}")
    if labels.dim() != 4 or not labels.is_contiguous():
        raise RuntimeError(f"sdm_masks: labels must be contiguous (n, D, H, W), got shape {tuple(labels.shape)}")
    n, D, H, W = labels.shape
    if not 1 <= n <= L.METRICS_MAX_PLANES:
        raise RuntimeError(f"sdm_masks: between 1 and {L.METRICS_MAX_PLANES} volumes per call, got {n}")
    if min(D, H, W) < 1 or max(D, H, W) > L.EDT_LONG_MAX_LINE or D * H * W > L.METRICS_MAX_VOXELS:
        raise RuntimeError(f"sdm_masks: sides in [1, {L.EDT_LONG_MAX_LINE}] and at most {L.METRICS_MAX_VOXELS} voxels per volume, got {(D, H, W)}")
    n_regions = int(n_regions)
    if not 1 <= n_regions <= L.METRICS_MAX_REGIONS:
        raise RuntimeError(f"sdm_masks: between 1 and {L.METRICS_MAX_REGIONS} regions per call, got {n_regions}")
    if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or tuple(table.shape) != (256,) or not table.is_contiguous():
        raise RuntimeError("sdm_masks: table must be a contiguous uint8 tensor of 256 entries")
    if table.device != labels.device:
        raise RuntimeError("sdm_masks: labels and table must be on one device")
    bits = torch.empty(4, n, D, H, W, dtype=torch.uint8, device=labels.device)
    counts = torch.empty(n, L.METRICS_MAX_REGIONS, dtype=torch.int64, device=labels.device)
    a = L.SdmMasksArgs()
    a.depth, a.height, a.width, a.n, a.n_regions, a.label_dtype = D, H, W, n, n_regions, _SDM_LABEL_DTYPES[labels.dtype]
    a.labels, a.table = labels.data_ptr(), table.data_ptr()
    a.inside, a.outside, a.edge, a.boundary = (bits[k].data_ptr() for k in range(4))
    a.counts, a.stream = counts.data_ptr(), L.stream_handle(labels)
    lib.check(lib.dll.segm_sdm_masks(a), "sdm_masks")
    return bits, counts


def sdm_compose(lib: L.SegmLib, bits: torch.Tensor, counts: torch.Tensor, edt: Optional[torch.Tensor], items, sdf: torch.Tensor = None,
                sdm: torch.Tensor = None, edge: torch.Tensor = None) -> None:
    """bits, counts as `sdm_masks` returns them; edt (P, D, H, W) int32 squared distances at unit spacing (None when only `edge` is
    asked for); items: (volume, bit, pos plane, neg plane, output plane) - pos plane = the transform seeded by that bit of
    bits[1] (outside), neg plane = by that bit of bits[0] (inside).  Writes plane `output plane` of the given outputs, each
    (Q, D, H, W) fp32 contiguous: sdf, sdm = 1 - sdf + edge, edge as 0.0 / 1.0."""
    if not isinstance(bits, torch.Tensor) or bits.dtype != torch.uint8 or bits.dim() != 5 or bits.shape[0] != 4 or not bits.is_contiguous():
        raise RuntimeError("sdm_compose: bits must be the contiguous (4, n, D, H, W) uint8 tensor of sdm_masks")
    n, shape = bits.shape[1], tuple(bits.shape[2:])
    N = bits[0, 0].numel()
    if N == 0 or N > L.METRICS_MAX_VOXELS:
        raise RuntimeError(f"sdm_compose: between 1 and {L.METRICS_MAX_VOXELS} voxels per volume, got shape {shape}")
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int64 or tuple(counts.shape) != (n, L.METRICS_MAX_REGIONS) \
            or not counts.is_contiguous() or counts.device != bits.device:
        raise RuntimeError(f"sdm_compose: counts must be the contiguous ({n}, {L.METRICS_MAX_REGIONS}) int64 tensor of sdm_masks")
    outs = [t for t in (sdf, sdm, edge) if t is not None]
    if not outs:
        raise RuntimeError("sdm_compose: at least one of sdf, sdm and edge is required")
    for t in outs:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4 or tuple(t.shape[1:]) != shape or not t.is_contiguous() \
                or t.device != bits.device or t.shape[0] != outs[0].shape[0]:
            raise RuntimeError(f"sdm_compose: outputs must be contiguous fp32 (Q, {', '.join(str(s) for s in shape)}) tensors of one Q on the bits' device")
    dist = sdf is not None or sdm is not None
    if dist:
        if not isinstance(edt, torch.Tensor) or edt.dtype != torch.int32 or edt.dim() != 4 or tuple(edt.shape[1:]) != shape \
                or not edt.is_contiguous() or edt.device != bits.device:
            raise RuntimeError("sdm_compose: edt must be a contiguous (P, D, H, W) int32 tensor of the bits' volume shape and device")
    items = [tuple(int(v) for v in it) for it in items]
    if not 1 <= len(items) <= L.METRICS_MAX_PLANES or any(len(it) != 5 for it in items):
        raise RuntimeError(f"sdm_compose: between 1 and {L.METRICS_MAX_PLANES} items (volume, bit, pos plane, neg plane, output plane)")
    n_planes = edt.shape[0] if dist else 0
    for v, b, pp, npl, o in items:
        if not (0 <= v < n and 0 <= b < L.METRICS_MAX_REGIONS and 0 <= o < outs[0].shape[0]):
            raise RuntimeError(f"sdm_compose: item (volume {v}, bit {b}, output plane {o}) out of range")
        if dist and not (0 <= pp < n_planes and 0 <= npl < n_planes):
            raise RuntimeError(f"sdm_compose: planes ({pp}, {npl}) outside the {n_planes} planes of edt")
    if len({it[4] for it in items}) != len(items):
        raise RuntimeError("sdm_compose: two items write one output plane")
    ws = torch.empty(L.SDM_COMPOSE_WORKSPACE_BYTES // 4, dtype=torch.int32, device=bits.device) if dist else None     # the maxima
    a = L.SdmComposeArgs()
    a.voxels, a.n_items, a.n_volumes, a.n_planes, a.n_out_planes = N, len(items), n, n_planes, outs[0].shape[0]
    for i, (v, b, pp, npl, o) in enumerate(items):
        a.volume[i], a.bit[i], a.pos_plane[i], a.neg_plane[i], a.out_plane[i] = v, b, pp, npl, o
    a.edt = edt.data_ptr() if dist else None
    a.inside, a.edge, a.boundary, a.counts = bits[0].data_ptr(), bits[2].data_ptr(), bits[3].data_ptr(), counts.data_ptr()
    a.sdf, a.sdm, a.edge_out = L.fptr(sdf), L.fptr(sdm), L.fptr(edge)
    a.workspace, a.workspace_bytes, a.stream = L.fptr(ws), L.SDM_COMPOSE_WORKSPACE_BYTES if dist else 0, L.stream_handle(bits)
    lib.check(lib.dll.segm_sdm_compose(a), "sdm_compose")


# ---------------------------------------------------------------------------------------------------------
# finishing a prediction (csrc/postprocess.hip, csrc/ccl_roots.hip): logits -> labels, connected components, sizes, selection
# ---------------------------------------------------------------------------------------------------------
def _same_volume(t, what: str, dtype, shape, device) -> None:
    """a caller's buffer: dtype, shape, device and contiguity before its pointer leaves Python"""
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise RuntimeError(f"{what}: a {dtype} tensor is required, got {getattr(t, 'dtype', type(t))}")
    if tuple(t.shape) != tuple(shape) or t.device != device or not t.is_contiguous():
        raise RuntimeError(f"{what}: must be contiguous, of shape {tuple(shape)} and on {device}; got {tuple(t.shape)} on {t.device}")


def _ccl_volume(t: torch.Tensor, what: str, dtype=torch.uint8) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != dtype:
        raise RuntimeError(f"{what}: a {dtype} tensor is required, got {getattr(t, 'dtype', type(t))}")
    if t.dim() != 3:
        raise RuntimeError(f"{what}: a (D, H, W) volume is required, got shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: must be contiguous")
    if t.numel() == 0 or t.numel() > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"{what}: between 1 and 2^31 - 1 voxels, got shape {tuple(t.shape)}")


def resample_argmax(lib: L.SegmLib, logits: torch.Tensor, out_shape=None, box_start=(0, 0, 0), box_shape=None, table=None,
                    out: torch.Tensor = None, max_classes: int = L.RESAMPLE_MAX_CLASSES):
    """logits (C, d, h, w) fp32 / bf16 / fp16 with a unit stride along w, C <= `max_classes` (8 unless the caller raises it, at most
    L.RESAMPLE_CLASS_LIMIT).  -> uint8 labels of shape `out_shape`: inside the box
    `box_start` + `box_shape` the arg-max over the classes of the logits resampled (trilinear, align_corners False) to the box's
    shape, 0 outside.  Defaults: the box has the logits' shape and fills the output.  With `table` (256 uint8, device) also the
    region bit planes table[label]: -> (labels, regions)."""
    if not isinstance(logits, torch.Tensor) or logits.dim() != 4:
        raise RuntimeError(f"resample_argmax: logits (C, d, h, w) required, got {getattr(logits, 'shape', type(logits))}")
    dtype = L.dtype_code(logits)
    C_, d, h, w = logits.shape
    max_classes = int(max_classes)
    if not 1 <= max_classes <= L.RESAMPLE_CLASS_LIMIT:
        raise RuntimeError(f"resample_argmax: max_classes must lie in 1 .. {L.RESAMPLE_CLASS_LIMIT}, got {max_classes}")
    if not 1 <= C_ <= max_classes or min(d, h, w) < 1:
        raise RuntimeError(f"resample_argmax: 1 .. {max_classes} classes and a non-empty volume, got {tuple(logits.shape)}")
    sc, sz, sy, sx = logits.stride()
    if w > 1 and sx != 1:
        raise RuntimeError("resample_argmax: logits need a unit stride along the last dimension")
    if (h > 1 and sy < w) or min(sc, sz) < 0:
        raise RuntimeError(f"resample_argmax: unsupported logits strides {logits.stride()}")
    box_shape = (d, h, w) if box_shape is None else tuple(int(v) for v in box_shape)
    box_start = tuple(int(v) for v in box_start)
    out_shape = tuple(b0 + bs for b0, bs in zip(box_start, box_shape)) if out_shape is None else tuple(int(v) for v in out_shape)
    if len(box_shape) != 3 or len(box_start) != 3 or len(out_shape) != 3:
        raise RuntimeError("resample_argmax: out_shape, box_start and box_shape have three entries each")
    if any(bs < 1 or b0 < 0 or b0 + bs > o for b0, bs, o in zip(box_start, box_shape, out_shape)):
        raise RuntimeError(f"resample_argmax: the box {box_start} + {box_shape} does not lie inside the output {out_shape}")
    n = out_shape[0] * out_shape[1] * out_shape[2]
    if n > L.CCL_MAX_VOXELS or max(d, h, w, *out_shape) > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"resample_argmax: at most 2^31 - 1 output voxels, got {out_shape}")
    if out is None:
        out = torch.empty(out_shape, dtype=torch.uint8, device=logits.device)
    else:
        _same_volume(out, "resample_argmax: out", torch.uint8, out_shape, logits.device)
    regions = None
    if table is not None:
        if not isinstance(table, torch.Tensor) or table.dtype != torch.uint8 or tuple(table.shape) != (256,) or not table.is_contiguous() \
                or table.device != logits.device:
            raise RuntimeError("resample_argmax: table must be a contiguous uint8 tensor of 256 entries on the logits' device")
        regions = torch.empty(out_shape, dtype=torch.uint8, device=logits.device)
    a = L.ResampleArgmaxArgs()
    a.classes, a.dtype = C_, dtype
    a.in_depth, a.in_height, a.in_width = d, h, w
    a.box_z, a.box_y, a.box_x = box_start
    a.box_depth, a.box_height, a.box_width = box_shape
    a.out_depth, a.out_height, a.out_width = out_shape
    a.stride_c, a.stride_z, a.stride_y = sc, sz, max(sy, w)
    a.logits, a.labels, a.stream = logits.data_ptr(), out.data_ptr(), L.stream_handle(logits)
    if regions is not None:
        a.regions, a.table = regions.data_ptr(), table.data_ptr()
    lib.check(lib.dll.segm_resample_argmax(a), "resample_argmax")
    return out if regions is None else (out, regions)


def _connectivity(connectivity, what: str) -> int:
    """1, 2 or 3 as in scipy.ndimage.generate_binary_structure(3, c): 6, 18 or 26 neighbours"""
    if isinstance(connectivity, bool) or connectivity not in (1, 2, 3):
        raise ValueError(f"{what}: connectivity must be 1, 2 or 3, got {connectivity!r}")
    return int(connectivity)


def ccl_roots(lib: L.SegmLib, volume: torch.Tensor, bit: int = -1, invert: bool = False, out: torch.Tensor = None,
              connectivity: int = 1) -> torch.Tensor:
    """Connected components of the mask `(volume >> bit) & 1` (bit = -1: `volume != 0`), or of its complement with `invert`, at
    `connectivity` 1, 2 or 3 (6, 18 or 26 neighbours).  volume (D, H, W) uint8.
    -> int32 (D, H, W): -1 outside the mask, else the smallest linear index of the voxel's component."""
    connectivity = _connectivity(connectivity, "ccl_roots")
    _ccl_volume(volume, "ccl_roots: volume")
    bit = int(bit)
    if not -1 <= bit <= 7:
        raise RuntimeError(f"ccl_roots: bit must be -1 or 0 .. 7, got {bit}")
    if out is None:
        out = torch.empty(volume.shape, dtype=torch.int32, device=volume.device)
    else:
        _same_volume(out, "ccl_roots: out", torch.int32, volume.shape, volume.device)
    nbytes = lib.dll.segm_ccl_roots_workspace_bytes(volume.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=volume.device)
    a = L.CclRootsConnArgs()
    a.depth, a.height, a.width = volume.shape
    a.bit, a.invert, a.connectivity = bit, 1 if invert else 0, connectivity
    a.volume, a.roots, a.workspace, a.workspace_bytes, a.stream = volume.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(volume)
    lib.check(lib.dll.segm_ccl_roots_conn(a), "ccl_roots")
    return out


def ccl_sizes(lib: L.SegmLib, roots: torch.Tensor):
    """roots as `ccl_roots` gives them.  -> (sizes int32 (D, H, W): the component's voxel count at its root voxel, 0 elsewhere;
    touches uint8 (D, H, W): 1 at the roots whose component has a voxel on a face of the volume)."""
    _ccl_volume(roots, "ccl_sizes: roots", torch.int32)
    sizes = torch.empty(roots.shape, dtype=torch.int32, device=roots.device)
    touches = torch.empty(roots.shape, dtype=torch.uint8, device=roots.device)
    a = L.CclSizesArgs()
    a.depth, a.height, a.width = roots.shape
    a.roots, a.sizes, a.touches, a.stream = roots.data_ptr(), sizes.data_ptr(), touches.data_ptr(), L.stream_handle(roots)
    lib.check(lib.dll.segm_ccl_sizes(a), "ccl_sizes")
    return sizes, touches


def ccl_select(lib: L.SegmLib, roots: torch.Tensor, sizes: torch.Tensor, mode: int, min_size: int = 0, touches: torch.Tensor = None,
               out: torch.Tensor = None):
    """-> (mask uint8 (D, H, W), info int64 (3,) on the device = [components, root of the largest or -1, its voxel count]).
    mode L.CCL_LARGEST: the largest component (equal counts: the root that comes last); L.CCL_MIN_SIZE: every component of at least
    `min_size` voxels; L.CCL_FILL (roots / sizes / touches of the INVERTED mask): the mask with its holes filled."""
    _ccl_volume(roots, "ccl_select: roots", torch.int32)
    _same_volume(sizes, "ccl_select: sizes", torch.int32, roots.shape, roots.device)
    if mode not in (L.CCL_LARGEST, L.CCL_MIN_SIZE, L.CCL_FILL):
        raise RuntimeError(f"ccl_select: unknown mode {mode}")
    if mode == L.CCL_FILL or touches is not None:
        _same_volume(touches, "ccl_select: touches", torch.uint8, roots.shape, roots.device)
    min_size = int(min_size)
    if not 0 <= min_size <= L.CCL_MAX_VOXELS:
        raise RuntimeError(f"ccl_select: min_size must lie in [0, 2^31 - 1], got {min_size}")
    if out is None:
        out = torch.empty(roots.shape, dtype=torch.uint8, device=roots.device)
    else:
        _same_volume(out, "ccl_select: out", torch.uint8, roots.shape, roots.device)
    info = torch.empty(3, dtype=torch.int64, device=roots.device)
    nbytes = lib.dll.segm_ccl_select_workspace_bytes(roots.numel())
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=roots.device)
    a = L.CclSelectArgs()
    a.depth, a.height, a.width = roots.shape
    a.mode, a.min_size = mode, min_size
    a.roots, a.sizes, a.out, a.info = roots.data_ptr(), sizes.data_ptr(), out.data_ptr(), info.data_ptr()
    a.touches = None if touches is None else touches.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, L.stream_handle(roots)
    lib.check(lib.dll.segm_ccl_select(a), "ccl_select")
    return out, info


def ccl_label_roots(lib: L.SegmLib, labels: torch.Tensor, out: torch.Tensor = None, connectivity: int = 1) -> torch.Tensor:
    """Connected components of every class of a label volume in one pass: two voxels are joined by a path of neighbours of the same
    non-zero label, at `connectivity` 1, 2 or 3 (6, 18 or 26 neighbours).  labels (D, H, W) uint8.  -> int32 (D, H, W): -1 where the
    label is 0, else the smallest linear index of the voxel's component (on `labels == k` what `ccl_roots(labels == k)` gives at the
    same connectivity)."""
    connectivity = _connectivity(connectivity, "ccl_label_roots")
    _ccl_volume(labels, "ccl_label_roots: labels")
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.int32, device=labels.device)
    else:
        _same_volume(out, "ccl_label_roots: out", torch.int32, labels.shape, labels.device)
    nbytes = lib.dll.segm_ccl_label_roots_workspace_bytes(labels.numel())
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=labels.device)
    a = L.CclLabelRootsConnArgs()
    a.depth, a.height, a.width, a.connectivity = *labels.shape, connectivity
    a.labels, a.roots, a.workspace, a.workspace_bytes, a.stream = labels.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(labels)
    lib.check(lib.dll.segm_ccl_label_roots_conn(a), "ccl_label_roots")
    return out


def ccl_label_select(lib: L.SegmLib, labels: torch.Tensor, roots: torch.Tensor, sizes: torch.Tensor, mode: int, min_size: int = 0,
                     apply: torch.Tensor = None, out: torch.Tensor = None):
    """-> (labels uint8 (D, H, W), info int64 (256, 3) on the device = per label [components, root of the largest or -1, its voxel
    count]).  mode L.CCL_LARGEST: a voxel keeps its label iff its component is the largest of its label (equal counts: the root that
    comes last); L.CCL_MIN_SIZE: iff its component has at least `min_size` voxels.  `apply` (256 uint8 on the device): labels whose
    entry is 0 pass through untouched; None selects on every label."""
    _ccl_volume(labels, "ccl_label_select: labels")
    _same_volume(roots, "ccl_label_select: roots", torch.int32, labels.shape, labels.device)
    _same_volume(sizes, "ccl_label_select: sizes", torch.int32, labels.shape, labels.device)
    if mode not in (L.CCL_LARGEST, L.CCL_MIN_SIZE):
        raise RuntimeError(f"ccl_label_select: mode must be CCL_LARGEST or CCL_MIN_SIZE, got {mode}")
    min_size = int(min_size)
    if not 0 <= min_size <= L.CCL_MAX_VOXELS:
        raise RuntimeError(f"ccl_label_select: min_size must lie in [0, 2^31 - 1], got {min_size}")
    if apply is not None:
        _same_volume(apply, "ccl_label_select: apply", torch.uint8, (256,), labels.device)
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    else:
        _same_volume(out, "ccl_label_select: out", torch.uint8, labels.shape, labels.device)
    info = torch.empty((256, 3), dtype=torch.int64, device=labels.device)
    nbytes = lib.dll.segm_ccl_label_select_workspace_bytes(labels.numel())
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=labels.device)
    a = L.CclLabelSelectArgs()
    a.depth, a.height, a.width = labels.shape
    a.mode, a.min_size = mode, min_size
    a.labels, a.roots, a.sizes, a.out, a.info = labels.data_ptr(), roots.data_ptr(), sizes.data_ptr(), out.data_ptr(), info.data_ptr()
    a.apply = None if apply is None else apply.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), nbytes, L.stream_handle(labels)
    lib.check(lib.dll.segm_ccl_label_select(a), "ccl_label_select")
    return out, info


# ---------------------------------------------------------------------------------------------------------
# preparing a case (csrc/preprocess.hip): non-zero mask and box, crop statistics, crop + z-score + seg relabelling
# ---------------------------------------------------------------------------------------------------------
_SEG_DTYPES = {torch.float32: L.PREP_SEG_F32, torch.uint8: L.PREP_SEG_U8, torch.int16: L.PREP_SEG_I16}


def _prep_data(data, what: str):
    """(C, D, H, W) fp32 with a unit stride along x, C <= 8: -> (C, D, H, W, stride_c, stride_z, stride_y)"""
    if not isinstance(data, torch.Tensor) or data.dim() != 4:
        raise RuntimeError(f"{what}: data (C, D, H, W) required, got {getattr(data, 'shape', type(data))}")
    if data.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 data are required, got {data.dtype}")
    C_, D, H, W = data.shape
    if not 1 <= C_ <= L.PREP_MAX_CHANNELS or min(D, H, W) < 1:
        raise RuntimeError(f"{what}: 1 .. {L.PREP_MAX_CHANNELS} channels and a non-empty volume, got {tuple(data.shape)}")
    if D * H * W > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"{what}: at most 2^31 - 1 voxels per channel, got {tuple(data.shape)}")
    sc, sz, sy, sx = data.stride()
    if W > 1 and sx != 1:
        raise RuntimeError(f"{what}: data need a unit stride along the last dimension")
    if (H > 1 and sy < W) or min(sc, sz) < 0:
        raise RuntimeError(f"{what}: unsupported data strides {data.stride()}")
    return C_, D, H, W, sc, sz, max(sy, W)


def _prep_box(box_start, box_shape, shape, what: str):
    box_start = (0, 0, 0) if box_start is None else tuple(int(v) for v in box_start)
    box_shape = tuple(n - b for n, b in zip(shape, box_start)) if box_shape is None else tuple(int(v) for v in box_shape)
    if len(box_start) != 3 or len(box_shape) != 3:
        raise RuntimeError(f"{what}: box_start and box_shape have three entries each")
    if any(bs < 1 or b0 < 0 or b0 + bs > n for b0, bs, n in zip(box_start, box_shape, shape)):
        raise RuntimeError(f"{what}: the box {box_start} + {box_shape} does not lie inside the volume {tuple(shape)}")
    return box_start, box_shape


def _crop_args(data, mask, seg, box_start, box_shape, masked, nonzero_label, what: str):
    C_, D, H, W, sc, sz, sy = _prep_data(data, what)
    box_start, box_shape = _prep_box(box_start, box_shape, (D, H, W), what)
    if mask is not None:
        _same_volume(mask, f"{what}: mask", torch.uint8, (D, H, W), data.device)
    seg_code = L.PREP_SEG_NONE
    if seg is not None:
        if not isinstance(seg, torch.Tensor) or seg.dtype not in _SEG_DTYPES:
            raise RuntimeError(f"{what}: seg must be a float32, uint8 or int16 tensor, got {getattr(seg, 'dtype', type(seg))}")
        _same_volume(seg, f"{what}: seg", seg.dtype, (D, H, W), data.device)
        seg_code = _SEG_DTYPES[seg.dtype]
    nonzero_label = int(nonzero_label)
    if not -1 <= nonzero_label <= 32767:
        raise RuntimeError(f"{what}: nonzero_label must lie in [-1, 32767], got {nonzero_label}")
    a = L.CropArgs()
    a.channels, a.depth, a.height, a.width = C_, D, H, W
    a.box_z, a.box_y, a.box_x = box_start
    a.box_depth, a.box_height, a.box_width = box_shape
    a.seg_dtype, a.masked, a.nonzero_label = seg_code, 1 if masked else 0, nonzero_label
    a.stride_c, a.stride_z, a.stride_y = sc, sz, sy
    a.data, a.mask, a.seg, a.stream = data.data_ptr(), L.fptr(mask), L.fptr(seg), L.stream_handle(data)
    return a, box_shape


def nonzero_mask_bbox(lib: L.SegmLib, data: torch.Tensor):
    """data (C, D, H, W) fp32 with a unit stride along x, C <= 8.  -> (mask uint8 (D, H, W): 1 where any channel is != 0 (NaN is);
    bbox int32 (6,) on the device = [z0, y0, x0, z1, y1, x1], half-open; z1 = y1 = x1 = 0 for an all-zero volume)."""
    C_, D, H, W, sc, sz, sy = _prep_data(data, "nonzero_mask_bbox")
    mask = torch.empty(D, H, W, dtype=torch.uint8, device=data.device)
    bbox = torch.empty(6, dtype=torch.int32, device=data.device)
    a = L.NonzeroMaskBboxArgs()
    a.channels, a.depth, a.height, a.width = C_, D, H, W
    a.stride_c, a.stride_z, a.stride_y = sc, sz, sy
    a.data, a.mask, a.bbox, a.stream = data.data_ptr(), mask.data_ptr(), bbox.data_ptr(), L.stream_handle(data)
    lib.check(lib.dll.segm_nonzero_mask_bbox(a), "nonzero_mask_bbox")
    return mask, bbox


def crop_stats(lib: L.SegmLib, data: torch.Tensor, box_start=None, box_shape=None, mask: torch.Tensor = None, seg: torch.Tensor = None,
               masked: bool = False, nonzero_label: int = -1):
    """Per-channel mean and population std of data (C, D, H, W) over the box (default: the volume), with `masked` over the box's
    voxels whose relabelled seg is >= 0 (mask: the filled non-zero mask, uint8 (D, H, W); seg: float32 / uint8 / int16 (D, H, W) or
    None).  fp64, fixed order.  -> (stats64 float64 (17,): mean [0:8], std [8:16], voxel count [16]; stats32 float32 (16,)), on the device."""
    if masked and mask is None:
        raise RuntimeError("crop_stats: the masked form needs the mask")
    a, box_shape = _crop_args(data, mask, seg, box_start, box_shape, masked, nonzero_label, "crop_stats")
    stats64 = torch.zeros(17, dtype=torch.float64, device=data.device)
    stats32 = torch.zeros(16, dtype=torch.float32, device=data.device)
    nbytes = lib.dll.segm_crop_stats_workspace_bytes(a.channels, *box_shape)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=data.device)
    a.stats64, a.stats32, a.workspace, a.workspace_bytes = stats64.data_ptr(), stats32.data_ptr(), ws.data_ptr(), nbytes
    lib.check(lib.dll.segm_crop_stats(a), "crop_stats")
    return stats64, stats32


def crop_normalize(lib: L.SegmLib, data: torch.Tensor, stats32: torch.Tensor, box_start=None, box_shape=None, mask: torch.Tensor = None,
                   seg: torch.Tensor = None, masked: bool = False, nonzero_label: int = -1, want_seg: bool = True):
    """The box of data (C, D, H, W), normalised with `stats32` (as `crop_stats` gives it): (x - mean) / max(std, 1e-8) in fp32; with
    `masked` the voxels whose relabelled seg is < 0 are copied.  With `want_seg` (needs the mask) also the relabelled seg and its label
    counts.  -> (out float32 (C, d, h, w), seg_out int16 (d, h, w) or None, counts int64 (260,) on the device or None)."""
    if (want_seg or masked) and mask is None:
        raise RuntimeError("crop_normalize: the relabelled seg and the masked form need the mask")
    a, box_shape = _crop_args(data, mask, seg, box_start, box_shape, masked, nonzero_label, "crop_normalize")
    _same_volume(stats32, "crop_normalize: stats32", torch.float32, (16,), data.device)
    out = torch.empty((a.channels,) + box_shape, dtype=torch.float32, device=data.device)
    seg_out = counts = None
    if want_seg:
        seg_out = torch.empty(box_shape, dtype=torch.int16, device=data.device)
        counts = torch.empty(L.PREP_COUNT_BINS, dtype=torch.int64, device=data.device)
        a.seg_out, a.counts = seg_out.data_ptr(), counts.data_ptr()
    a.stats32, a.out = stats32.data_ptr(), out.data_ptr()
    lib.check(lib.dll.segm_crop_normalize(a), "crop_normalize")
    return out, seg_out, counts


def crop_clip_normalize(lib: L.SegmLib, data: torch.Tensor, stats32: torch.Tensor, box_start=None, box_shape=None, mask: torch.Tensor = None,
                        seg: torch.Tensor = None, nonzero_label: int = -1, want_seg: bool = True):
    """`crop_normalize` with the CT clip in front: (min(max(x, lower), upper) - mean) / max(std, 1e-8) in fp32.  `stats32` float32
    (32,): mean [0:8], std [8:16], lower [16:24], upper [24:32].  There is no masked form.  -> (out, seg_out or None, counts or None)."""
    if want_seg and mask is None:
        raise RuntimeError("crop_clip_normalize: the relabelled seg needs the mask")
    a, box_shape = _crop_args(data, mask, seg, box_start, box_shape, False, nonzero_label, "crop_clip_normalize")
    _same_volume(stats32, "crop_clip_normalize: stats32", torch.float32, (32,), data.device)
    out = torch.empty((a.channels,) + box_shape, dtype=torch.float32, device=data.device)
    seg_out = counts = None
    if want_seg:
        seg_out = torch.empty(box_shape, dtype=torch.int16, device=data.device)
        counts = torch.empty(L.PREP_COUNT_BINS, dtype=torch.int64, device=data.device)
        a.seg_out, a.counts = seg_out.data_ptr(), counts.data_ptr()
    a.stats32, a.out = stats32.data_ptr(), out.data_ptr()
    lib.check(lib.dll.segm_crop_clip_normalize(a), "crop_clip_normalize")
    return out, seg_out, counts


# ---------------------------------------------------------------------------------------------------------
# the intensity fingerprint of a case (csrc/fingerprint.hip): foreground count and sums, order statistics, gather by rank
# ---------------------------------------------------------------------------------------------------------
class FgState:
    """What `fg_count` leaves for `fg_order_stats` and `fg_gather`: the tensors (kept alive), the argument skeleton, the workspace"""

    def __init__(self, data, seg, workspace, args):
        self.data, self.seg, self.workspace, self.args = data, seg, workspace, args

    def fresh(self) -> "L.FgArgs":
        a = L.FgArgs()
        C.memmove(C.byref(a), C.byref(self.args), C.sizeof(L.FgArgs))
        return a


def fg_count(lib: L.SegmLib, data: torch.Tensor, seg: torch.Tensor, workspace: torch.Tensor = None):
    """data (C, D, H, W) fp32 with a unit stride along x, C <= 8; seg (D, H, W) float32 / uint8 / int16, contiguous.  Foreground is
    seg > 0.  -> (count int64 (1,): the number n of foreground voxels; sums float64 (8,): per channel the fp64 sum of the foreground
    values, fixed order; state for `fg_order_stats` / `fg_gather`), all on the device.  `workspace`: a uint8 tensor to use instead
    of a fresh one (`segm_fg_workspace_bytes`)."""
    C_, D, H, W, sc, sz, sy = _prep_data(data, "fg_count")
    if not isinstance(seg, torch.Tensor) or seg.dtype not in _SEG_DTYPES:
        raise RuntimeError(f"fg_count: seg must be a float32, uint8 or int16 tensor, got {getattr(seg, 'dtype', type(seg))}")
    _same_volume(seg, "fg_count: seg", seg.dtype, (D, H, W), data.device)
    nbytes = lib.dll.segm_fg_workspace_bytes(C_, D * H * W)
    if nbytes == 0:
        raise RuntimeError(f"fg_count: no workspace size for {tuple(data.shape)}")
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=data.device)
    elif not isinstance(workspace, torch.Tensor) or workspace.device != data.device or not workspace.is_contiguous():
        raise RuntimeError("fg_count: the workspace must be a contiguous tensor on the data's device")
    count = torch.empty(1, dtype=torch.int64, device=data.device)
    sums = torch.zeros(L.PREP_MAX_CHANNELS, dtype=torch.float64, device=data.device)
    a = L.FgArgs()
    a.channels, a.depth, a.height, a.width = C_, D, H, W
    a.seg_dtype = _SEG_DTYPES[seg.dtype]
    a.stride_c, a.stride_z, a.stride_y = sc, sz, sy
    a.data, a.seg, a.stream = data.data_ptr(), seg.data_ptr(), L.stream_handle(data)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    state = FgState(data, seg, workspace, a)
    b = state.fresh()
    b.count, b.sums = count.data_ptr(), sums.data_ptr()
    lib.check(lib.dll.segm_fg_count(b), "fg_count")
    return count, sums, state


def fg_order_stats(lib: L.SegmLib, state: FgState, n: int, ranks) -> torch.Tensor:
    """-> float32 (C, len(ranks)) on the device: per channel the ranks[r]-th smallest foreground value (0-based; np.sort(fg)[k]).
    Up to 8 ranks in [0, n), repeats allowed; `n` as `fg_count` reported it.  Exact: radix selection, three passes, no readback."""
    ranks = [int(k) for k in ranks]
    n = int(n)
    if not 1 <= len(ranks) <= L.FG_MAX_RANKS:
        raise RuntimeError(f"fg_order_stats: 1 .. {L.FG_MAX_RANKS} ranks per call, got {len(ranks)}")
    if n < 1 or any(not 0 <= k < n for k in ranks):
        raise RuntimeError(f"fg_order_stats: every rank must lie in [0, {n}), got {ranks}")
    out = torch.empty(state.args.channels, L.FG_MAX_RANKS, dtype=torch.float32, device=state.data.device)
    a = state.fresh()
    a.n, a.n_ranks, a.out = n, len(ranks), out.data_ptr()
    for r, k in enumerate(ranks):
        a.ranks[r] = k
    lib.check(lib.dll.segm_fg_order_stats(a), "fg_order_stats")
    return out[:, :len(ranks)]


def fg_gather(lib: L.SegmLib, state: FgState, n: int, idx) -> torch.Tensor:
    """-> float32 (C, m) on the device: channel c at the idx[j]-th foreground voxel in C order - `images[c][mask][idx]` without the
    compaction.  idx: int64, (m,) for all channels or (C, m) with a row per channel; unsorted, repeats allowed, each in [0, n).  A
    numpy array or host tensor is checked against n here and uploaded; a device tensor is the caller's word (an index outside [0, n)
    gives NaN)."""
    n = int(n)
    dev = state.data.device
    if isinstance(idx, np.ndarray):
        idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64))
    if not isinstance(idx, torch.Tensor) or idx.dtype != torch.int64 or idx.dim() not in (1, 2):
        raise RuntimeError(f"fg_gather: idx must be int64 of shape (m,) or (C, m), got {getattr(idx, 'dtype', type(idx))}")
    C_ = state.args.channels
    if idx.dim() == 2 and idx.shape[0] != C_:
        raise RuntimeError(f"fg_gather: a per-channel idx needs {C_} rows, got {tuple(idx.shape)}")
    m = int(idx.shape[-1])
    if not 1 <= m <= L.FG_MAX_INDICES:
        raise RuntimeError(f"fg_gather: 1 .. {L.FG_MAX_INDICES} indices per call, got {m}")
    if n < 1:
        raise RuntimeError("fg_gather: there is no foreground voxel to index")
    if idx.device.type == "cpu":
        if int(idx.min()) < 0 or int(idx.max()) >= n:
            raise RuntimeError(f"fg_gather: every index must lie in [0, {n}), got [{int(idx.min())}, {int(idx.max())}]")
        idx = idx.to(dev)
    elif idx.device != dev:
        raise RuntimeError(f"fg_gather: idx lies on {idx.device}, the data on {dev}")
    idx = idx.contiguous()
    out = torch.empty(C_, m, dtype=torch.float32, device=dev)
    a = state.fresh()
    a.n, a.idx, a.n_idx, a.idx_stride_c, a.out = n, idx.data_ptr(), m, (m if idx.dim() == 2 else 0), out.data_ptr()
    lib.check(lib.dll.segm_fg_gather(a), "fg_gather")
    return out


# ---------------------------------------------------------------------------------------------------------
# resampling a case (csrc/resample.hip): cubic / linear zoom of the data, the label rule for the seg
# ---------------------------------------------------------------------------------------------------------
def _zoom_shape(shape, what: str):
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise RuntimeError(f"{what}: the new shape has three entries, got {shape}")
    if any(not 1 <= n <= L.ZOOM_MAX_SIDE for n in shape):
        raise RuntimeError(f"{what}: every side must lie in [1, {L.ZOOM_MAX_SIDE}], got {shape}")
    if shape[0] * shape[1] * shape[2] > L.CCL_MAX_VOXELS:
        raise RuntimeError(f"{what}: at most 2^31 - 1 voxels per channel, got {shape}")
    return shape


def zoom(lib: L.SegmLib, data: torch.Tensor, new_shape, order: int = 3, clip: bool = True) -> torch.Tensor:
    """data (C, D, H, W) fp32 with a unit stride along x, C <= 8 -> (C,) + new_shape fp32: skimage's `resize(order, mode='edge',
    anti_aliasing=False, clip=clip)` per channel (scipy.ndimage.zoom with mode='nearest', grid_mode=True).  order 3 (cubic B-spline,
    fp64 coefficients in a workspace of C (D + 4) (H + 4) (W + 4) doubles) or 1 (trilinear).  Sides up to 2048; two calls are bit-equal."""
    C_, D, H, W, sc, sz, sy = _prep_data(data, "zoom")
    _zoom_shape((D, H, W), "zoom: data")
    new_shape = _zoom_shape(new_shape, "zoom")
    if order not in (1, 3):
        raise RuntimeError(f"zoom: order 1 or 3, got {order}")
    nbytes = lib.dll.segm_zoom_workspace_bytes(C_, D, H, W, order)
    if nbytes == 0:
        raise RuntimeError(f"zoom: no workspace size for {tuple(data.shape)}, order {order}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=data.device)
    out = torch.empty((C_,) + new_shape, dtype=torch.float32, device=data.device)
    a = L.ZoomArgs()
    a.channels, a.depth, a.height, a.width = C_, D, H, W
    a.out_depth, a.out_height, a.out_width = new_shape
    a.order, a.clip = order, 1 if clip else 0
    a.stride_c, a.stride_z, a.stride_y = sc, sz, sy
    a.data, a.out, a.workspace, a.workspace_bytes, a.stream = data.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, L.stream_handle(data)
    lib.check(lib.dll.segm_zoom(a), "zoom")
    return out


def zoom_labels(lib: L.SegmLib, seg: torch.Tensor, new_shape, want_counts: bool = True):
    """seg (D, H, W) int16, contiguous -> (new_shape int16, counts int64 (260,) on the device or None): batchgenerators'
    `resize_segmentation(seg, new_shape, 1)` - the largest label whose trilinear weight is >= 0.5, else 0 - and the label counts of
    the result in `crop_normalize`'s layout."""
    if not isinstance(seg, torch.Tensor) or seg.dim() != 3:
        raise RuntimeError(f"zoom_labels: a (D, H, W) seg is required, got {getattr(seg, 'shape', type(seg))}")
    _same_volume(seg, "zoom_labels: seg", torch.int16, tuple(seg.shape), seg.device)
    D, H, W = _zoom_shape(seg.shape, "zoom_labels: seg")
    new_shape = _zoom_shape(new_shape, "zoom_labels")
    out = torch.empty(new_shape, dtype=torch.int16, device=seg.device)
    counts = torch.empty(L.PREP_COUNT_BINS, dtype=torch.int64, device=seg.device) if want_counts else None
    a = L.ZoomLabelsArgs()
    a.depth, a.height, a.width = D, H, W
    a.out_depth, a.out_height, a.out_width = new_shape
    a.seg, a.out, a.counts, a.stream = seg.data_ptr(), out.data_ptr(), L.fptr(counts), L.stream_handle(seg)
    lib.check(lib.dll.segm_zoom_labels(a), "zoom_labels")
    return out, counts


def _zoom_source(source, out_slices: int, device, what: str) -> torch.Tensor:
    """the slice table of the separate-z entries: `out_slices` integers -> int32 on the device, contiguous"""
    t = source if isinstance(source, torch.Tensor) else torch.as_tensor(np.asarray(source))
    if t.dim() != 1 or t.numel() != out_slices or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise RuntimeError(f"{what}: source holds one integer per output slice ({out_slices}), got {tuple(t.shape)} {t.dtype}")
    return t.to(device=device, dtype=torch.int32).contiguous()


def zoom_slices(lib: L.SegmLib, data: torch.Tensor, new_shape, source, order: int = 3, clip: bool = True) -> torch.Tensor:
    """data (C, S, H, W) fp32 with a unit stride along x, C <= 8 -> (C,) + new_shape fp32: output slice k is input slice source[k]
    (int32 on the device, or host integers; clamped to [0, S) by the kernel) resized in its plane as `zoom` resizes a volume - order 3
    or 1 - and with `clip` clamped to the range of that slice alone.  The separate-z branch of the reference's `resample_data_or_seg`
    with order_z = 0.  An unchanged in-plane shape copies the slices.  Two calls are bit-equal."""
    C_, S, H, W, sc, ss, sy = _prep_data(data, "zoom_slices")
    _zoom_shape((S, H, W), "zoom_slices: data")
    new_shape = _zoom_shape(new_shape, "zoom_slices")
    if order not in (1, 3):
        raise RuntimeError(f"zoom_slices: order 1 or 3, got {order}")
    src = _zoom_source(source, new_shape[0], data.device, "zoom_slices")
    nbytes = lib.dll.segm_zoom_slices_workspace_bytes(C_, S, H, W, new_shape[1], new_shape[2], order)
    if nbytes == 0:
        raise RuntimeError(f"zoom_slices: no workspace size for {tuple(data.shape)} -> {new_shape}, order {order}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=data.device)
    out = torch.empty((C_,) + new_shape, dtype=torch.float32, device=data.device)
    a = L.ZoomSlicesArgs()
    a.channels, a.slices, a.height, a.width = C_, S, H, W
    a.out_slices, a.out_height, a.out_width = new_shape
    a.order, a.clip = order, 1 if clip else 0
    a.stride_c, a.stride_s, a.stride_y = sc, ss, sy
    a.data, a.source, a.out, a.workspace, a.workspace_bytes = data.data_ptr(), src.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes
    a.stream = L.stream_handle(data)
    lib.check(lib.dll.segm_zoom_slices(a), "zoom_slices")
    return out


def zoom_labels_slices(lib: L.SegmLib, seg: torch.Tensor, new_shape, source, want_counts: bool = True):
    """seg (S, H, W) int16, contiguous -> (new_shape int16, counts int64 (260,) on the device or None): output slice k is
    `resize_segmentation(seg[source[k]], new_shape[1:], 1)` - the largest label whose bilinear weight is >= 0.5, else 0 - and the label
    counts of the result in `crop_normalize`'s layout."""
    if not isinstance(seg, torch.Tensor) or seg.dim() != 3:
        raise RuntimeError(f"zoom_labels_slices: a (S, H, W) seg is required, got {getattr(seg, 'shape', type(seg))}")
    _same_volume(seg, "zoom_labels_slices: seg", torch.int16, tuple(seg.shape), seg.device)
    S, H, W = _zoom_shape(seg.shape, "zoom_labels_slices: seg")
    new_shape = _zoom_shape(new_shape, "zoom_labels_slices")
    src = _zoom_source(source, new_shape[0], seg.device, "zoom_labels_slices")
    out = torch.empty(new_shape, dtype=torch.int16, device=seg.device)
    counts = torch.empty(L.PREP_COUNT_BINS, dtype=torch.int64, device=seg.device) if want_counts else None
    a = L.ZoomLabelsSlicesArgs()
    a.slices, a.height, a.width = S, H, W
    a.out_slices, a.out_height, a.out_width = new_shape
    a.seg, a.source, a.out, a.counts, a.stream = seg.data_ptr(), src.data_ptr(), out.data_ptr(), L.fptr(counts), L.stream_handle(seg)
    lib.check(lib.dll.segm_zoom_labels_slices(a), "zoom_labels_slices")
    return out, counts


# ---------------------------------------------------------------------------------------------------------
# augmentation at the reference's interpolation orders (csrc/augment.hip): spline coefficients, the affine warp of data and
# labels, order-0 zoom, gaussian blur.  Matrices, sigmas and flags are host values and travel in the argument structs.
# ---------------------------------------------------------------------------------------------------------
def _aug_batch(x, what: str):
    """(N, C, D, H, W) fp32 with a unit stride along x, N <= 8, C <= 8: -> (N, C, D, H, W, stride_n, stride_c, stride_z, stride_y)"""
    if not isinstance(x, torch.Tensor) or x.dim() != 5:
        raise RuntimeError(f"{what}: a batch (N, C, D, H, W) is required, got {getattr(x, 'shape', type(x))}")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 data are required, got {x.dtype}")
    N, C_, D, H, W = x.shape
    if not 1 <= N <= L.AUG_MAX_SAMPLES or not 1 <= C_ <= L.PREP_MAX_CHANNELS:
        raise RuntimeError(f"{what}: 1 .. {L.AUG_MAX_SAMPLES} samples and 1 .. {L.PREP_MAX_CHANNELS} channels per call, got {tuple(x.shape)}")
    _zoom_shape((D, H, W), what)
    sn, sc, sz, sy, sx = x.stride()
    if W > 1 and sx != 1:
        raise RuntimeError(f"{what}: data need a unit stride along the last dimension")
    if (H > 1 and sy < W) or min(sn, sc, sz) < 0:
        raise RuntimeError(f"{what}: unsupported data strides {x.stride()}")
    return N, C_, D, H, W, sn, sc, sz, max(sy, W)


def _aug_flags(on, n: int, what: str):
    on = [True] * n if on is None else [bool(v) for v in on]
    if len(on) != n:
        raise RuntimeError(f"{what}: {n} on / off flags are required, got {len(on)}")
    return on


def _aug_matrices(a, matrices, n: int, what: str) -> None:
    import numpy as np
    m = np.asarray(matrices, dtype=np.float64)
    if m.shape != (n, 3, 4) or not np.isfinite(m).all():
        raise RuntimeError(f"{what}: finite matrices ({n}, 3, 4) [A | t] are required, got shape {m.shape}")
    for b in range(n):
        a.matrix[b][:] = m[b].reshape(12).tolist()


def spline_coefs(lib: L.SegmLib, x: torch.Tensor, on=None) -> torch.Tensor:
    """x (N, C, D, H, W) fp32, N <= 8, C <= 8 -> float64 (N, C, D, H, W): `scipy.ndimage.spline_filter(x, 3, output=float64,
    mode='mirror')` of every volume of the samples that are `on` (default: all); the volumes of the others are left unwritten."""
    N, C_, D, H, W, sn, sc, sz, sy = _aug_batch(x, "spline_coefs")
    on = _aug_flags(on, N, "spline_coefs")
    nbytes = lib.dll.segm_spline_coefs_workspace_bytes(N, C_, D, H, W)
    if nbytes == 0:
        raise RuntimeError(f"spline_coefs: no workspace size for {tuple(x.shape)}")
    coefs = torch.empty((N, C_, D, H, W), dtype=torch.float64, device=x.device)
    a = L.SplineCoefsArgs()
    a.samples, a.channels, a.depth, a.height, a.width = N, C_, D, H, W
    a.stride_n, a.stride_c, a.stride_z, a.stride_y = sn, sc, sz, sy
    a.on[:N] = [int(v) for v in on]
    a.data, a.workspace, a.workspace_bytes, a.stream = x.data_ptr(), coefs.data_ptr(), nbytes, L.stream_handle(x)
    lib.check(lib.dll.segm_spline_coefs(a), "spline_coefs")
    return coefs


def affine_spline3(lib: L.SegmLib, x: torch.Tensor, coefs: torch.Tensor, matrices, on=None, cval: float = 0.0) -> torch.Tensor:
    """x (N, C, D, H, W) fp32 and its `spline_coefs` -> (N, C, D, H, W) fp32: sample n at p = A_n (z, y, x)^T + t_n, matrices (N, 3, 4)
    = [A | t] host float64 - `map_coordinates(x.astype(float64), p, order=3, mode='constant', cval).astype(float32)`.  Samples that
    are off are copied bit for bit."""
    N, C_, D, H, W, sn, sc, sz, sy = _aug_batch(x, "affine_spline3")
    on = _aug_flags(on, N, "affine_spline3")
    _same_volume(coefs, "affine_spline3: coefs", torch.float64, tuple(x.shape), x.device)
    out = torch.empty((N, C_, D, H, W), dtype=torch.float32, device=x.device)
    a = L.AffineSpline3Args()
    a.samples, a.channels, a.depth, a.height, a.width = N, C_, D, H, W
    a.stride_n, a.stride_c, a.stride_z, a.stride_y = sn, sc, sz, sy
    _aug_matrices(a, matrices, N, "affine_spline3")
    a.cval = float(cval)
    a.on[:N] = [int(v) for v in on]
    a.data, a.coefs, a.out, a.stream = x.data_ptr(), coefs.data_ptr(), out.data_ptr(), L.stream_handle(x)
    lib.check(lib.dll.segm_affine_spline3(a), "affine_spline3")
    return out


def affine_labels(lib: L.SegmLib, seg: torch.Tensor, matrices, on=None) -> torch.Tensor:
    """seg (N, D, H, W) int16 or int64, contiguous, N <= 8 -> the same shape and dtype: 0 outside the volume, inside the largest
    label whose trilinear weight at p is >= 0.5, else 0 (batchgenerators' `interpolate_img(is_seg=True, order=1, cval=-1)`).
    Samples that are off are copied."""
    if not isinstance(seg, torch.Tensor) or seg.dim() != 4:
        raise RuntimeError(f"affine_labels: a (N, D, H, W) seg is required, got {getattr(seg, 'shape', type(seg))}")
    if seg.dtype not in (torch.int16, torch.int64):
        raise RuntimeError(f"affine_labels: an int16 or int64 seg is required, got {seg.dtype}")
    if not seg.is_contiguous():
        raise RuntimeError("affine_labels: seg must be contiguous")
    N, D, H, W = seg.shape
    if not 1 <= N <= L.AUG_MAX_SAMPLES:
        raise RuntimeError(f"affine_labels: 1 .. {L.AUG_MAX_SAMPLES} samples per call, got {N}")
    _zoom_shape((D, H, W), "affine_labels")
    on = _aug_flags(on, N, "affine_labels")
    out = torch.empty_like(seg)
    a = L.AffineLabelsArgs()
    a.samples, a.depth, a.height, a.width, a.wide = N, D, H, W, 1 if seg.dtype == torch.int64 else 0
    _aug_matrices(a, matrices, N, "affine_labels")
    a.on[:N] = [int(v) for v in on]
    a.seg, a.out, a.stream = seg.data_ptr(), out.data_ptr(), L.stream_handle(seg)
    lib.check(lib.dll.segm_affine_labels(a), "affine_labels")
    return out


def zoom_nearest(lib: L.SegmLib, data: torch.Tensor, new_shape) -> torch.Tensor:
    """data (C, D, H, W) fp32 with a unit stride along x, C <= 8 -> (C,) + new_shape: `scipy.ndimage.zoom(order=0, mode='nearest',
    grid_mode=True)` per channel (skimage's `resize(order=0, mode='edge', anti_aliasing=False)`)."""
    C_, D, H, W, sc, sz, sy = _prep_data(data, "zoom_nearest")
    _zoom_shape((D, H, W), "zoom_nearest: data")
    new_shape = _zoom_shape(new_shape, "zoom_nearest")
    out = torch.empty((C_,) + new_shape, dtype=torch.float32, device=data.device)
    a = L.ZoomNearestArgs()
    a.channels, a.depth, a.height, a.width = C_, D, H, W
    a.out_depth, a.out_height, a.out_width = new_shape
    a.stride_c, a.stride_z, a.stride_y = sc, sz, sy
    a.data, a.out, a.stream = data.data_ptr(), out.data_ptr(), L.stream_handle(data)
    lib.check(lib.dll.segm_zoom_nearest(a), "zoom_nearest")
    return out


def gauss_blur(lib: L.SegmLib, x: torch.Tensor, sigma, on=None) -> torch.Tensor:
    """x (N, C, D, H, W) fp32, N <= 8, C <= 8; sigma and on: N * C host values, volume n * C + c -> (N, C, D, H, W) fp32:
    `scipy.ndimage.gaussian_filter(x[n, c], sigma)` (truncate 4, mode 'reflect', fp32 between the passes) for the volumes that are
    on, a copy of the others.  int(4 sigma + 0.5) must not exceed 4."""
    N, C_, D, H, W, sn, sc, sz, sy = _aug_batch(x, "gauss_blur")
    on = _aug_flags(on, N * C_, "gauss_blur")
    sigma = [float(v) for v in sigma]
    if len(sigma) != N * C_:
        raise RuntimeError(f"gauss_blur: {N * C_} sigmas are required, got {len(sigma)}")
    if any(f and not (s > 0.0 and int(4.0 * s + 0.5) <= L.BLUR_MAX_RADIUS) for s, f in zip(sigma, on)):
        raise RuntimeError(f"gauss_blur: every sigma must be positive with a radius int(4 sigma + 0.5) <= {L.BLUR_MAX_RADIUS}, got {sigma}")
    out = torch.empty((N, C_, D, H, W), dtype=torch.float32, device=x.device)
    ws = torch.empty_like(out) if any(on) else None
    a = L.GaussBlurArgs()
    a.samples, a.channels, a.depth, a.height, a.width = N, C_, D, H, W
    a.stride_n, a.stride_c, a.stride_z, a.stride_y = sn, sc, sz, sy
    a.sigma[:N * C_] = sigma
    a.on[:N * C_] = [int(v) for v in on]
    a.data, a.out, a.stream = x.data_ptr(), out.data_ptr(), L.stream_handle(x)
    a.workspace, a.workspace_bytes = L.fptr(ws), 0 if ws is None else ws.numel() * 4
    lib.check(lib.dll.segm_gauss_blur(a), "gauss_blur")
    return out


# ---------------------------------------------------------------------------------------------------------
# intensity augmentation (csrc/intensity.hip): noise, brightness, contrast, gamma and the mirror as streaming passes.  The op and the
# parameters of every plane are host values and travel in the argument struct; the statistics stay on the device.
# ---------------------------------------------------------------------------------------------------------
def _intensity_batch(x, what: str):
    """(N, C, D, H, W) fp32 with a unit stride along x, N * C <= 64 -> (N, C, D, H, W, stride_n, stride_c, stride_z, stride_y)"""
    if not isinstance(x, torch.Tensor) or x.dim() != 5:
        raise RuntimeError(f"{what}: a batch (N, C, D, H, W) is required, got {getattr(x, 'shape', type(x))}")
    if x.dtype != torch.float32:
        raise RuntimeError(f"{what}: float32 data are required, got {x.dtype}")
    N, C_, D, H, W = x.shape
    if min(x.shape) < 1 or N * C_ > L.AUG_MAX_VOLUMES:
        raise RuntimeError(f"{what}: 1 .. {L.AUG_MAX_VOLUMES} planes (samples x channels) of at least one voxel per call, got {tuple(x.shape)}")
    if D * H * W >= 2 ** 31:
        raise RuntimeError(f"{what}: fewer than 2^31 voxels per plane are required, got {tuple(x.shape)}")
    sn, sc, sz, sy, sx = x.stride()
    if W > 1 and sx != 1:
        raise RuntimeError(f"{what}: data need a unit stride along the last dimension")
    if (H > 1 and sy < W) or min(sn, sc, sz) < 0:
        raise RuntimeError(f"{what}: unsupported data strides {x.stride()}")
    return N, C_, D, H, W, sn, sc, sz, max(sy, W)


def _intensity_rows(t, planes: int, like: torch.Tensor, what: str) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (planes, L.INTENSITY_STATS_DOUBLES) \
            or not t.is_contiguous() or t.device != like.device:
        raise RuntimeError(f"{what}: contiguous float64 rows ({planes}, {L.INTENSITY_STATS_DOUBLES}) on {like.device} are required, got "
                           f"{getattr(t, 'shape', type(t))} {getattr(t, 'dtype', '')}")


def _intensity_args(x: torch.Tensor, ops, what: str):
    """`ops`: one entry per plane n * C + c - None (off), ("noise", s, field (D, H, W)), ("scale", m), ("contrast", m, f) or
    ("gamma", g, invert)"""
    import math
    N, C_, D, H, W, sn, sc, sz, sy = _intensity_batch(x, what)
    ops = list(ops)
    if len(ops) != N * C_:
        raise RuntimeError(f"{what}: {N * C_} ops (one per plane) are required, got {len(ops)}")
    a = L.IntensityArgs()
    a.samples, a.channels, a.depth, a.height, a.width = N, C_, D, H, W
    a.stride_n, a.stride_c, a.stride_z, a.stride_y, a.stride_x = sn, sc, sz, sy, 1
    a.data, a.stream = x.data_ptr(), L.stream_handle(x)
    arity = {"noise": 3, "scale": 2, "contrast": 3, "gamma": 3}
    for v, op in enumerate(ops):
        if op is None:
            continue
        if not isinstance(op, (tuple, list)) or not op or op[0] not in arity or len(op) != arity[op[0]]:
            raise RuntimeError(f"{what}: plane {v}: None, ('noise', s, field), ('scale', m), ('contrast', m, f) or ('gamma', g, invert) "
                               f"is required, got {op!r}")
        kind = op[0]
        values = [float(p) for p in (op[1:2] if kind in ("noise", "gamma") else op[1:])]
        if not all(math.isfinite(p) for p in values):
            raise RuntimeError(f"{what}: plane {v}: finite parameters are required, got {op[1:]!r}")
        if kind == "noise":
            field = op[2]
            if not isinstance(field, torch.Tensor) or field.dtype != torch.float32 or tuple(field.shape) != (D, H, W) \
                    or not field.is_contiguous() or field.device != x.device:
                raise RuntimeError(f"{what}: plane {v}: a contiguous float32 noise field {(D, H, W)} on {x.device} is required, got "
                                   f"{getattr(field, 'shape', type(field))} {getattr(field, 'dtype', '')}")
            a.op[v], a.a[v], a.noise[v] = L.INTENSITY_NOISE, values[0], field.data_ptr()
        elif kind == "scale":
            a.op[v], a.a[v] = L.INTENSITY_SCALE, values[0]
        elif kind == "contrast":
            a.op[v], a.a[v], a.b[v] = L.INTENSITY_CONTRAST, values[0], values[1]
        else:
            a.op[v], a.a[v], a.invert[v] = L.INTENSITY_GAMMA, values[0], int(bool(op[2]))
    return a, N * C_, D * H * W


def intensity_stats(lib: L.SegmLib, x: torch.Tensor, ops, stage: int = 0, stats: torch.Tensor = None) -> torch.Tensor:
    """x (N, C, D, H, W) fp32, N * C <= 64, `ops` as in `intensity_apply` -> float64 rows (N * C, 8) = count, mean, population sd,
    min, max, zeros, on the device.  stage 0: of u = fl32(x m) for a contrast plane and of t = +-x for a gamma plane.  stage 1: of
    w for a gamma plane, formed from `stats` (the rows of stage 0).  Rows of planes that take no part are not written."""
    if stage not in (0, 1):
        raise RuntimeError(f"intensity_stats: stage 0 or 1 is required, got {stage!r}")
    a, planes, voxels = _intensity_args(x, ops, "intensity_stats")
    if stage == 1:
        _intensity_rows(stats, planes, x, "intensity_stats: stats")
    rows = torch.empty((planes, L.INTENSITY_STATS_DOUBLES), dtype=torch.float64, device=x.device)
    nbytes = lib.dll.segm_intensity_workspace_bytes(planes, voxels)
    if nbytes == 0:
        raise RuntimeError(f"intensity_stats: no workspace size for {tuple(x.shape)}")
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    a.stage = stage
    a.stats, a.stats2 = (rows.data_ptr(), None) if stage == 0 else (stats.data_ptr(), rows.data_ptr())
    a.workspace, a.workspace_bytes = ws.data_ptr(), nbytes
    lib.check(lib.dll.segm_intensity_stats(a), "intensity_stats")
    return rows


def intensity_apply(lib: L.SegmLib, x: torch.Tensor, ops, stats: torch.Tensor = None, stats2: torch.Tensor = None, mirror=None,
                    out_of_place: bool = False) -> torch.Tensor:
    """x (N, C, D, H, W) fp32, N * C <= 64; `ops`: per plane n * C + c None (off), ("noise", s, field): x + fl32(s field),
    ("scale", m): x m, ("contrast", m, f): u = x m clipped-stretched about its mean by f, ("gamma", g, invert) - the formulas of
    include/segmamba_hip.h.  Contrast planes read their row of `stats`, gamma planes theirs of `stats` and `stats2`
    (`intensity_stats`, stage 0 and 1), from the device.  In place (-> x; planes that are off are not touched), or with
    `out_of_place` into a new dense tensor, every plane at its mirrored position: `mirror` holds per plane the sum of 1 (flip z), 2 (flip
    y) and 4 (flip x); planes that are off are copied bit for bit."""
    a, planes, _ = _intensity_args(x, ops, "intensity_apply")
    kinds = [int(a.op[v]) for v in range(planes)]
    if any(k in (L.INTENSITY_CONTRAST, L.INTENSITY_GAMMA) for k in kinds):
        _intensity_rows(stats, planes, x, "intensity_apply: stats")
        a.stats = stats.data_ptr()
    if L.INTENSITY_GAMMA in kinds:
        _intensity_rows(stats2, planes, x, "intensity_apply: stats2")
        a.stats2 = stats2.data_ptr()
    mirror = [0] * planes if mirror is None else [int(m) for m in mirror]
    if len(mirror) != planes or any(not 0 <= m <= 7 for m in mirror):
        raise RuntimeError(f"intensity_apply: {planes} mirror masks in 0 .. 7 are required, got {mirror}")
    if any(mirror) and not out_of_place:
        raise RuntimeError("intensity_apply: a mirror needs the out-of-place form")
    if not out_of_place:
        lib.check(lib.dll.segm_intensity_apply(a), "intensity_apply")
        return x
    out = torch.empty(tuple(x.shape), dtype=torch.float32, device=x.device)
    a.mirror[:planes] = mirror
    a.out = out.data_ptr()
    a.out_stride_n, a.out_stride_c, a.out_stride_z, a.out_stride_y = out.stride()[:4]
    lib.check(lib.dll.segm_intensity_apply(a), "intensity_apply")
    return out


# ---------------------------------------------------------------------------------------------------------
# stitching a sliding-window prediction (csrc/stitch.hip): window gather, count map, blending, the close of a mirror pass.  The
# windows of a launch travel by value in the argument struct; nothing is read back to the host.
# ---------------------------------------------------------------------------------------------------------
def _stitch_sides(size, roi, what: str):
    """-> (size, roi, image = max(size, roi)) as tuples of 3 ints"""
    try:
        size, roi = tuple(int(v) for v in size), tuple(int(v) for v in roi)
    except (TypeError, ValueError):
        raise RuntimeError(f"{what}: three integer sides each for size and roi are required, got {size!r} and {roi!r}") from None
    if len(size) != 3 or len(roi) != 3 or min(size + roi) < 1:
        raise RuntimeError(f"{what}: three sides of at least 1 each for size and roi are required, got {size} and {roi}")
    image = tuple(max(s, r) for s, r in zip(size, roi))
    if image[0] * image[1] * image[2] >= 2 ** 31:
        raise RuntimeError(f"{what}: fewer than 2^31 voxels per plane are required, got {image}")
    return size, roi, image


def _stitch_dense(t, shape, dtypes, like, what: str) -> None:
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype not in dtypes or not t.is_contiguous() \
            or (like is not None and t.device != like.device) or t.data_ptr() % t.element_size():
        where = f" on {like.device}" if like is not None else ""
        raise RuntimeError(f"{what}: a contiguous tensor {tuple(shape)} of {' / '.join(str(d) for d in dtypes)}{where} is required, got "
                           f"{getattr(t, 'shape', type(t))} {getattr(t, 'dtype', '')} {getattr(t, 'device', '')}")


def _stitch_windows(a, windows, batch: int, channels: int, image, roi, what: str) -> int:
    windows = [tuple(w) for w in windows]
    if not 1 <= len(windows) <= L.STITCH_MAX_WINDOWS:
        raise RuntimeError(f"{what}: 1 .. {L.STITCH_MAX_WINDOWS} windows per launch are required, got {len(windows)}")
    if len(windows) * channels > 65535:
        raise RuntimeError(f"{what}: windows x channels must not exceed 65535, got {len(windows)} x {channels}")
    for j, w in enumerate(windows):
        if len(w) != 4 or any(int(v) != v for v in w):
            raise RuntimeError(f"{what}: window {j}: (sample, start z, y, x) integers are required, got {w!r}")
        if not 0 <= w[0] < batch or any(not 0 <= w[1 + d] <= image[d] - roi[d] for d in range(3)):
            raise RuntimeError(f"{what}: window {j} = {w} leaves the {batch} samples of the image {tuple(image)} (roi {tuple(roi)})")
        for d in range(4):
            a.window[j][d] = int(w[d])
    a.n_windows = len(windows)
    return len(windows)


def _stitch_mirror(mirror, what: str) -> int:
    if isinstance(mirror, bool) or not isinstance(mirror, int) or not 0 <= mirror <= 7:
        raise RuntimeError(f"{what}: a mirror mask in 0 .. 7 is required (1: flip z, 2: flip y, 4: flip x), got {mirror!r}")
    return mirror


def window_gather(lib: L.SegmLib, volume: torch.Tensor, roi, windows, mirror: int = 0, cval: float = 0.0) -> torch.Tensor:
    """volume (B, C, Z, Y, X) fp32 with a unit stride along x (other strides free), `windows` 1 .. 64 tuples (sample, start z, y, x)
    in the padded frame image = max(size, roi) -> (n, C, *roi) fp32 dense: the volume mirrored by `mirror` and centred in the
    padding `cval`, cut at the windows.  Neither the mirrored nor the padded volume is formed."""
    what = "window_gather"
    if not isinstance(volume, torch.Tensor) or volume.dim() != 5:
        raise RuntimeError(f"{what}: a volume (B, C, Z, Y, X) is required, got {getattr(volume, 'shape', type(volume))}")
    if volume.dtype != torch.float32:
        raise RuntimeError(f"{what}: a float32 volume is required, got {volume.dtype}")
    B, C_ = int(volume.shape[0]), int(volume.shape[1])
    if B < 1 or C_ < 1:
        raise RuntimeError(f"{what}: at least one sample and one channel are required, got {tuple(volume.shape)}")
    size, roi, image = _stitch_sides(volume.shape[2:], roi, what)
    sb, sc, sz, sy, sx = volume.stride()
    if size[2] > 1 and sx != 1:
        raise RuntimeError(f"{what}: the volume needs a unit stride along the last dimension, got strides {volume.stride()}")
    if min(sb, sc, sz, sy) < 0 or volume.data_ptr() % 4:
        raise RuntimeError(f"{what}: unsupported volume strides {volume.stride()} or a misaligned base")
    cval = float(cval)
    a = L.StitchArgs()
    n = _stitch_windows(a, windows, B, C_, image, roi, what)
    a.mirror = _stitch_mirror(mirror, what)
    out = torch.empty((n, C_) + roi, dtype=torch.float32, device=volume.device)
    a.batch, a.channels, a.cval = B, C_, cval
    a.size[:], a.roi[:] = size, roi
    a.stride_b, a.stride_c, a.stride_z, a.stride_y, a.stride_x = sb, sc, sz, sy, 1
    a.volume, a.windows_out, a.stream = volume.data_ptr(), out.data_ptr(), L.stream_handle(volume)
    lib.check(lib.dll.segm_window_gather(a), what)
    return out


def window_count(lib: L.SegmLib, weight: torch.Tensor, size, starts) -> torch.Tensor:
    """weight (*roi) fp32 dense, `starts` the window starts of the three axes (1 .. 64 each, in order) in the padded frame
    image = max(size, roi) -> the count map (*image) fp32: per voxel the weights of the covering windows, added in the order of the
    lists' product (z outermost, x fastest) - the bits of the loop `count[slice] += weight`."""
    what = "window_count"
    if not isinstance(weight, torch.Tensor) or weight.dim() != 3:
        raise RuntimeError(f"{what}: a weight map (rz, ry, rx) is required, got {getattr(weight, 'shape', type(weight))}")
    size, roi, image = _stitch_sides(size, weight.shape, what)
    _stitch_dense(weight, roi, (torch.float32,), None, f"{what}: weight")
    starts = [[int(v) for v in axis] for axis in starts]
    if len(starts) != 3 or any(not 1 <= len(axis) <= L.STITCH_MAX_STARTS for axis in starts):
        raise RuntimeError(f"{what}: three lists of 1 .. {L.STITCH_MAX_STARTS} window starts are required, got {starts}")
    a = L.StitchArgs()
    for d, axis in enumerate(starts):
        if any(not 0 <= v <= image[d] - roi[d] for v in axis):
            raise RuntimeError(f"{what}: axis {d}: a start of {axis} leaves the image {image} (roi {roi})")
        a.n_starts[d] = len(axis)
        for i, v in enumerate(axis):
            a.starts[d][i] = v
    count = torch.empty(image, dtype=torch.float32, device=weight.device)
    a.batch, a.channels = 1, 1
    a.size[:], a.roi[:] = size, roi
    a.weight, a.count, a.stream = weight.data_ptr(), count.data_ptr(), L.stream_handle(weight)
    lib.check(lib.dll.segm_window_count(a), what)
    return count


def window_blend(lib: L.SegmLib, acc: torch.Tensor, pred: torch.Tensor, weight: torch.Tensor, windows) -> torch.Tensor:
    """acc (B, Cout, *image) fp32 dense, pred (n, Cout, *roi) dense in fp32 / bf16 / fp16, weight (*roi) fp32, `windows` n tuples
    (sample, start z, y, x): acc[sample, :, start + i] += fl32(float(pred[n, :, i]) * weight[i]), the windows in their order, every
    voxel of acc written by one thread (windows of a launch may overlap).  -> acc."""
    what = "window_blend"
    if not isinstance(acc, torch.Tensor) or acc.dim() != 5 or not isinstance(pred, torch.Tensor) or pred.dim() != 5:
        raise RuntimeError(f"{what}: acc (B, Cout, Z, Y, X) and pred (n, Cout, rz, ry, rx) are required, got "
                           f"{getattr(acc, 'shape', type(acc))} and {getattr(pred, 'shape', type(pred))}")
    B, C_ = int(acc.shape[0]), int(acc.shape[1])
    if B < 1 or C_ < 1 or B * C_ > 65535:
        raise RuntimeError(f"{what}: 1 .. 65535 planes (samples x channels) are required, got {tuple(acc.shape)}")
    image, roi, _ = _stitch_sides(acc.shape[2:], pred.shape[2:], what)
    if any(r > s for r, s in zip(roi, image)):
        raise RuntimeError(f"{what}: the windows {roi} are larger than the accumulator {image}")
    _stitch_dense(acc, (B, C_) + image, (torch.float32,), None, f"{what}: acc")
    a = L.StitchArgs()
    n = _stitch_windows(a, windows, B, C_, image, roi, what)
    _stitch_dense(pred, (n, C_) + roi, (torch.float32, torch.bfloat16, torch.float16), acc, f"{what}: pred")
    _stitch_dense(weight, roi, (torch.float32,), acc, f"{what}: weight")
    a.batch, a.channels, a.dtype = B, C_, L.dtype_code(pred)
    a.size[:], a.roi[:] = image, roi
    a.pred, a.weight, a.acc, a.stream = pred.data_ptr(), weight.data_ptr(), acc.data_ptr(), L.stream_handle(acc)
    lib.check(lib.dll.segm_window_blend(a), what)
    return acc


def window_finish(lib: L.SegmLib, acc: torch.Tensor, count: torch.Tensor, total: torch.Tensor, roi, mirror: int = 0,
                  pass_index: int = 0, passes: int = 1) -> torch.Tensor:
    """Closes mirror pass `pass_index` of `passes`.  total (B, Cout, *size) fp32 dense, acc (B, Cout, *image) and count (*image) fp32
    dense, image = max(size, roi): with p the mirrored position of a voxel in the padded frame, total = acc[p] / count[p] on pass 0
    and total + acc[p] / count[p] later; the last pass divides by `passes`.  acc is all zero afterwards.  -> total."""
    what = "window_finish"
    if not isinstance(total, torch.Tensor) or total.dim() != 5:
        raise RuntimeError(f"{what}: total (B, Cout, Z, Y, X) is required, got {getattr(total, 'shape', type(total))}")
    B, C_ = int(total.shape[0]), int(total.shape[1])
    if B < 1 or C_ < 1 or B * C_ > 65535:
        raise RuntimeError(f"{what}: 1 .. 65535 planes (samples x channels) are required, got {tuple(total.shape)}")
    size, roi, image = _stitch_sides(total.shape[2:], roi, what)
    _stitch_dense(total, (B, C_) + size, (torch.float32,), None, f"{what}: total")
    _stitch_dense(acc, (B, C_) + image, (torch.float32,), total, f"{what}: acc")
    _stitch_dense(count, image, (torch.float32,), total, f"{what}: count")
    if isinstance(passes, bool) or not isinstance(passes, int) or not isinstance(pass_index, int) or passes < 1 \
            or not 0 <= pass_index < passes:
        raise RuntimeError(f"{what}: a pass index in [0, passes) is required, got {pass_index!r} of {passes!r}")
    a = L.StitchArgs()
    a.mirror = _stitch_mirror(mirror, what)
    a.batch, a.channels, a.pass_, a.passes = B, C_, pass_index, passes
    a.size[:], a.roi[:] = size, roi
    a.acc, a.count, a.total, a.stream = acc.data_ptr(), count.data_ptr(), total.data_ptr(), L.stream_handle(total)
    lib.check(lib.dll.segm_window_finish(a), what)
    return total


# ---------------------------------------------------------------------------------------------------------
# fused residual add + LayerNorm / RMSNorm (csrc/add_norm.hip)
# ---------------------------------------------------------------------------------------------------------
def _add_norm_rows(t, shape, dtypes, like, what: str):
    """a (M, N) operand of the add + norm entries: its dtype among `dtypes`, on the device of `like`, unit stride along a row and a
    row stride of at least N, aligned to its element -> the row stride as the entry takes it"""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what} must be a tensor of shape {tuple(shape)}, got {getattr(t, 'shape', type(t))}")
    if t.dtype not in dtypes:
        raise RuntimeError(f"{what} must be of {' / '.join(str(d) for d in dtypes)}, got {t.dtype}")
    if like is not None and t.device != like.device:
        raise RuntimeError(f"{what} must be on {like.device}, got {t.device}")
    M, N = shape
    if M == 0:
        return N
    if N > 1 and t.stride(1) != 1:
        raise RuntimeError(f"{what} must have a unit stride along its rows, got strides {t.stride()}")
    if M > 1 and t.stride(0) < N:
        raise RuntimeError(f"{what} must have a row stride of at least {N}, got strides {t.stride()}")
    if t.data_ptr() % t.element_size():
        raise RuntimeError(f"{what} is not aligned to its element")
    return t.stride(0) if M > 1 else N


def _add_norm_vector(t, N: int, like, what: str, optional: bool = False):
    """weight / bias / mean / rstd: fp32, contiguous, of N elements, on the device of `like`"""
    if t is None and optional:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != (N,) or t.device != like.device \
            or not t.is_contiguous():
        raise RuntimeError(f"{what} must be a contiguous fp32 tensor of {N} elements on {like.device}, "
                           f"got {getattr(t, 'shape', type(t))} {getattr(t, 'dtype', '')} {getattr(t, 'device', '')}")
    return t


def _add_norm_shape(x, what: str):
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise RuntimeError(f"{what}: a 2-D tensor (rows, cols) is required, got {getattr(x, 'shape', type(x))}")
    M, N = int(x.shape[0]), int(x.shape[1])
    if not 1 <= N <= L.ADD_NORM_MAX_COLS:
        raise RuntimeError(f"{what}: 1 .. {L.ADD_NORM_MAX_COLS} columns are supported, got {N}")
    if M >= 1 << 31:
        raise RuntimeError(f"{what}: fewer than 2^31 rows are supported, got {M}")
    return M, N


def add_norm_fwd(lib: L.SegmLib, x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
                 residual: Optional[torch.Tensor] = None, eps: float = 1e-6, rms: bool = False, residual_dtype=None):
    """s = x + residual in fp32; y = LayerNorm(s) or RMSNorm(s) with weight / bias, in x's dtype -> (y, mean, rstd, residual_out).
    x (M, N <= 8192) fp32 / fp16 / bf16 and residual (M, N) of x's dtype or fp32: unit stride along a row, any row stride >= N.
    weight, bias: fp32 (N,).  residual_out = s rounded to the residual's dtype is written when there is a residual, or when
    `residual_dtype` (x's dtype or fp32) differs from x's dtype; None otherwise (the row saved for the backward is then x).
    mean (None for rms) and rstd: fp32 (M,).  The statistics come from the unrounded s (reference layernorm.py:65-120)."""
    what = "add_norm_fwd"
    M, N = _add_norm_shape(x, what)
    sx = _add_norm_rows(x, (M, N), tuple(L._DTYPES), None, f"{what}: x")
    weight = _add_norm_vector(weight, N, x, f"{what}: weight")
    bias = _add_norm_vector(bias, N, x, f"{what}: bias", optional=True)
    res_choices = (x.dtype, torch.float32)
    sres = 0
    if residual is not None:
        sres = _add_norm_rows(residual, (M, N), res_choices, x, f"{what}: residual")
        residual_dtype = residual.dtype
    elif residual_dtype is not None and residual_dtype not in res_choices:
        raise RuntimeError(f"{what}: residual_dtype must be {x.dtype} or torch.float32, got {residual_dtype}")
    y = torch.empty((M, N), dtype=x.dtype, device=x.device)
    residual_out = None
    if residual is not None or (residual_dtype is not None and residual_dtype != x.dtype):
        residual_out = torch.empty((M, N), dtype=residual_dtype, device=x.device)
    mean = None if rms else torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device)
    if M == 0:
        return y, mean, rstd, residual_out
    a = L.AddNormArgs()
    a.rows, a.cols, a.dtype, a.rms, a.eps = M, N, L.dtype_code(x), int(bool(rms)), float(eps)
    a.res_dtype = L._DTYPES[residual_dtype] if residual_dtype is not None else a.dtype
    a.x, a.x_stride, a.y, a.y_stride = x.data_ptr(), sx, y.data_ptr(), N
    if residual is not None:
        a.residual, a.residual_stride = residual.data_ptr(), sres
    if residual_out is not None:
        a.residual_out, a.residual_out_stride = residual_out.data_ptr(), N
    a.weight, a.bias, a.mean, a.rstd = weight.data_ptr(), L.fptr(bias), L.fptr(mean), rstd.data_ptr()
    a.stream = L.stream_handle(x)
    lib.check(lib.dll.segm_add_norm_fwd(a), what)
    return y, mean, rstd, residual_out


def add_norm_bwd(lib: L.SegmLib, dy: torch.Tensor, x_saved: torch.Tensor, weight: torch.Tensor, mean: Optional[torch.Tensor],
                 rstd: torch.Tensor, dresidual: Optional[torch.Tensor] = None, has_residual: bool = False, has_bias: bool = False,
                 rms: bool = False):
    """The backward of `add_norm_fwd` -> (dx, dweight, dbias, dresidual_in).  dy (M, N) in x's dtype; x_saved (M, N) what the
    forward kept: residual_out where it wrote one (x's dtype or fp32), x otherwise; mean (None for rms), rstd fp32 (M,);
    dresidual (M, N) of x_saved's dtype: the gradient that reached residual_out, added to dx.  dx has dy's dtype; dweight and dbias
    (None without `has_bias`) are fp32 (N,).  dresidual_in, the gradient of the residual, is None without `has_residual`, dx itself
    where the residual has x's dtype, and dx before its rounding, in fp32, otherwise (reference layernorm.py:293-377)."""
    what = "add_norm_bwd"
    M, N = _add_norm_shape(dy, what)
    sdy = _add_norm_rows(dy, (M, N), tuple(L._DTYPES), None, f"{what}: dy")
    ssaved = _add_norm_rows(x_saved, (M, N), (dy.dtype, torch.float32), dy, f"{what}: x_saved")
    weight = _add_norm_vector(weight, N, dy, f"{what}: weight")
    if not rms:
        mean = _add_norm_vector(mean, M, dy, f"{what}: mean")
    rstd = _add_norm_vector(rstd, M, dy, f"{what}: rstd")
    sdres = 0
    if dresidual is not None:
        sdres = _add_norm_rows(dresidual, (M, N), (x_saved.dtype,), dy, f"{what}: dresidual")
    dx = torch.empty((M, N), dtype=dy.dtype, device=dy.device)
    dweight = torch.empty((N,), dtype=torch.float32, device=dy.device)
    dbias = torch.empty((N,), dtype=torch.float32, device=dy.device) if has_bias else None
    wide = x_saved.dtype != dy.dtype
    dresidual_in = torch.empty((M, N), dtype=x_saved.dtype, device=dy.device) if has_residual and wide else None
    if M == 0:
        dweight.zero_()
        if dbias is not None:
            dbias.zero_()
        return dx, dweight, dbias, (dresidual_in if wide else dx) if has_residual else None
    a = L.AddNormArgs()
    a.rows, a.cols, a.dtype, a.res_dtype, a.rms = M, N, L.dtype_code(dy), L.dtype_code(x_saved), int(bool(rms))
    if wide:
        a.residual_out, a.residual_out_stride = x_saved.data_ptr(), ssaved
    else:
        a.x, a.x_stride = x_saved.data_ptr(), ssaved
    a.dy, a.dy_stride, a.dx, a.dx_stride = dy.data_ptr(), sdy, dx.data_ptr(), N
    if dresidual is not None:
        a.dresidual, a.dresidual_stride = dresidual.data_ptr(), sdres
    if dresidual_in is not None:
        a.dresidual_in, a.dresidual_in_stride = dresidual_in.data_ptr(), N
    a.weight, a.mean, a.rstd = weight.data_ptr(), L.fptr(None if rms else mean), rstd.data_ptr()
    a.dweight, a.dbias = dweight.data_ptr(), L.fptr(dbias)
    nbytes = lib.dll.segm_add_norm_workspace_bytes(M, N)
    if nbytes == 0:
        raise RuntimeError(f"{what}: the shape {(M, N)} is out of range")
    workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=dy.device)
    a.workspace, a.workspace_bytes = workspace.data_ptr(), nbytes
    a.stream = L.stream_handle(dy)
    lib.check(lib.dll.segm_add_norm_bwd(a), what)
    return dx, dweight, dbias, (dresidual_in if wide else dx) if has_residual else None


# ---------------------------------------------------------------------------------------------------------
# device guard
# ---------------------------------------------------------------------------------------------------------
# The reference's native ops run under a CUDAGuard on their first tensor's device (selective_scan.cpp:326-327,
# causal_conv1d.cpp:178-179): a kernel launch goes to the CURRENT device, whatever device the pointers and the stream
# belong to.  Every launching wrapper above therefore runs with the device of its first CUDA tensor current (a model on
# cuda:1 while the process's current device is cuda:0 must work); nothing happens - one integer compare - when it already is.
def _first_cuda_tensor(args):
    """the first CUDA tensor among the arguments, looking into lists / tuples and into the keyword dicts of the `*_multi` calls"""
    for a in args:
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                return a
        elif isinstance(a, dict):
            t = _first_cuda_tensor(a.values())
            if t is not None:
                return t
        elif isinstance(a, (list, tuple)) and a:
            t = _first_cuda_tensor(a)
            if t is not None:
                return t
    return None


def _device_guard(fn):
    import functools

    @functools.wraps(fn)
    def guarded(lib, *args, **kw):
        t = _first_cuda_tensor(args)
        if t is None:
            t = _first_cuda_tensor(kw.values())
        if t is not None and t.device.index != torch.cuda.current_device():
            with torch.cuda.device(t.device):
                return fn(lib, *args, **kw)
        return fn(lib, *args, **kw)
    return guarded


for _name in ("scan_fwd", "scan_bwd", "conv1d_fwd", "conv1d_bwd", "conv3d_k3_wgrad", "conv3d_k3_fwd", "instnorm_fwd",
              "instnorm_bwd", "instnorm_tail_bwd", "transpose_add", "layernorm_tokens_fwd", "layernorm_tokens_bwd", "sgd_clip_step", "cross_entropy",
              "conv1d_update", "state_update", "linear_rows", "skinny_tn", "pointwise_cf", "stem_conv_fwd", "stem_conv_wgrad", "wgrad_gemm",
              "scan_fwd_multi", "scan_bwd_multi", "conv1d_fwd_multi", "conv1d_bwd_multi", "channel_sum", "depth_to_space2",
              "space_to_depth2", "seg_regions", "edt_sq", "edt_sq_long", "planes_bbox", "border_distances", "border_stats", "sdm_masks", "sdm_compose", "resample_argmax", "ccl_roots", "ccl_sizes", "ccl_select",
              "nonzero_mask_bbox", "crop_stats", "crop_normalize", "zoom", "zoom_labels", "zoom_slices", "zoom_labels_slices", "spline_coefs", "affine_spline3", "affine_labels",
              "zoom_nearest", "gauss_blur", "intensity_stats", "intensity_apply", "window_gather", "window_count", "window_blend",
              "window_finish", "add_norm_fwd", "add_norm_bwd"):
    globals()[_name] = _device_guard(globals()[_name])
