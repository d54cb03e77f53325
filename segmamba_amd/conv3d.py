"""Dense 3x3x3 (stride 1, "same") convolutions of the SegMamba stem: forward, data gradient and weight gradient, each routed
by one table of the shape to one of the library's own MFMA kernels or to the vendor (MIOpen) call.

Every call is mathematically the same convolution, whichever route it takes:

  fwd    y  = conv(x, W)                      F.conv3d
                                              or  segm_conv3d_k3_fwd, the row kernels, per 48-channel input block (csrc/conv3d_fwd.hip)
                                              or  segm_conv3d_k3_cube_fwd, the whole contraction in one launch (csrc/conv3d_cube.hip)
  dgrad  dx = conv_bwd_data(dy, W)            the vendor call, or the same two forward kernels on dy with flip(W)^T
  wgrad  dW = conv_bwd_weight(x, dy)          the vendor call, segm_conv3d_k3_wgrad ("mfma") or segm_conv3d_k3_cube_wgrad

A call lists the variants that apply to its operands (`_fwd_variants`, `_wgrad_variants`: the vendor route first), `_route` picks
one of them through `_table_choice`, and `_run_fwd` / `_run_wgrad` launch it.  The choice is a pure function of the shape, so every
rank, every run and every captured graph takes the same kernels.  Why MIOpen does not serve these shapes, and the timing runs the
table was frozen from: docs/history/, profiles/r01_probe_convs.log, r02_bench_variants.log, r03_conv_tuner_vs_table.log.
"""
from __future__ import annotations

import os
from typing import List, Tuple

import torch
import torch.nn.functional as F

from . import linear

_BLOCK = 48                      # channel block of the library's kernels (and of MIOpen's fast 3-D bf16 solvers)
# cat(up, skip) convolutions as one autograd node with the later parts added in place (_ConvSameCat, linear._PointwiseCat): with the
# statistics epilogue the cat layers feed their InstanceNorm too (profiles/r05_inorm_epilogue_step.log).  SEGM_CONV_CAT_FUSED=0: one
# node per part.
_CAT_FUSED = os.environ.get("SEGM_CONV_CAT_FUSED", "1") == "1"
# the chained row kernels and the cube kernel store K part sums {count, y, y^2} of what they write; the InstanceNorm behind the
# convolution merges those partials instead of reading the volume again (csrc/conv3d_fwd.hip STATS; free on the convolution side,
# profiles/r05_inorm_epilogue.log).  SEGM_CONV_STATS=0: every InstanceNorm makes its own statistics pass (A/B).
_STATS = os.environ.get("SEGM_CONV_STATS", "1") == "1"
# conv1 + the 1x1x1 projection of a residual block's input as one node (_ResFront): the two data gradients of the input are summed
# by the 3x3x3 kernel's accumulate mode instead of an element-wise add.  SEGM_RES_FRONT=0: two nodes (A/B).
_RES_FRONT = os.environ.get("SEGM_RES_FRONT", "1") == "1"
# the wide layers of the 8^3 / 16^3 / 32^3 levels on segm_conv3d_k3_cube_fwd - forward and data gradient; 2.5 - 6x over the row
# kernels / the vendor route there (profiles/r06_conv_cube_v2.txt).  SEGM_CONV_CUBE=0: row kernels and the vendor route only.
_CUBE = os.environ.get("SEGM_CONV_CUBE", "1") == "1"
_CUBE_MAX_WIDTH = int(os.environ.get("SEGM_CONV_CUBE_MAX_WIDTH", "32"))
# ... and the weight gradients of the 8^3 level and of the 384-channel layers at 16^3 on segm_conv3d_k3_cube_wgrad (dY cube and X halo
# cube in LDS, a wave = a 16 x 16 (co, ci) tile x 27 taps): 2.1 - 2.6x over the vendor route at 8^3, 1.7 - 1.8x over the row kernel at
# 384 -> 384 @16^3; behind it below 384 channels and at 32^3 (profiles/r06_conv_cube_wgrad_v5.txt)
_CUBE_WGRAD = os.environ.get("SEGM_CONV_CUBE_WGRAD", "1") == "1"
_CUBE_WGRAD_MAX_WIDTH = int(os.environ.get("SEGM_CONV_CUBE_WGRAD_MAX_WIDTH", "16"))


def _table_variant(width: int):
    """the library forward kernel's (chain, pitch48, chain32) flags for a volume of this width (profiles/r02_bench_variants.log,
    r02_conv_stride_pad.log, r04_conv_chain_final.log): chained K parts everywhere; 64-wide blocks with unpadded LDS rows at 128^3;
    the 32-wide-block variant (two workgroups per CU) for 64^3 and below - since round 4, when its storing wave stopped staging
    the halo columns, it is level at 48 -> 48 @64^3 (0.074 ms both) and ahead at 96 -> 96 @64^3 (0.315 vs 0.334 ms)"""
    return (True, True, False) if width >= 128 else (False, False, True)


def _is_lib(v) -> bool:
    """a routing variant that is a library kernel: the row kernels' flag tuple, or "cube" """
    return isinstance(v, tuple) or v == "cube"


def _table_choice(kind: str, width: int, variants) -> int:
    """index of the routing the table prescribes among `variants` (None = a vendor route, tuple = library kernel flags, "mfma" =
    the library's weight-gradient kernel).  Measured on MI355X (profiles/r02_bench_variants.log): the library's kernels win every
    3x3x3 layer of width >= 16 - forward, data gradient (as a forward convolution with flipped, transposed weights) and weight
    gradient; the 8^3 bottleneck layers (768 / 384 channels, 0.1 ms each) stay on the vendor GEMM route, where they are
    weight-bandwidth-bound GEMMs."""
    if kind == "wgrad":
        if "cube" in variants:                           # only offered where it is the table's choice (_wgrad)
            return variants.index("cube")
        return variants.index("mfma") if width >= 16 and "mfma" in variants else 0
    if "cube" in variants:                               # only offered where it is the table's choice (_cube_ok)
        return variants.index("cube")
    if width >= 16:
        want = _table_variant(width)
        if want in variants:
            return variants.index(want)
        lib_routes = [i for i, v in enumerate(variants) if isinstance(v, tuple)]
        if lib_routes:
            return lib_routes[0]
    return 0


def _route(kind: str, width: int, variants):
    """the variant this call takes: the table's choice among `variants`; the vendor route where nothing else applies or there is
    no device.  The one place a route is decided (tests force a route by replacing this function)."""
    if len(variants) == 1 or not torch.cuda.is_available():
        return variants[0]
    return variants[_table_choice(kind, width, variants)]


def _blocks(c: int) -> List[slice]:
    return [slice(i, min(i + _BLOCK, c)) for i in range(0, c, _BLOCK)]


def _hip_fwd_ok(x, w) -> bool:
    from . import ops_raw
    return w.shape[2:] == (3, 3, 3) and (w.shape[1] % _BLOCK == 0 or w.shape[1] < _BLOCK) and w.shape[0] % 16 == 0 \
        and x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and \
        ops_raw.conv3d_k3_fwd_supported(x[:, :_BLOCK], w.shape[0])


def _packed_block(w, ib, flipped, dtype):
    """the library kernel's register layout of one 48-channel input block of a weight: (Cout, 3, 3, 3, 48) in the activations'
    dtype; `flipped`: the block of the data-gradient weight flip(W)^T.  A re-arrangement of the step's 16-bit copy: inside a
    bank step it is a view of the bank's gather buffer (param_bank.packed), not a per-call copy chain."""
    from . import ops_raw
    from .param_bank import packed
    if w.dtype != dtype:
        return ops_raw.pack_conv3d_weight((w.flip(2, 3, 4).transpose(0, 1) if flipped else w)[:, ib], dtype)
    if flipped:
        return packed(w, ("conv3d_k3_dgrad", ib.start, ib.stop),
                      lambda t: ops_raw.pack_conv3d_weight(t.flip(2, 3, 4).transpose(0, 1)[:, ib], t.dtype))
    return packed(w, ("conv3d_k3_fwd", ib.start, ib.stop), lambda t: ops_raw.pack_conv3d_weight(t[:, ib], t.dtype))


def _fwd_hip(x, w, pad, bias=None, chain=False, pitch48=False, chain32=False, into=None, flipped=False, stats_box=None):
    """segm_conv3d_k3_fwd per 48-channel input block (the kernel keeps one block's weights in registers).  With
    Cout % 48 == 0 the later blocks accumulate into the first block's output in place; `chain` picks the kernel whose K
    parts are pipelined (csrc/conv3d_fwd.hip, variant 1).  `into`: an existing result every block is added to (the next part
    of a concatenated input; Cout % 48 == 0, no bias).  `stats_box` (a list): the LAST block's launch - the one that stores the
    finished values - also sums the InstanceNorm statistics of the result and appends the partials (kernels with that epilogue only)."""
    from . import lib as L, ops_raw
    hip = L.get_lib()
    cout, cin = (w.shape[1], w.shape[0]) if flipped else (w.shape[0], w.shape[1])     # flipped: w is the forward weight
    inplace = cout % _BLOCK == 0
    out = into
    blocks = _blocks(cin)
    for i, ib in enumerate(blocks):
        wp = _packed_block(w, ib, flipped, x.dtype)
        if inplace:
            last = stats_box is not None and i + 1 == len(blocks) and ((chain and pitch48) or chain32)
            out = ops_raw.conv3d_k3_fwd(hip, x[:, ib], wp, bias if i == 0 else None, out=out, accumulate=i > 0 or into is not None,
                                        chain=chain, pitch48=pitch48, chain32=chain32, want_stats=last)
            if last:
                out, st = out
                if st is not None:
                    stats_box.append(st)
        else:
            y = ops_raw.conv3d_k3_fwd(hip, x[:, ib], wp, bias if i == 0 else None)
            out = y if out is None else out + y
    return out


def _cube_ok(x, cout: int, cin_w: int) -> bool:
    """the cube kernel takes this convolution AND the table prefers it: every supported layer of width <= 16, at 32^3 the layers from
    96 -> 192 channels up (96 -> 96 is level with the row kernel, which also carries the statistics epilogue)"""
    from . import ops_raw
    if not _CUBE or not ops_raw.conv3d_cube_supported(x, cout) or x.shape[1] != cin_w:
        return False
    width = x.shape[4]
    return width <= min(16, _CUBE_MAX_WIDTH) or (width <= _CUBE_MAX_WIDTH and width <= 32 and x.shape[1] * cout >= 96 * 192)


def _fwd_cube(x, w, bias=None, into=None, flipped=False, stats_box=None):
    """segm_conv3d_k3_cube_fwd: the whole contraction in one launch (+ its reduction); `flipped`: w is the forward weight and x
    the output gradient (the data gradient); `into`: an existing result the launch adds to; `stats_box`: the InstanceNorm partials of
    what the launch stores are appended"""
    from . import lib as L, ops_raw
    from .param_bank import packed_cube_image
    hip = L.get_lib()
    cout = w.shape[1] if flipped else w.shape[0]
    if w.dtype != x.dtype:
        img = ops_raw.conv3d_cube_weight_image(hip, w, flipped, x.dtype)
    else:                                                  # inside a bank step: one of the images the step's pack launch refreshes
        img = packed_cube_image(w, flipped, lambda t: ops_raw.conv3d_cube_weight_image(hip, t, flipped))
    res = ops_raw.conv3d_k3_cube_fwd(hip, x, img, cout, bias, out=into, accumulate=into is not None, want_stats=stats_box is not None)
    if stats_box is not None:
        res, st = res
        stats_box.append(st)
    return res


def _dgrad_native(dy, w, x, pad):
    return torch.ops.aten.convolution_backward(dy, x, w, None,
                                                [1, 1, 1], [pad] * 3, [1, 1, 1], False, [0, 0, 0], 1,
                                                [True, False, False])[0]


def _dgrad_hip(dy, w, x, pad, chain=False, pitch48=False, chain32=False, into=None):
    return _fwd_hip(dy, w, pad, None, chain, pitch48, chain32, into=into, flipped=True)


def _wgrad_native(x, dy, w, pad):
    return torch.ops.aten.convolution_backward(dy, x, w, None,
                                                [1, 1, 1], [pad] * 3, [1, 1, 1], False, [0, 0, 0], 1,
                                                [False, True, False])[1]


def _wgrad_mfma(x, dy, w, pad, out_dtype=None):
    """segm_conv3d_k3_wgrad: the hand-written MFMA weight-gradient kernel (csrc/conv3d_wgrad.hip); the result in the dtype
    of the master weight (fp32 under autocast: the kernel's accumulators, not rounded)."""
    from . import lib as L, ops_raw
    if not ops_raw.conv3d_k3_wgrad_supported(x, dy):
        x = x.contiguous()                       # e.g. the permuted (channel-last) outputs of the Mamba encoder
    return ops_raw.conv3d_k3_wgrad(L.get_lib(), x, dy, out_dtype or w.dtype)


def _cube_wgrad_ok(x, dy, w) -> bool:
    """segm_conv3d_k3_cube_wgrad takes the layer AND the table prefers it (8^3: every wide layer; 16^3: from 384 x 384 channels)"""
    from . import ops_raw
    if not _CUBE_WGRAD or w.shape[2:] != (3, 3, 3) or not ops_raw.conv3d_cube_wgrad_supported(x, dy):
        return False
    width, prod = x.shape[4], x.shape[1] * dy.shape[1]
    return width <= _CUBE_WGRAD_MAX_WIDTH and ((width <= 8 and prod >= 96 * 192) or (width <= 16 and prod >= 384 * 384))


def _wgrad_cube(x, dy, out_dtype):
    from . import lib as L, ops_raw
    return ops_raw.conv3d_k3_cube_wgrad(L.get_lib(), x, dy, out_dtype if out_dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32)


def _mfma_wgrad_ok(x, dy, w) -> bool:
    from . import ops_raw
    if w.shape[2:] != (3, 3, 3) or w.dtype not in (torch.bfloat16, torch.float16, torch.float32) or \
            x.dtype not in (torch.bfloat16, torch.float16):
        return False
    return (x.shape[1] % 48 == 0 or x.shape[1] < 48) and dy.shape[1] % 48 == 0 and x.shape[4] % 8 == 0 and \
        x.shape[0] == dy.shape[0] and ops_raw.conv3d_k3_wgrad_spans_fit(x, dy)


_HIP_VARIANTS = ((False, False, False), (True, False, False), (True, True, False), (False, False, True))   # (chain, pitch48, chain32)


def _fwd_variants(x, w, flipped=False) -> list:
    """the routes that apply to the forward convolution of x with w, the table's preference aside: None (the vendor call), the row
    kernels' flag tuples (the chained ones need Cout % 48 == 0), "cube" where `_cube_ok`.  `flipped`: the data gradient - x is the
    output gradient, w the forward weight."""
    if flipped:
        w = w.transpose(0, 1)
    variants = [None]
    if _hip_fwd_ok(x, w):
        variants += _HIP_VARIANTS if w.shape[0] % _BLOCK == 0 else _HIP_VARIANTS[:1]
    if w.shape[2:] == (3, 3, 3) and w.dtype == x.dtype and _cube_ok(x, w.shape[0], w.shape[1]):
        variants.append("cube")
    return variants


def _wgrad_variants(x, dy, w) -> list:
    """the routes that apply to the weight gradient: None (the vendor call), "mfma", "cube" where `_cube_wgrad_ok`"""
    variants = [None]
    if _mfma_wgrad_ok(x, dy, w):
        variants.append("mfma")
    if _cube_wgrad_ok(x, dy, w):
        variants.append("cube")
    return variants


def _run_fwd(v, x, w, pad, bias=None, into=None, stats_box=None, flipped=False, like=None):
    """route `v` on one part of a convolution.  `into` (library kernels): an existing result the launch adds to; `stats_box`: see
    `_fwd_hip`; `flipped`: the data gradient - x is the output gradient, w the forward weight and `like` the convolution's input,
    whose shape the vendor call wants."""
    if v == "cube":
        return _fwd_cube(x, w, bias, into=into, flipped=flipped, stats_box=stats_box)
    if v is not None:
        return _fwd_hip(x, w, pad, bias, *v, into=into, flipped=flipped, stats_box=stats_box)
    assert into is None
    return _dgrad_native(x, w, like, pad) if flipped else F.conv3d(x, w, bias, 1, pad)


def _add_part(into, v, x, w, pad, stats_box=None, flipped=False, like=None):
    """into += the convolution `_run_fwd(v, x, w, ...)` computes (the next part of a concatenated input; a second gradient of the
    same tensor): by the library kernel's accumulate mode where it has one for this shape (Cout % 48 == 0) and `into` has dense
    channels (a vendor-route result or another consumer's gradient may not), by an ordinary add otherwise"""
    from . import ops_raw
    cout = w.shape[1] if flipped else w.shape[0]
    if _is_lib(v) and cout % _BLOCK == 0 and ops_raw.channel_dense(into):
        return _run_fwd(v, x, w, pad, into=into, stats_box=stats_box, flipped=flipped)
    return into.add_(_run_fwd(v, x, w, pad, flipped=flipped, like=like))


def _run_wgrad(v, x, dy, w, pad, w_dtype):
    if v == "cube":
        return _wgrad_cube(x, dy, w_dtype)
    if v == "mfma":
        return _wgrad_mfma(x, dy, w, pad, w_dtype)
    return _wgrad_native(x, dy, w, pad)


def _dgrad(dy, w, x, pad, into=None):
    """`into`: a gradient of x that already exists (another consumer's, owned by the caller) - the result is added to it"""
    v = _route("dgrad", dy.shape[4], _fwd_variants(dy, w, flipped=True))
    if into is not None:
        return _add_part(into, v, dy, w, pad, flipped=True, like=x)
    return _run_fwd(v, dy, w, pad, flipped=True, like=x)


def _wgrad(x, dy, w, pad, w_dtype):
    return _run_wgrad(_route("wgrad", x.shape[4], _wgrad_variants(x, dy, w)), x, dy, w, pad, w_dtype).to(w_dtype)


class _ConvSame(torch.autograd.Function):
    """stride-1 "same" convolution, odd kernel; x already in the compute dtype, w / bias in any dtype (fp32 masters under autocast)."""

    @staticmethod
    def forward(ctx, x, w, bias, want_stats=False):
        from .linear import _masters
        w, bias = _masters(ctx, x, w, bias)              # fp32 masters -> the step's 16-bit copies; gradients go back in fp32
        ctx.save_for_backward(x, w)
        box = [] if want_stats else None
        out = _run_fwd(_route("fwd", x.shape[4], _fwd_variants(x, w)), x, w, w.shape[2] // 2, bias, stats_box=box)
        ctx.with_stats = bool(want_stats)
        if not want_stats:
            return out
        stats = box[-1] if box else out.new_empty(0, dtype=torch.float32)      # a launch without the epilogue leaves the box empty
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dy, *_):
        x, w = ctx.saved_tensors
        pad = w.shape[2] // 2
        from . import ops_raw
        if not ops_raw.channel_dense(dy):                # the kernels take strides; a padded channel stride is not copied
            dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dy, w, x, pad)
        if ctx.needs_input_grad[1]:
            dw = _wgrad(x, dy, w, pad, ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = linear.bias_grad(dy).to(ctx.b_dtype)
        return dx, dw, db, None


class _ConvSameCat(torch.autograd.Function):
    """conv3d_same(cat(xs, 1), w) without the concatenation AND without the adds: the convolution is linear in its input
    channels; the first part is a plain convolution with w[:, :c0], every later part is added in place by the library kernel its
    shape routes to (`accumulate`) - or, where it routes to the vendor call, through an ordinary add (`_add_part`).  One node
    for the whole layer: the weight gradient is assembled by one cat instead of autograd's zero-fill + copy + add per slice."""

    @staticmethod
    def forward(ctx, want_stats, w, *xs):
        from .param_bank import low_precision
        ctx.w_dtype = w.dtype
        w = low_precision(w, xs[0].dtype)
        pad = w.shape[2] // 2
        ctx.save_for_backward(w, *xs)
        out, c0, stats = None, 0, None
        for j, x in enumerate(xs):
            wi = w[:, c0:c0 + x.shape[1]]
            c0 += x.shape[1]
            v = _route("fwd", x.shape[4], _fwd_variants(x, wi))
            if out is None:
                out = _run_fwd(v, x, wi, pad)
                continue
            box = [] if (want_stats and j + 1 == len(xs)) else None          # the launch that stores the finished values
            out = _add_part(out, v, x, wi, pad, stats_box=box)
            stats = box[-1] if box else None
        if not want_stats:
            return out
        stats = stats if stats is not None else out.new_empty(0, dtype=torch.float32)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, dy, *_):
        w, *xs = ctx.saved_tensors
        pad = w.shape[2] // 2
        from . import ops_raw
        if not ops_raw.channel_dense(dy):
            dy = dy.contiguous()
        dxs, dws, c0 = [], [], 0
        for i, x in enumerate(xs):
            wi = w[:, c0:c0 + x.shape[1]]
            c0 += x.shape[1]
            dxs.append(_dgrad(dy, wi, x, pad) if ctx.needs_input_grad[2 + i] else None)
            if ctx.needs_input_grad[1]:
                dws.append(_wgrad(x, dy, wi, pad, ctx.w_dtype))
        dw = torch.cat(dws, dim=1) if ctx.needs_input_grad[1] else None
        return (None, dw, *dxs)


class _ResFront(torch.autograd.Function):
    """The two convolutions a residual block with a projection skip applies to its input - conv1 (3x3x3) and conv3 (1x1x1),
    dynunet_block.py:93-104 of the reference - on cat(xs, 1), as ONE node: each part then has ONE data gradient, written by the
    1x1x1 kernel and added to in place by the 3x3x3 kernel, where two nodes leave autograd an element-wise add per part (three
    passes over a 128^3 volume each).  Forward arithmetic = _ConvSameCat + linear._PointwiseCat.  -> (y1, stats of y1 or an empty
    tensor, y3)."""

    @staticmethod
    def forward(ctx, want_stats, w1, w3, *xs):
        from .param_bank import low_precision
        ctx.w_dtypes = (w1.dtype, w3.dtype)
        dt = xs[0].dtype
        w1, w3 = low_precision(w1, dt), low_precision(w3, dt)
        pad = w1.shape[2] // 2
        ctx.save_for_backward(w1, w3, *xs)
        y1, y3, c0, stats = None, None, 0, None
        for j, x in enumerate(xs):
            c1 = c0 + x.shape[1]
            w1i, w3i, xf = w1[:, c0:c1], w3[:, c0:c1], x.flatten(2)
            c0 = c1
            box = [] if (want_stats and j + 1 == len(xs)) else None          # the launch that stores the finished values
            v = _route("fwd", x.shape[4], _fwd_variants(x, w1i))
            if y1 is None:
                y1 = _run_fwd(v, x, w1i, pad, stats_box=box)
                y3 = linear._pw_hip(w3i, xf, None)
                if y3 is None:
                    y3 = linear._bmm_w(w3i, xf)
            else:
                y1 = _add_part(y1, v, x, w1i, pad, stats_box=box)
                y = linear._pw_hip(w3i, xf, None, into=y3)
                y3 = y if y is not None else y3 + linear._bmm_w(w3i, xf)
            stats = box[-1] if box else None
        stats = stats if stats is not None else y1.new_empty(0, dtype=torch.float32)
        ctx.mark_non_differentiable(stats)
        return y1, stats, y3.view(y1.shape)

    @staticmethod
    def backward(ctx, dy1, _, dy3):
        w1, w3, *xs = ctx.saved_tensors
        pad = w1.shape[2] // 2
        from . import ops_raw
        if not ops_raw.channel_dense(dy1):
            dy1 = dy1.contiguous()
        dy3 = dy3.flatten(2) if ops_raw.channel_dense(dy3) else dy3.contiguous().flatten(2)
        dxs, dw1, dw3, c0 = [], [], [], 0
        for i, x in enumerate(xs):
            c1 = c0 + x.shape[1]
            w1i, w3i = w1[:, c0:c1], w3[:, c0:c1]
            c0 = c1
            dx = None
            if ctx.needs_input_grad[3 + i]:
                dx = linear._pw_hip(w3i.t(), dy3, None)
                if dx is None:
                    dx = linear._bmm_w(w3i.t(), dy3)
                dx = _dgrad(dy1, w1i, x, pad, into=dx.view(x.shape))
            dxs.append(dx)
            if ctx.needs_input_grad[1]:
                dw1.append(_wgrad(x, dy1, w1i, pad, ctx.w_dtypes[0]))
            if ctx.needs_input_grad[2]:
                dw3.append(linear.nt_matmul_rows(dy3, x.flatten(2)))
        g1 = torch.cat(dw1, dim=1) if ctx.needs_input_grad[1] else None
        g3 = torch.cat(dw3, dim=1).to(ctx.w_dtypes[1]) if ctx.needs_input_grad[2] else None
        return (None, g1, g3, *dxs)


def res_front(xs: Tuple[torch.Tensor, ...], w1: torch.Tensor, w3: torch.Tensor, want_stats: bool = False):
    """(conv3d_same(cat(xs, 1), w1), its InstanceNorm partials or None, the 1x1x1 convolution of cat(xs, 1) with w3) as one autograd
    node (_ResFront), or None when the parts are not the library kernels' (device, one 16-bit dtype, dense channels, more than 4
    input channels) - the caller then runs the two convolutions on their own."""
    from . import lib as L, ops_raw
    if not (_RES_FRONT and _CAT_FUSED and all(L.on_device(x) for x in xs) and w1.shape[2:] == (3, 3, 3) and w1.shape[1] > 4):
        return None
    if torch.is_autocast_enabled():
        dt = torch.get_autocast_dtype("cuda")
        xs = tuple(x.to(dt) for x in xs)
    if xs[0].dtype not in (torch.bfloat16, torch.float16) or any(x.dtype != xs[0].dtype or not ops_raw.channel_dense(x) for x in xs):
        return None
    y1, st, y3 = _ResFront.apply(bool(want_stats and _STATS), w1, w3.reshape(w3.shape[0], w3.shape[1]), *xs)
    return y1, (st if st.numel() else None), y3


def _unpack_stats(res):
    y, st = res
    return y, (st if st.numel() else None)


def conv3d_same(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None, want_stats: bool = False):
    """Conv3d(kernel k odd, stride 1, padding k//2).  Follows autocast like `F.conv3d` does.
    want_stats: -> (y, stats); stats = the InstanceNorm partials of y for fused_norm.instance_norm_act(y, ..., stats=stats) when the
    launch that produced y has the statistics epilogue, else None."""
    from . import lib as L
    if not L.on_device(x):
        y = F.conv3d(x, weight, bias, 1, weight.shape[2] // 2)
        return (y, None) if want_stats else y
    if torch.is_autocast_enabled():
        x = x.to(torch.get_autocast_dtype("cuda"))       # the weights stay masters: _ConvSame makes its own copies
    if want_stats and _STATS:
        return _unpack_stats(_ConvSame.apply(x, weight, bias, True))
    y = _ConvSame.apply(x, weight, bias)
    return (y, None) if want_stats else y


def conv3d_same_cat(xs: Tuple[torch.Tensor, ...], weight: torch.Tensor, want_stats: bool = False):
    """conv3d_same(torch.cat(xs, 1), weight) without materialising the concatenation: the convolution is linear in
    its input channels, so it is the sum of convolutions of the parts with the matching weight slices.  (The UNETR
    decoder convolves cat(upsampled, skip), unetr_block.py:82-84; MIOpen's 96 -> 48 @128^3 solver is the 600 ms one.)"""
    from . import lib as L
    if _CAT_FUSED and len(xs) > 1 and all(L.on_device(x) for x in xs):
        if torch.is_autocast_enabled():
            dt = torch.get_autocast_dtype("cuda")
            xs = tuple(x.to(dt) for x in xs)
        if all(x.dtype == xs[0].dtype for x in xs):
            if want_stats and _STATS:
                return _unpack_stats(_ConvSameCat.apply(True, weight, *xs))
            y = _ConvSameCat.apply(False, weight, *xs)
            return (y, None) if want_stats else y
    out, c0 = None, 0
    for x in xs:
        c = x.shape[1]
        y = conv3d_same(x, weight[:, c0:c0 + c])
        out = y if out is None else out + y
        c0 += c
    return (out, None) if want_stats else out
