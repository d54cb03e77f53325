"""The residual tail y = act(IN(out2) + IN(skip)) in one apply pass per direction (csrc/instnorm.hip: segm_instnorm_stats,
segm_instnorm_tail_fwd, segm_instnorm_tail_bwd), shared by tests/test_emu_norm_tail.py (kernel sources on the CPU emulator) and
tests/test_gpu_norm_tail.py (the HIP library).

The oracle is the two-call sequence ON THE SAME LIBRARY: instnorm_fwd(skip, act none) -> residual, instnorm_fwd(out2, residual, act),
and their two backwards with the residual's gradient wanted.  The tail must give the same BITS: torch.equal on y, both mean / rstd
pairs, dx and dskip - no tolerance, no element left out.  How a pass streams is forced by the caller through SEGM_NORM_NT."""
import torch

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from tests import norm_checks as K

SLOPE, EPS = K.SLOPE, K.EPS
ACTS = ("leaky_relu", "relu")
NAMES = ("y", "mean", "rstd", "skip_mean", "skip_rstd", "dx", "dskip")


def inputs(dev, shape, dtype, r, seed=K.DRAW):
    """-> out2, skip, dy: the draws of norm_checks.inputs, the skip with a mean and a spread of its own"""
    x, s, dy = K.inputs("cpu", shape, dtype, r, seed)
    skip = (0.7 * s.float() - 0.4 * r).to(dtype)
    return x.to(dev), skip.to(dev), dy.to(dev)


def two_calls(lib, x, skip, dy, act, stats=None):
    """the oracle -> (y, mean, rstd, skip_mean, skip_rstd, dx, dskip)"""
    res, m3, r3 = ops_raw.instnorm_fwd(lib, skip, None, "none", SLOPE, EPS)
    y, m2, r2 = ops_raw.instnorm_fwd(lib, x, res, act, SLOPE, EPS, stats=stats)
    dx, dres = ops_raw.instnorm_bwd(lib, x, dy, m2, r2, y, act, SLOPE, want_dresidual=True)
    dskip, none = ops_raw.instnorm_bwd(lib, skip, dres, m3, r3, None, "none", SLOPE)
    assert none is None
    return y, m2, r2, m3, r3, dx, dskip


def tail(lib, x, skip, dy, act, stats=None):
    h = ops_raw.instnorm_fwd(lib, skip, stats_only=True)
    assert isinstance(h, ops_raw.NormStats) and h.mean.numel() == x.shape[0] * x.shape[1]
    y, m2, r2 = ops_raw.instnorm_fwd(lib, x, None, act, SLOPE, EPS, stats=stats, skip=skip, skip_stats=h)
    dx, dskip = ops_raw.instnorm_tail_bwd(lib, x, skip, dy, m2, r2, h.mean, h.rstd, y, act, SLOPE)
    return y, m2, r2, h.mean, h.rstd, dx, dskip


def same_bits(got, want, what):
    for n, a, b in zip(NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, n)
        assert bool(torch.isfinite(b.float()).all()), (what, n, "the oracle is not finite")
        ok = torch.equal(a, b)
        K.log(f"{what} {n}", 0.0 if ok else float("inf"), 0.0)
        assert ok, (what, n, "differs at", int((a != b).sum()), "of", a.numel())


def check_shape(lib, dev, shape, dtype, offsets=(3.0,)):
    """(a) tail against the two calls, both activations"""
    for r in offsets:
        x, skip, dy = inputs(dev, shape, dtype, r)
        for act in ACTS:
            what = f"tail (a) mode {K.mode_name()} {K.name(dtype)} {shape} {act} r={r}"
            same_bits(tail(lib, x, skip, dy, act), two_calls(lib, x, skip, dy, act), what)


# ---- (b) padded and unequal instance strides -----------------------------------------------------------------------------------
def _ws(lib, x, tail_bwd=False):
    inst = x.shape[0] * x.shape[1]
    fn = lib.dll.segm_instnorm_tail_workspace_bytes if tail_bwd else lib.dll.segm_instnorm_workspace_bytes
    n = fn(inst, x.numel() // inst)
    return torch.empty(n, dtype=torch.uint8, device=x.device), n


def tail_into(lib, x, skip, dy, y, dx, dskip, act):
    """the three entry points on tensors of the caller's, each with its own instance stride -> (mean, rstd, skip_mean, skip_rstd)"""
    inst = x.shape[0] * x.shape[1]
    S = x.numel() // inst
    st = ops_raw.instance_stride
    part, n = _ws(lib, x)
    a = L.InstNormStatsArgs()
    a.instances, a.dtype, a.spatial = inst, L.dtype_code(x), S
    a.x, a.x_instance_stride, a.partials, a.partials_bytes, a.stream = skip.data_ptr(), st(skip), part.data_ptr(), n, L.stream_handle(x)
    lib.check(lib.dll.segm_instnorm_stats(a), "instnorm_stats")
    mean, rstd, m3, r3 = (torch.empty(inst, dtype=torch.float32, device=x.device) for _ in range(4))
    ws, nws = _ws(lib, x)
    f = L.InstNormTailFwdArgs()
    f.instances, f.dtype, f.act, f.spatial, f.slope, f.eps = inst, L.dtype_code(x), ops_raw.ACT_CODES[act], S, SLOPE, EPS
    f.x, f.skip, f.y = x.data_ptr(), skip.data_ptr(), y.data_ptr()
    f.mean, f.rstd, f.skip_mean, f.skip_rstd = mean.data_ptr(), rstd.data_ptr(), m3.data_ptr(), r3.data_ptr()
    f.skip_partials, f.skip_partials_bytes = part.data_ptr(), n
    f.workspace, f.workspace_bytes, f.stream = ws.data_ptr(), nws, L.stream_handle(x)
    f.x_instance_stride, f.skip_instance_stride, f.y_instance_stride = st(x), st(skip), st(y)
    lib.check(lib.dll.segm_instnorm_tail_fwd(f), "instnorm_tail_fwd")
    ws, nws = _ws(lib, x, tail_bwd=True)
    b = L.InstNormTailBwdArgs()
    b.instances, b.dtype, b.act, b.spatial, b.slope = inst, L.dtype_code(x), ops_raw.ACT_CODES[act], S, SLOPE
    b.x, b.skip, b.dy, b.y = x.data_ptr(), skip.data_ptr(), dy.data_ptr(), y.data_ptr()
    b.mean, b.rstd, b.skip_mean, b.skip_rstd = mean.data_ptr(), rstd.data_ptr(), m3.data_ptr(), r3.data_ptr()
    b.dx, b.dskip = dx.data_ptr(), dskip.data_ptr()
    b.workspace, b.workspace_bytes, b.stream = ws.data_ptr(), nws, L.stream_handle(x)
    b.x_instance_stride, b.skip_instance_stride, b.dy_instance_stride = st(x), st(skip), st(dy)
    b.y_instance_stride, b.dx_instance_stride, b.dskip_instance_stride = st(y), st(dx), st(dskip)
    lib.check(lib.dll.segm_instnorm_tail_bwd(b), "instnorm_tail_bwd")
    return mean, rstd, m3, r3


PADDED_CASES = (
    # shape, dtype, act, paddings of (out2, skip, y, dy, dx, dskip): multiples of 8 keep the vector path, odd ones take the scalar path
    ((2, 3, 4, 8, 16), torch.bfloat16, "leaky_relu", (192, 64, 8, 64, 8, 192)),
    ((1, 2, 18, 32, 48), torch.float16, "relu", (8, 192, 64, 192, 64, 8)),
    ((1, 2, 40, 40, 41), torch.float32, "leaky_relu", (64, 8, 192, 8, 192, 64)),
    ((2, 2, 3, 5, 7), torch.float32, "leaky_relu", (3, 5, 3, 5, 3, 5)),
    ((1, 2, 3, 5, 7), torch.bfloat16, "relu", (3, 8, 5, 64, 192, 5)),
)


def check_padded(lib, dev):
    """(b) every operand with its own padded instance stride, the skip's different from out2's: the bits of the dense two-call
    sequence, the padding of the inputs (NaN) never read, that of the outputs (a sentinel) never written"""
    nan = float("nan")
    for shape, dtype, act, (px, ps, py, pdy, pdx, pds) in PADDED_CASES:
        assert px != ps
        what = f"tail (b) mode {K.mode_name()} {K.name(dtype)} {shape} {act}"
        x, skip, dy = inputs(dev, shape, dtype, 3.0, seed=1)
        want = two_calls(lib, x, skip, dy, act)
        S = x[0, 0].numel()
        xp, sp, dyp = K.padded(x, px, nan)[1], K.padded(skip, ps, nan)[1], K.padded(dy, pdy, nan)[1]
        bufs = [K.padded(shape, p, K.SENTINEL, dtype, dev) for p in (py, pdx, pds)]
        (ybuf, yp), (dxbuf, dxp), (dsbuf, dsp) = bufs
        stats = tail_into(lib, xp, sp, dyp, yp, dxp, dsp, act)
        same_bits((yp,) + tuple(stats) + (dxp, dsp), want, what)
        fill = torch.full((), K.SENTINEL, dtype=dtype, device=dev)
        for buf, _ in bufs:
            assert bool((buf[:, :, S:] == fill).all()), (what, "padding written")


# ---- (c) statistics of out2 summed by its producer -----------------------------------------------------------------------------
def check_producer_stats(lib, dev, nparts):
    """(c) the partials of norm_checks.check_producer_stats for out2, handed to both forms"""
    shape = (1, 3, 8, 32, 48)
    for dtype in (torch.float32, torch.bfloat16):
        g = torch.Generator().manual_seed(nparts)
        x, skip, dy = inputs("cpu", shape, dtype, 3.0, seed=2)
        S = x[0, 0].numel()
        counts = torch.stack([K.unequal_counts(S, nparts, g) for _ in range(3)])
        st = K.producer_partials(K.flat(x), counts).reshape(1, 3, nparts, 4).to(dev)
        x, skip, dy = x.to(dev), skip.to(dev), dy.to(dev)
        what = f"tail (c) {K.name(dtype)} nparts={nparts}"
        got = tail(lib, x, skip, dy, "leaky_relu", stats=st)
        same_bits(got, two_calls(lib, x, skip, dy, "leaky_relu", stats=st), what)
        own = two_calls(lib, x, skip, dy, "leaky_relu")
        assert torch.equal(got[3], own[3]) and torch.equal(got[4], own[4]), (what, "the skip's statistics are its own pass's")


# ---- (e) determinism -----------------------------------------------------------------------------------------------------------
def check_determinism(lib, dev):
    for shape, dtype in (((1, 2, 18, 32, 48), torch.bfloat16), ((1, 2, 40, 40, 41), torch.float32), ((1, 2, 3, 5, 7), torch.float16)):
        x, skip, dy = inputs(dev, shape, dtype, 3.0, seed=3)
        same_bits(tail(lib, x, skip, dy, "leaky_relu"), tail(lib, x, skip, dy, "leaky_relu"),
                  f"tail (e) mode {K.mode_name()} {K.name(dtype)} {shape} two calls")


# ---- (d) a residual block through autograd, the route on and off ---------------------------------------------------------------
BLOCKS = (
    # (cin, cout), shapes of the inputs (a pair = their channel concatenation), dtype
    ((96, 48), ((1, 48, 2, 4, 64), (1, 48, 2, 4, 64))),
    ((4, 48), ((1, 4, 4, 8, 16),)),
)


def check_block(dev, monkeypatch, channels, shapes):
    """UnetResBlock forward + backward with SEGM_NORM_TAIL 0 and 1 (fused_norm._NORM_TAIL, read at import like the other route
    switches): output, input gradients and every parameter gradient bit-equal, and the tail really is one node"""
    from segmamba_amd import fused_norm, unet_blocks as UB
    torch.manual_seed(3)
    blk = UB.UnetResBlock(*channels).bfloat16().to(dev)
    g = torch.Generator().manual_seed(9)
    xs = [torch.randn(s, generator=g).bfloat16().to(dev) for s in shapes]
    dy = torch.randn((shapes[0][0], channels[1]) + shapes[0][2:], generator=g).bfloat16().to(dev)
    res = []
    for on in (False, True):
        monkeypatch.setattr(fused_norm, "_NORM_TAIL", on)
        ins = [x.clone().requires_grad_() for x in xs]
        blk.zero_grad()
        y = blk(tuple(ins) if len(ins) > 1 else ins[0])
        assert type(y.grad_fn).__name__.startswith("_InstNormTail" if on else "_InstNormAct"), type(y.grad_fn).__name__
        y.backward(dy)
        assert all(p.grad is not None for p in blk.parameters())
        res.append([y.detach().clone()] + [x.grad.clone() for x in ins] + [p.grad.clone() for p in blk.parameters()])
    for i, (u, v) in enumerate(zip(*res)):
        assert bool(torch.isfinite(u.float()).all())
        assert torch.equal(u, v), (channels, "tensor", i, "differs at", int((u != v).sum()), "of", u.numel())


def check_cpu_fallback():
    """CPU tensors: the ATen expression of the two instance_norm_act calls"""
    from segmamba_amd import fused_norm
    x, skip, dy = inputs("cpu", (2, 3, 4, 8, 16), torch.float32, 3.0)
    a, b = x.clone().requires_grad_(), skip.clone().requires_grad_()
    y = fused_norm.instance_norm_tail(a, b, "leaky_relu", SLOPE, EPS)
    ga, gb = torch.autograd.grad(y, (a, b), dy)
    a2, b2 = x.clone().requires_grad_(), skip.clone().requires_grad_()
    y2 = fused_norm.instance_norm_act(a2, "leaky_relu", SLOPE, EPS, residual=fused_norm.instance_norm_act(b2, "none", eps=EPS))
    ga2, gb2 = torch.autograd.grad(y2, (a2, b2), dy)
    assert torch.equal(y, y2) and torch.equal(ga, ga2) and torch.equal(gb, gb2)
    ref = torch.nn.functional.leaky_relu(torch.nn.functional.instance_norm(x, eps=EPS) + torch.nn.functional.instance_norm(skip, eps=EPS), SLOPE)
    assert torch.equal(y.detach(), ref)
