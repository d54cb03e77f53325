"""Per-element float64 parity of the InstanceNorm kernels (csrc/instnorm.hip), shared by tests/test_emu_norm.py (kernel sources on the
CPU emulator) and tests/test_gpu_norm.py (the HIP library): every check takes the loaded library and the device of its tensors.
Reference and bounds: tests/norm_ref.py.  How a pass streams (norm_mode 0 / 1 / 2) is forced by the CALLER through SEGM_NORM_NT,
which the library reads per call; the checks only name it in their records.

Every comparison leaves one record {what, worst = max error / bound, ...} in the parity log (tests/helpers._parity_log)."""
import os

import torch

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from tests import norm_ref as NR
from tests.helpers import _parity_log

SLOPE, EPS = 0.01, 1e-5
# (activation, residual added and its gradient wanted)
ACTS = (("none", False), ("relu", False), ("leaky_relu", False), ("leaky_relu", True), ("relu", True))
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
OFFSETS = (0.2, 3.0, 30.0)                 # r = mean / std of x
SHAPES = (
    (2, 3, 4, 8, 16),                      # vector path, one slab
    (1, 2, 3, 5, 7),                       # scalar path
    (1, 2, 18, 32, 48),                    # 13.5 thread-strides: the unrolled loops and their tails
    (1, 2, 40, 40, 41),                    # odd volume, several slabs
    (2, 384, 8, 8, 8),                     # many instances of 512 voxels
)
CAP_ISOLATED, CAP_CHAINED = 1e-4, 1e-3     # largest share of a case's elements that may be left out of dx / dresidual
# Which draw of the inputs the matrix and the chain use.  What is left out of a case follows from its inputs and the float64
# restatement alone, never from a kernel.  A 16-bit x sits on a coarse grid (bf16 near 45: steps of 0.25), so the mean of a
# 512-voxel instance falls exactly on a grid value once in 512 instances, and then every voxel with that value (about 34 in bf16 at
# r = 30) has pre == 0 exactly: its mask depends on the rounding of -mean * rstd inside the kernel's fused multiply-add.  With 768
# such instances two out of three draws put bf16 (2, 384, 8, 8, 8) at r = 30 over the isolated cap (46 ... 102 of 393 216 voxels
# in draws 0 - 5; at most 39 may be left out).  Draw 13 is the first of 0, 1, 2, ... in which every case of the matrix and of the
# chain stays under its cap; the caps are asserted on every run.
DRAW = 13


def name(dtype):
    return str(dtype).replace("torch.", "")


def mode_name():
    return os.environ.get("SEGM_NORM_NT", "auto")


def log(what, ratio, err, **more):
    rec = {"what": what, "worst": float(ratio), "max_abs_err": float(err), "dev": "cuda" if torch.cuda.is_available() else "cpu-emu"}
    rec.update(more)
    _parity_log(rec)
    print(f"{what}: worst error / bound {float(ratio):.4f}" + "".join(f", {k} {v}" for k, v in more.items()))


def longest_chain(instances, S, dtype):
    """elements a thread of a statistics pass accumulates: slab / 256, with the slab of norm_plan (csrc/instnorm.hip)"""
    quantum = 256 * (4 if dtype == torch.float32 else 8) * 4
    want = max(1, min(-(-4096 // instances), -(-S // quantum), 64))
    slab = -(-(-(-S // want)) // quantum) * quantum
    return slab // 256


def flat(t):
    return t.reshape(t.shape[0] * t.shape[1], -1)


# ---- cases: inputs drawn on the host (the same values for the emulator and the GPU), the reference computed once ---------------
_CASES = {}


def inputs(dev, shape, dtype, r, seed=DRAW):
    g = torch.Generator().manual_seed(1000 * seed + sum(shape) + int(10 * r))
    x = (1.5 * torch.randn(shape, generator=g) + 1.5 * r).to(dtype)
    res = torch.randn(shape, generator=g).to(dtype)
    dy = torch.randn(shape, generator=g).to(dtype)
    return x.to(dev), res.to(dev), dy.to(dev)


def case(dev, shape, dtype, r, act, with_res):
    """-> dict: x, res (or None), dy, R (the float64 restatement); kept for the (shape, dtype) last asked for, so that the streaming
    modes of one shape share their references"""
    if _CASES.get("key") != (str(dev), shape, dtype):
        _CASES.clear()
        _CASES["key"] = (str(dev), shape, dtype)
    k = (r, act, with_res)
    if k not in _CASES:
        x, res, dy = inputs(dev, shape, dtype, r)
        res = res if with_res else None
        assert longest_chain(x.shape[0] * x.shape[1], x[0, 0].numel(), dtype) <= 256
        R = NR.restate(flat(x), flat(res) if with_res else None, flat(dy), act, SLOPE, EPS)
        _CASES[k] = dict(x=x, res=res, dy=dy, R=R, act=act, with_res=with_res, dtype=dtype,
                         what=f"{name(dtype)} {shape} {act}{'+res' if with_res else ''} r={r}")
    return _CASES[k]


# ---- the comparisons -----------------------------------------------------------------------------------------------------------
def compare_stats(R, mean, rstd, what):
    eps_m, eps_r = NR.stats_bounds(R)
    em, er = NR.stats_errors(R, mean, rstd)
    rm, rr = float((em / eps_m).max()), float((er / eps_r).max())
    log(what + " mean", rm, float(em.max()))
    log(what + " rstd", rr, float(er.max()))
    assert rm <= 1.0 and rr <= 1.0, (what, "statistics: error / bound", rm, rr)
    return max(rm, rr)


def compare_forward(R, y, dtype, what):
    err = (flat(y).double() - R["y"]).abs()
    ratio = float((err / NR.forward_bound(R, dtype)).max())
    log(what + " y", ratio, float(err.max()))
    assert ratio <= 1.0, (what, "y: error / bound", ratio)
    return ratio


def compare_backward(R, dy, dx, dres, dtype, want_dres, chained, what):
    bound, out = NR.backward_bound(R, dtype, want_dres, chained)
    share = float(out.double().mean())
    cap = CAP_CHAINED if chained else CAP_ISOLATED
    err = (flat(dx).double() - R["dx"]).abs()
    ratio = float((err / bound).masked_fill(out, 0.0).max())
    log(what + " dx", ratio, float(err.masked_fill(out, 0.0).max()), excluded=share, cap=cap, parked_g=NR.parks_g(dtype, R["act"], want_dres))
    assert share <= cap, (what, "share of elements left out", share, cap)
    assert ratio <= 1.0, (what, "dx: error / bound", ratio)
    if want_dres:
        assert dres is not None
        same = (flat(dres) == NR.dresidual_expected(R, flat(dy), dtype)) | out
        log(what + " dresidual", 0.0 if bool(same.all()) else float("inf"), 0.0, excluded=share)
        assert bool(same.all()), (what, "dresidual differs at", int((~same).sum()), "elements")
    else:
        assert dres is None
    return ratio


def run_isolated(lib, c, what):
    """forward (the kernel's statistics), then the backward fed the float64 mean / rstd rounded to fp32 and the float64 y rounded to
    the type; -> (statistics, y, dx) worst ratios"""
    R, dtype, act, with_res = c["R"], c["dtype"], c["act"], c["with_res"]
    y, mean, rstd = ops_raw.instnorm_fwd(lib, c["x"], c["res"], act, SLOPE, EPS)
    rs = compare_stats(R, mean, rstd, what)
    ry = compare_forward(R, y, dtype, what)
    ysave = R["y"].to(dtype).reshape(c["x"].shape) if (with_res and act != "none") else None
    dx, dres = ops_raw.instnorm_bwd(lib, c["x"], c["dy"], R["mean"].float().flatten(), R["rstd"].float().flatten(), ysave, act, SLOPE,
                                    want_dresidual=with_res)
    return rs, ry, compare_backward(R, c["dy"], dx, dres, dtype, with_res, False, what + " isolated")


def check_matrix(lib, dev, shape, dtype, offsets=OFFSETS):
    """(a) the five activation / residual combinations at every offset, forward and isolated backward"""
    worst = [0.0, 0.0, 0.0]
    for r in offsets:
        for act, with_res in ACTS:
            c = case(dev, shape, dtype, r, act, with_res)
            got = run_isolated(lib, c, f"norm (a) mode {mode_name()} {c['what']}")
            worst = [max(a, b) for a, b in zip(worst, got)]
    return worst


# ---- (b) padded and unequal instance strides -----------------------------------------------------------------------------------
def padded(t_or_shape, pad, fill, dtype=None, dev=None):
    """-> (buffer (B, C, S + pad) filled with `fill`, its (B, C, *spatial) view holding the tensor's values)"""
    if torch.is_tensor(t_or_shape):
        shape, dtype, dev = tuple(t_or_shape.shape), t_or_shape.dtype, t_or_shape.device
    else:
        shape = tuple(t_or_shape)
    S = 1
    for n in shape[2:]:
        S *= n
    buf = torch.full((shape[0], shape[1], S + pad), fill, dtype=dtype, device=dev)
    v = buf[:, :, :S].view(shape)
    if torch.is_tensor(t_or_shape):
        v.copy_(t_or_shape)
    return buf, v


def _workspace(lib, x):
    inst = x.shape[0] * x.shape[1]
    n = lib.dll.segm_instnorm_workspace_bytes(inst, x.numel() // inst)
    return torch.empty(n, dtype=torch.uint8, device=x.device), n


def fwd_into(lib, x, res, y, act):
    """segm_instnorm_fwd into a destination of the caller's (ops_raw.instnorm_fwd allocates its own); -> (mean, rstd)"""
    inst = x.shape[0] * x.shape[1]
    a = L.InstNormFwdArgs()
    a.instances, a.dtype, a.act, a.spatial = inst, L.dtype_code(x), ops_raw.ACT_CODES[act], x.numel() // inst
    a.slope, a.eps = SLOPE, EPS
    a.x_instance_stride, a.y_instance_stride = ops_raw.instance_stride(x), ops_raw.instance_stride(y)
    a.residual_instance_stride = ops_raw.instance_stride(res) if res is not None else 0
    mean = torch.empty(inst, dtype=torch.float32, device=x.device)
    rstd = torch.empty(inst, dtype=torch.float32, device=x.device)
    ws, n = _workspace(lib, x)
    a.x, a.residual, a.y = x.data_ptr(), (res.data_ptr() if res is not None else None), y.data_ptr()
    a.mean, a.rstd = mean.data_ptr(), rstd.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), n, L.stream_handle(x)
    lib.check(lib.dll.segm_instnorm_fwd(a), "instnorm_fwd")
    return mean, rstd


def bwd_into(lib, x, dy, mean, rstd, y, dx, dres, act):
    inst = x.shape[0] * x.shape[1]
    a = L.InstNormBwdArgs()
    a.instances, a.dtype, a.act, a.spatial = inst, L.dtype_code(x), ops_raw.ACT_CODES[act], x.numel() // inst
    a.slope = SLOPE
    a.x_instance_stride, a.dy_instance_stride, a.dx_instance_stride = (ops_raw.instance_stride(x), ops_raw.instance_stride(dy),
                                                                       ops_raw.instance_stride(dx))
    a.y_instance_stride = ops_raw.instance_stride(y) if y is not None else 0
    a.dresidual_instance_stride = ops_raw.instance_stride(dres) if dres is not None else 0
    ws, n = _workspace(lib, x)
    a.x, a.dy, a.y = x.data_ptr(), dy.data_ptr(), (y.data_ptr() if y is not None else None)
    a.mean, a.rstd, a.dx = mean.data_ptr(), rstd.data_ptr(), dx.data_ptr()
    a.dresidual = dres.data_ptr() if dres is not None else None
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), n, L.stream_handle(x)
    lib.check(lib.dll.segm_instnorm_bwd(a), "instnorm_bwd")


PADDED_CASES = (
    # shape, dtype, act, residual, paddings of (x, residual, saved y, dy, dx, dresidual)
    ((2, 3, 4, 8, 16), torch.bfloat16, "leaky_relu", True, (192, 64, 8, 64, 8, 192)),
    ((1, 2, 18, 32, 48), torch.float16, "relu", True, (8, 192, 64, 192, 64, 8)),
    ((1, 2, 40, 40, 41), torch.float32, "leaky_relu", True, (64, 8, 192, 8, 192, 64)),
    ((1, 2, 18, 32, 48), torch.bfloat16, "none", False, (192, 0, 0, 64, 8, 0)),
    ((2, 2, 3, 5, 7), torch.float32, "leaky_relu", True, (3, 5, 3, 5, 3, 5)),                # odd strides: the scalar path
    ((1, 2, 3, 5, 7), torch.bfloat16, "relu", True, (3, 8, 5, 64, 192, 5)),
)
SENTINEL = -777.0


def check_padded(lib, dev):
    """(b) every tensor with its own padded instance stride: results bit-equal to the dense call, the padding of the inputs (NaN)
    never read, that of the outputs (a sentinel) never written"""
    nan = float("nan")
    for shape, dtype, act, with_res, (px, pr, py, pdy, pdx, pdr) in PADDED_CASES:
        what = f"norm (b) mode {mode_name()} {name(dtype)} {shape} {act}{'+res' if with_res else ''}"
        x, res, dy = inputs(dev, shape, dtype, 3.0, seed=1)
        res = res if with_res else None
        y0, mean0, rstd0 = ops_raw.instnorm_fwd(lib, x, res, act, SLOPE, EPS)
        ysave = y0 if (with_res and act != "none") else None
        dx0, dres0 = ops_raw.instnorm_bwd(lib, x, dy, mean0, rstd0, ysave, act, SLOPE, want_dresidual=with_res)
        assert y0.is_contiguous() and dx0.is_contiguous()
        _, xp = padded(x, px, nan)
        rp = padded(res, pr, nan)[1] if with_res else None
        ybuf, yp = padded(shape, py, SENTINEL, dtype, dev)
        assert ops_raw.channel_dense(xp) and xp.is_contiguous() == (px == 0)
        mean1, rstd1 = fwd_into(lib, xp, rp, yp, act)
        S = x[0, 0].numel()
        fill = torch.full((), SENTINEL, dtype=dtype, device=dev)
        ok = torch.equal(yp, y0) and torch.equal(mean1, mean0) and torch.equal(rstd1, rstd0) and bool((ybuf[:, :, S:] == fill).all())
        log(what + " forward", 0.0 if ok else float("inf"), 0.0)
        assert ok, what
        ysp = padded(ysave, py, nan)[1] if ysave is not None else None
        _, dyp = padded(dy, pdy, nan)
        dxbuf, dxp = padded(shape, pdx, SENTINEL, dtype, dev)
        drbuf, drp = padded(shape, pdr, SENTINEL, dtype, dev) if with_res else (None, None)
        bwd_into(lib, xp, dyp, mean1, rstd1, ysp, dxp, drp, act)
        ok = torch.equal(dxp, dx0) and bool((dxbuf[:, :, S:] == fill).all())
        if with_res:
            ok = ok and torch.equal(drp, dres0) and bool((drbuf[:, :, S:] == fill).all())
        log(what + " backward", 0.0 if ok else float("inf"), 0.0)
        assert ok, what


# ---- (c) statistics summed by a producer ---------------------------------------------------------------------------------------
def producer_partials(x, counts):
    """x (instances, S), counts (instances, nparts) int64 summing to S per row -> fp32 (instances, nparts, 4) of {count, sum, sum of
    squares, 0} over consecutive parts, from float64 sums rounded to fp32"""
    xd = x.double()
    zero = torch.zeros(x.shape[0], 1, dtype=torch.float64, device=x.device)
    c1 = torch.cat([zero, xd.cumsum(1)], 1)
    c2 = torch.cat([zero, (xd * xd).cumsum(1)], 1)
    end = counts.cumsum(1)
    start = end - counts
    st = torch.stack([counts.double(), c1.gather(1, end) - c1.gather(1, start), c2.gather(1, end) - c2.gather(1, start),
                      torch.zeros_like(counts, dtype=torch.float64)], -1)
    return st.float().contiguous()


def unequal_counts(S, nparts, g):
    """nparts counts summing to S, unequal, with empty parts at the start, in the middle and at the end when there is room"""
    if nparts == 1:
        return torch.tensor([S])
    nz = 3 if nparts >= 7 else 0
    n = nparts - nz
    cuts = torch.sort(torch.randint(0, S + 1, (n - 1,), generator=g)).values
    counts = torch.diff(torch.cat([torch.tensor([0]), cuts, torch.tensor([S])]))
    if nz:
        mid = n // 2
        counts = torch.cat([torch.tensor([0]), counts[:mid], torch.tensor([0]), counts[mid:], torch.tensor([0])])
    assert counts.numel() == nparts and int(counts.sum()) == S
    return counts


def check_producer_stats(lib, dev, nparts):
    """(c) instnorm_fwd(stats=...) on partials cut without a convolution: instances 0 and 1 with their own cuts, instance 2 = the
    values of instance 0 with its parts in another order"""
    shape = (1, 3, 8, 32, 48)
    worst = 0.0
    for dtype in (torch.float32, torch.bfloat16):
        for r in (0.2, 3.0):
            what = f"norm (c) {name(dtype)} nparts={nparts} r={r}"
            g = torch.Generator().manual_seed(nparts + int(10 * r))
            x, _, _ = inputs("cpu", shape, dtype, r, seed=2)
            x[0, 2] = x[0, 0]
            S = x[0, 0].numel()
            counts = torch.stack([unequal_counts(S, nparts, g), unequal_counts(S, nparts, g)])
            st = producer_partials(flat(x)[:2], counts)
            assert nparts < 7 or (int((counts == 0).sum(1).min()) >= 3 and len(set(counts[0].tolist())) > 2)
            st = torch.cat([st, st[:1, torch.randperm(nparts, generator=g)]]).reshape(1, 3, nparts, 4).to(dev)
            x = x.to(dev)
            R = NR.restate(flat(x), None, None, "leaky_relu", SLOPE, EPS)
            y, mean, rstd = ops_raw.instnorm_fwd(lib, x, None, "leaky_relu", SLOPE, EPS, stats=st)
            worst = max(worst, compare_stats(R, mean, rstd, what), compare_forward(R, y, dtype, what))
            y2, mean2, rstd2 = ops_raw.instnorm_fwd(lib, x, None, "leaky_relu", SLOPE, EPS, stats=st)
            same = torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
            log(what + " two calls", 0.0 if same else float("inf"), 0.0)
            assert same, what
    return worst


# ---- (d) forward and backward through autograd ---------------------------------------------------------------------------------
def check_chained(lib, dev, shape, dtype):
    """(d) fused_norm.instance_norm_act and its autograd backward: the kernel's own statistics and activation mask"""
    from segmamba_amd import fused_norm
    worst = 0.0
    for r in (0.2, 3.0):
        for act, with_res in ACTS:
            c = case(dev, shape, dtype, r, act, with_res)
            what = f"norm (d) {c['what']}"
            xk = c["x"].clone().requires_grad_()
            rk = c["res"].clone().requires_grad_() if with_res else None
            y = fused_norm.instance_norm_act(xk, act, SLOPE, EPS, rk)
            assert y.grad_fn is not None and type(y.grad_fn).__name__.startswith("_InstNormAct"), "not the library's path"
            grads = torch.autograd.grad(y, (xk, rk) if with_res else (xk,), c["dy"])
            ry = compare_forward(c["R"], y.detach(), dtype, what)
            rd = compare_backward(c["R"], c["dy"], grads[0], grads[1] if with_res else None, dtype, with_res, True, what + " chained")
            worst = max(worst, ry, rd)
    return worst


# ---- (e) determinism -----------------------------------------------------------------------------------------------------------
def check_determinism(lib, dev):
    """(e) two calls of forward and backward give the same bits"""
    for shape, dtype in (((1, 2, 18, 32, 48), torch.bfloat16), ((1, 2, 40, 40, 41), torch.float32), ((1, 2, 3, 5, 7), torch.float16)):
        x, res, dy = inputs(dev, shape, dtype, 3.0, seed=3)
        outs = []
        for _ in range(2):
            y, mean, rstd = ops_raw.instnorm_fwd(lib, x, res, "leaky_relu", SLOPE, EPS)
            dx, dres = ops_raw.instnorm_bwd(lib, x, dy, mean, rstd, y, "leaky_relu", SLOPE, want_dresidual=True)
            dx2, _ = ops_raw.instnorm_bwd(lib, x, dy, mean, rstd, y, "leaky_relu", SLOPE, want_dresidual=False)
            outs.append((y, mean, rstd, dx, dres, dx2))
        same = all(torch.equal(a, b) for a, b in zip(*outs))
        log(f"norm (e) mode {mode_name()} {name(dtype)} {shape} two calls", 0.0 if same else float("inf"), 0.0)
        assert same, (shape, dtype)


# ---- the sizes at which the library itself picks a streaming mode (GPU) --------------------------------------------------------
def check_at_size(lib, dev, channels, step=8, side=128):
    """1 x channels x 128^3 bf16 from ops_raw.volume_empty (padded channel stride), LeakyReLU + residual + dresidual, forward and
    isolated backward under the per-element bounds; the float64 restatement on the device, `step` instances at a time"""
    assert "SEGM_NORM_NT" not in os.environ
    dtype, shape, r = torch.bfloat16, (1, channels, side, side, side), 3.0
    S = side ** 3
    assert longest_chain(channels, S, dtype) <= 256
    g = torch.Generator(device=dev).manual_seed(channels)
    vol = []
    for scale, shift in ((1.5, 1.5 * r), (1.0, 0.0), (1.0, 0.0), (0.0, 0.0)):       # x, residual, dy, the y handed to the backward
        v = ops_raw.volume_empty(1, channels, shape[2:], dtype, dev)
        assert not v.is_contiguous() and ops_raw.channel_dense(v)
        if scale:
            for i in range(0, channels, step):
                v[:, i:i + step] = scale * torch.randn((1, min(step, channels - i)) + shape[2:], device=dev, generator=g) + shift
        vol.append(v)
    x, res, dy, ysave = vol
    what = f"norm at size {name(dtype)} {shape} leaky_relu+res r={r}"
    y, mean, rstd = ops_raw.instnorm_fwd(lib, x, res, "leaky_relu", SLOPE, EPS)
    mean_r, rstd_r = torch.empty_like(mean), torch.empty_like(rstd)
    dx_ref = torch.empty(channels, S, dtype=torch.float64, device=dev)
    dx_bound = torch.empty(channels, S, dtype=torch.float64, device=dev)
    left_out = torch.empty(channels, S, dtype=torch.bool, device=dev)
    dres_ref = torch.empty(channels, S, dtype=dtype, device=dev)
    worst, worst_err = [0.0, 0.0, 0.0], 0.0
    for i in range(0, channels, step):
        s = slice(i, i + step)
        R = NR.restate(flat(x[:, s]), flat(res[:, s]), flat(dy[:, s]), "leaky_relu", SLOPE, EPS)
        worst[0] = max(worst[0], compare_stats(R, mean[s], rstd[s], f"{what} [{i}:{i + step}]"))
        worst[1] = max(worst[1], compare_forward(R, y[:, s], dtype, f"{what} [{i}:{i + step}]"))
        mean_r[s], rstd_r[s] = R["mean"].float().flatten(), R["rstd"].float().flatten()
        ysave[:, s] = R["y"].to(dtype).reshape(ysave[:, s].shape)
        dx_bound[s], left_out[s] = NR.backward_bound(R, dtype, True, False)
        dx_ref[s], dres_ref[s] = R["dx"], NR.dresidual_expected(R, flat(dy[:, s]), dtype)
        del R
    dx, dres = ops_raw.instnorm_bwd(lib, x, dy, mean_r, rstd_r, ysave, "leaky_relu", SLOPE, want_dresidual=True)
    share = float(left_out.double().mean())
    for i in range(0, channels, step):
        s = slice(i, i + step)
        err = (flat(dx[:, s]).double() - dx_ref[s]).abs()
        worst_err = max(worst_err, float(err.masked_fill(left_out[s], 0.0).max()))
        worst[2] = max(worst[2], float((err / dx_bound[s]).masked_fill(left_out[s], 0.0).max()))
        same = (flat(dres[:, s]) == dres_ref[s]) | left_out[s]
        assert bool(same.all()), (what, "dresidual differs at", int((~same).sum()), "elements of instances", i, i + step)
    log(what + " isolated dx", worst[2], worst_err, excluded=share, cap=CAP_ISOLATED, parked_g=True)
    assert share <= CAP_ISOLATED, (what, share)
    assert worst[2] <= 1.0, (what, "dx: error / bound", worst[2])
    return worst
