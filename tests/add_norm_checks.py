"""The checks of the fused add + LayerNorm / RMSNorm (csrc/add_norm.hip through segmamba_amd.ops_raw, add_norm and mamba_simple.Block)
that the CPU emulation (tests/test_emu_add_norm.py) and the GPU (tests/test_gpu_add_norm.py) share: `lib` is the loaded library, `dev`
where the tensors live.  References: tests/add_norm_ref.py (float64, closed form) and the recorded tests/golden/add_norm.npz.  TEST
INFRASTRUCTURE ONLY.

Bounds.  y, dx, dresidual_in: tol x max(1, max |ref|) with tol = 2e-5 (fp32) and 2e-2 (bf16), the bounds tests/test_gpu_kernels.py
holds the existing LayerNorm to, and 2.5e-3 (fp16) = the bf16 bound times the ratio of the unit roundoffs 2^-11 / 2^-8.  dweight,
dbias: 2e-3 x max(1, max |ref|), as there.  mean and rstd are fp32 statistics of fp32 data: the fp32 bound.  Everything called
"exact" is compared bit for bit."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from segmamba_amd import add_norm as AN, lib as L, ops_raw
from segmamba_amd.mamba_simple import Block
from tests import add_norm_ref as R
from tests import helpers

NEW_EXPORTS = ("segm_add_norm_fwd", "segm_add_norm_bwd", "segm_add_norm_workspace_bytes")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "add_norm.npz")
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
TOL = {torch.float32: 2e-5, torch.bfloat16: 2e-2, torch.float16: 2.5e-3}
TOL_W = 2e-3
EPS = 1e-5
# every N of {1, 7, 8, 48, 96, 100, 384, 768, 1024, 1032, 4100, 8192} and every M of {1, 2, 63, 64, 65, 257}: the wide rows with
# few of them.  In 16 bits 1032 and 4100 leave the last packet partial; in fp32 4100 is whole packets, eight per lane at 8192.
GRID = ((257, 1), (65, 7), (64, 8), (257, 48), (63, 96), (257, 100), (65, 384), (64, 768), (63, 1024), (2, 1032), (1, 4100),
        (2, 8192), (65, 4100))
RESIDUALS = ("none", "same", "fp32", "none_fp32")     # none_fp32: no residual, the sum kept as an fp32 stream

_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
        assert os.path.getsize(GOLDEN) < 1 << 20
    return _golden


def close(got, ref, tol, what):
    """|got - ref| <= tol x max(1, max |ref|); the margin goes to the parity log"""
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return
    ref = ref.detach().double()
    err = float((got.detach().double() - ref.to(got.device)).abs().max())
    scale = max(1.0, float(ref.abs().max()))
    helpers._parity_log({"what": what, "max_abs_err": err, "ref_max": scale, "worst": err / (tol * scale), "rtol": 0.0, "atol": tol * scale,
                         "dev": "cuda" if got.is_cuda else "cpu-emu"})
    assert err <= tol * scale, f"{what}: max error {err:.3e} > {tol:g} x {scale:.3e}"


def same_bits(a, b, what):
    assert (a is None) == (b is None), what
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape, what
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), what


def make_case(rs, M, N, dtype, res, dev):
    """-> dict of device tensors: x, residual (or None), w, b, dy, dres; residual_dtype as add_norm_fwd takes it"""
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))      # noqa: E731
    rdt = {"none": None, "same": dtype, "fp32": torch.float32, "none_fp32": torch.float32}[res]
    c = {"x": t(M, N).to(dtype).to(dev), "w": (1.0 + 0.3 * t(N)).to(dev), "b": (0.5 * t(N)).to(dev), "dy": t(M, N).to(dtype).to(dev),
         "residual": t(M, N).to(rdt).to(dev) if res in ("same", "fp32") else None,
         "dres": t(M, N).to(rdt or dtype).to(dev), "residual_dtype": rdt if res == "none_fp32" else None}
    return c


def run(lib, c, rms, has_b, with_dres, eps=EPS):
    """forward and backward through ops_raw -> dict of everything the two entries wrote"""
    y, mean, rstd, res_out = ops_raw.add_norm_fwd(lib, c["x"], c["w"], c["b"] if has_b else None, c["residual"], eps, rms,
                                                  c["residual_dtype"])
    saved = res_out if res_out is not None else c["x"]
    dres = c["dres"] if with_dres else None
    dx, dw, db, dres_in = ops_raw.add_norm_bwd(lib, c["dy"], saved, c["w"], mean, rstd, dres, c["residual"] is not None, has_b, rms)
    return {"y": y, "mean": mean, "rstd": rstd, "res_out": res_out, "dx": dx, "dw": dw, "db": db, "dres_in": dres_in, "saved": saved}


# ---- 1. values against the float64 restatement --------------------------------------------------------------------------------------------
def check_values_one(lib, dev, rs, M, N, dtype, res, rms, has_b, with_dres):
    what = f"add_norm {M}x{N} {dtype} res={res} rms={rms} bias={has_b} dres={with_dres}"
    c = make_case(rs, M, N, dtype, res, dev)
    o = run(lib, c, rms, has_b, with_dres)
    yr, s, meanr, rstdr = R.forward(c["x"], c["w"], c["b"] if has_b else None, c["residual"], EPS, rms)
    tol = TOL[dtype]
    assert o["y"].dtype == dtype and o["dx"].dtype == dtype
    close(o["y"], yr, tol, what + " y")
    close(o["rstd"], rstdr, TOL[torch.float32], what + " rstd")
    if rms:
        assert o["mean"] is None
    else:
        close(o["mean"], meanr, TOL[torch.float32], what + " mean")
    if res == "none" or (res == "none_fp32" and dtype == torch.float32):      # the sum is x itself: nothing to write
        assert o["res_out"] is None
    else:
        want = c["x"].float() + c["residual"].float() if c["residual"] is not None else c["x"].float()
        same_bits(o["res_out"], want.to(torch.float32 if res != "same" else dtype), what + " residual_out")
    dxr, dwr, dbr = R.backward(c["dy"], o["saved"], c["w"], meanr, rstdr, c["dres"] if with_dres else None, rms)
    close(o["dx"], dxr, tol, what + " dx")
    close(o["dw"], dwr, TOL_W, what + " dweight")
    if has_b:
        close(o["db"], dbr, TOL_W, what + " dbias")
    else:
        assert o["db"] is None
    if c["residual"] is None:
        assert o["dres_in"] is None
    elif o["saved"].dtype == dtype:
        assert o["dres_in"] is o["dx"]
    else:
        assert o["dres_in"].dtype == torch.float32
        close(o["dres_in"], dxr, tol, what + " dresidual_in")
        same_bits(o["dres_in"].to(dtype), o["dx"], what + " dx is dresidual_in rounded")


def check_values(lib, dev, grid=GRID):
    """every (M, N) of GRID x the three dtypes x the four residual kinds x LayerNorm / RMS; bias and dresidual (prenorm) rotate so
    that each of their four pairs meets every dtype, residual kind and norm"""
    rs = np.random.RandomState(7)
    n = 0
    for gi, (M, N) in enumerate(grid):
        for di, dtype in enumerate(DTYPES):
            for ri, res in enumerate(RESIDUALS):
                for rms in (False, True):
                    k = gi + di + ri + int(rms)
                    check_values_one(lib, dev, rs, M, N, dtype, res, rms, bool(k & 1), bool(k & 2))
                    n += 1
    # all four (bias, dresidual) pairs on one shape of each route, so none of them depends on the rotation above
    for M, N in ((65, 100), (64, 96)):
        for dtype in DTYPES:
            for res in RESIDUALS:
                for rms in (False, True):
                    for pair in range(4):
                        check_values_one(lib, dev, rs, M, N, dtype, res, rms, bool(pair & 1), bool(pair & 2))
    return n


# ---- 2. exact values --------------------------------------------------------------------------------------------------------------------------
EXACT_SIZES = ((3, 48), (4099, 96), (70001, 48))


def check_exact(lib, dev, sizes=EXACT_SIZES):
    """residual_out is one fp32 add and one rounding; small-integer dy gives the integer column sums in dbias; RMS with eps = 0,
    w = 1 and rows of +-2^k has rstd = 2^-k and xhat = +-1, so y = +-1 and dweight = the signed integer sums - all exactly.  A dropped
    or doubled row or column shows here, where the scaled bounds would hide it.  Sums stay below 2^24: 70001 rows x |dy| <= 3."""
    rs = np.random.RandomState(3)
    for M, N in sizes:
        what = f"add_norm exact {M}x{N}"
        x = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(torch.bfloat16).to(dev)
        res = torch.from_numpy(rs.standard_normal((M, N)).astype(np.float32)).to(dev)
        w = torch.ones(N, device=dev)
        b = torch.zeros(N, device=dev)
        dy_i = torch.from_numpy(rs.randint(-3, 4, size=(M, N)).astype(np.float32)).to(dev)
        y, mean, rstd, res_out = ops_raw.add_norm_fwd(lib, x, w, b, res, EPS, False)
        same_bits(res_out, x.float() + res, what + " residual_out fp32")
        dx, dw, db, dres_in = ops_raw.add_norm_bwd(lib, dy_i.to(torch.bfloat16), res_out, w, mean, rstd, None, True, True, False)
        same_bits(db, dy_i.double().sum(0).float(), what + " dbias")
        res16 = res.to(torch.bfloat16)
        _, _, _, out16 = ops_raw.add_norm_fwd(lib, x, w, None, res16, EPS, True)
        same_bits(out16, (x.float() + res16.float()).to(torch.bfloat16), what + " residual_out bf16")
        # RMS on rows of +-2^k
        k = torch.from_numpy(rs.randint(-3, 4, size=(M, 1)).astype(np.float32)).to(dev)
        sign = torch.from_numpy((rs.randint(0, 2, size=(M, N)) * 2 - 1).astype(np.float32)).to(dev)
        for dtype in (torch.bfloat16, torch.float32):
            xp = (sign * torch.exp2(k)).to(dtype)
            y, mean, rstd, res_out = ops_raw.add_norm_fwd(lib, xp, w, None, None, 0.0, True)
            assert mean is None and res_out is None
            same_bits(rstd, torch.exp2(-k[:, 0]), what + f" rstd {dtype}")
            same_bits(y, sign.to(dtype), what + f" y {dtype}")
            dx, dw, db, _ = ops_raw.add_norm_bwd(lib, dy_i.to(dtype), xp, w, None, rstd, None, False, False, True)
            assert db is None
            same_bits(dw, (dy_i.double() * sign.double()).sum(0).float(), what + f" dweight {dtype}")
            # with w = 1 and xhat = +-1: dx = (dy - xhat mean(xhat dy)) 2^-k
            dxr, _, _ = R.backward(dy_i, xp, w, torch.zeros(M, device=dev), rstd, None, True)
            close(dx, dxr, TOL[dtype], what + f" dx {dtype}")


# ---- 3. independence, repeatability, the two routes -------------------------------------------------------------------------------------------
OUTPUTS = ("y", "mean", "rstd", "res_out", "dx", "dw", "db", "dres_in")


def assert_same_outputs(a, b, what, names=OUTPUTS):
    for n in names:
        same_bits(a[n], b[n], f"{what}: {n}")


def check_repeat(lib, dev):
    """two calls are bit-equal in every output; (4099, 96) has several workgroups and partial rows in the backward"""
    rs = np.random.RandomState(5)
    for (M, N), dtype, res, rms in (((257, 100), torch.bfloat16, "fp32", False), ((65, 1032), torch.float16, "same", True),
                                    ((4099, 96), torch.bfloat16, "fp32", False), ((9, 8192), torch.float32, "same", False)):
        c = make_case(rs, M, N, dtype, res, dev)
        assert_same_outputs(run(lib, c, rms, True, True), run(lib, c, rms, True, True), f"add_norm repeat {M}x{N}")


def check_row_independence(lib, dev):
    """row 0 computed alone equals row 0 inside M = 257 and inside M = 4099, bit for bit: y, residual_out, dx, dresidual_in, mean, rstd"""
    rs = np.random.RandomState(6)
    for N, dtype, res in ((96, torch.bfloat16, "fp32"), (100, torch.float16, "same"), (1032, torch.float32, "same"),
                          (4100, torch.bfloat16, "fp32")):
        for M in (257, 4099) if N <= 100 else (257,):
            for rms in (False, True):
                c = make_case(rs, M, N, dtype, res, dev)
                full = run(lib, c, rms, True, True)
                one = run(lib, {k: (v[:1] if isinstance(v, torch.Tensor) and v.dim() == 2 else v) for k, v in c.items()}, rms, True, True)
                for n in ("y", "mean", "rstd", "res_out", "dx", "dres_in"):
                    if full[n] is not None:
                        same_bits(full[n][:1].clone(), one[n], f"add_norm row 0 of {M}x{N} {dtype} rms={rms}: {n}")


def shifted(t, stride, offset):
    """the (M, N) values of t in a fresh buffer with row stride `stride`, starting `offset` elements into it; the last element of
    the view is the last of the buffer"""
    M, N = t.shape
    buf = torch.zeros(offset + (M - 1) * stride + N, dtype=t.dtype, device=t.device)
    v = buf.as_strided((M, N), (stride, 1), offset)
    v.copy_(t)
    return v


def check_routes(lib, dev):
    """the packet and the element route agree bit for bit: the same data once at an aligned base with an aligned row stride, once
    one element further (nothing is aligned then); every packets-per-lane case of both element sizes"""
    rs = np.random.RandomState(8)
    for N, dtype, res in ((8, torch.bfloat16, "same"), (48, torch.bfloat16, "fp32"), (768, torch.bfloat16, "fp32"),
                          (1024, torch.float32, "same"), (2048, torch.float16, "same"), (4096, torch.bfloat16, "fp32"),
                          (8192, torch.float32, "same"), (8192, torch.float16, "fp32")):
        M = 5
        for rms in (False, True):
            c = make_case(rs, M, N, dtype, res, dev)
            moved = lambda off: {k: (shifted(v, N + 16, off) if isinstance(v, torch.Tensor) and v.dim() == 2 else v)   # noqa: E731
                                 for k, v in c.items()}
            a, b = moved(0), moved(1)
            assert a["x"].data_ptr() % 16 == 0 and b["x"].data_ptr() % 16 != 0
            assert_same_outputs(run(lib, a, rms, True, True), run(lib, b, rms, True, True), f"add_norm routes N={N} {dtype} rms={rms}")
            assert_same_outputs(run(lib, a, rms, True, True), run(lib, c, rms, True, True), f"add_norm strided N={N} {dtype}")


def check_layouts(lib, dev):
    """row strides larger than N, a multiple of the packet or not, give the bits of the dense call"""
    rs = np.random.RandomState(9)
    for (M, N), dtype, res in (((7, 48), torch.bfloat16, "fp32"), ((5, 100), torch.float32, "same"), ((3, 1032), torch.float16, "same")):
        c = make_case(rs, M, N, dtype, res, dev)
        dense = run(lib, c, False, True, True)
        for stride, off in ((N + 8, 0), (N + 3, 0), (N + 8, 5)):
            v = {k: (shifted(t, stride, off) if isinstance(t, torch.Tensor) and t.dim() == 2 else t) for k, t in c.items()}
            assert_same_outputs(dense, run(lib, v, False, True, True), f"add_norm {M}x{N} stride {stride} offset {off}")


# ---- 4. refusals, exports ---------------------------------------------------------------------------------------------------------------------
def check_refusals(lib, dev):
    """the C entries return their codes and write nothing; ops_raw raises before any call"""
    M, N = 4, 48
    x = torch.randn(M, N, device=dev)
    y = torch.full((M, N), 7.0, device=dev)
    w = torch.ones(N, device=dev)
    mean, rstd = torch.full((M,), 7.0, device=dev), torch.full((M,), 7.0, device=dev)
    dwt = torch.full((N,), 7.0, device=dev)
    ws = torch.empty(lib.dll.segm_add_norm_workspace_bytes(M, N) // 4, device=dev)

    def args(**kw):
        a = L.AddNormArgs()
        a.rows, a.cols, a.dtype, a.res_dtype, a.eps = M, N, L.SEGM_F32, L.SEGM_F32, 1e-5
        a.x, a.x_stride, a.y, a.y_stride = x.data_ptr(), N, y.data_ptr(), N
        a.dy, a.dy_stride, a.dx, a.dx_stride = x.data_ptr(), N, y.data_ptr(), N
        a.weight, a.mean, a.rstd, a.dweight = w.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dwt.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
        a.stream = L.stream_handle(x)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    E_NULL, E_SHAPE, E_DTYPE, E_WS = -1, -2, -4, -6
    both = (lib.dll.segm_add_norm_fwd, lib.dll.segm_add_norm_bwd)
    for fn in both:
        assert fn(None) == E_NULL
        for kw in (dict(cols=0), dict(cols=L.ADD_NORM_MAX_COLS + 1), dict(rows=0), dict(rows=1 << 31), dict(x_stride=N - 1),
                   dict(x=x.data_ptr() + 2)):
            assert fn(args(**kw)) == E_SHAPE, (fn.__name__, kw)
        for kw in (dict(dtype=7), dict(dtype=L.SEGM_BF16, res_dtype=L.SEGM_F16)):
            assert fn(args(**kw)) == E_DTYPE, (fn.__name__, kw)
        for kw in (dict(x=None), dict(weight=None), dict(rstd=None), dict(mean=None)):
            assert fn(args(**kw)) == E_NULL, (fn.__name__, kw)
        assert fn(args(mean=None, rms=1, cols=0)) == E_SHAPE
    assert lib.dll.segm_add_norm_fwd(args(y=None)) == E_NULL
    assert lib.dll.segm_add_norm_fwd(args(residual=x.data_ptr(), residual_stride=N - 1)) == E_SHAPE
    for kw in (dict(dy=None), dict(dx=None), dict(dweight=None)):
        assert lib.dll.segm_add_norm_bwd(args(**kw)) == E_NULL, kw
    assert lib.dll.segm_add_norm_bwd(args(dy_stride=N - 1)) == E_SHAPE
    for kw in (dict(workspace=None), dict(workspace_bytes=ws.numel() * 4 - 1)):
        assert lib.dll.segm_add_norm_bwd(args(**kw)) == E_WS, kw
    assert lib.dll.segm_add_norm_workspace_bytes(0, N) == 0 and lib.dll.segm_add_norm_workspace_bytes(M, 8193) == 0
    assert lib.dll.segm_add_norm_workspace_bytes(1 << 31, N) == 0
    if dev != "cpu":
        torch.cuda.synchronize()
    for t in (y, mean, rstd, dwt):
        assert bool((t == 7.0).all()), "a refused call wrote"

    b = torch.zeros(N, device=dev)
    elsewhere = torch.ones(N, device="meta")
    for bad in (lambda: ops_raw.add_norm_fwd(lib, x[None], w), lambda: ops_raw.add_norm_fwd(lib, x, w[:-1]),
                lambda: ops_raw.add_norm_fwd(lib, x, w, b[:-1]), lambda: ops_raw.add_norm_fwd(lib, x, w, None, x[:-1]),
                lambda: ops_raw.add_norm_fwd(lib, x.to(torch.int32), w), lambda: ops_raw.add_norm_fwd(lib, x, w.to(torch.bfloat16)),
                lambda: ops_raw.add_norm_fwd(lib, x.double(), w), lambda: ops_raw.add_norm_fwd(lib, x, w, None, x.to(torch.bfloat16)),
                lambda: ops_raw.add_norm_fwd(lib, x.to(torch.bfloat16), w, None, x.to(torch.float16)),
                lambda: ops_raw.add_norm_fwd(lib, x, w, None, None, 1e-5, False, torch.float16),
                lambda: ops_raw.add_norm_fwd(lib, x, elsewhere), lambda: ops_raw.add_norm_fwd(lib, x, w, elsewhere),
                lambda: ops_raw.add_norm_fwd(lib, x, w, None, torch.ones(M, N, device="meta")),
                lambda: ops_raw.add_norm_fwd(lib, x.t().contiguous().t(), w),
                lambda: ops_raw.add_norm_fwd(lib, torch.zeros(2, 8193, device=dev), torch.ones(8193, device=dev)),
                lambda: ops_raw.add_norm_fwd(lib, x.expand(3, M, N)[:, 0], w),
                lambda: ops_raw.add_norm_bwd(lib, x, x, w, mean, rstd[:-1]), lambda: ops_raw.add_norm_bwd(lib, x, x, w, None, rstd),
                lambda: ops_raw.add_norm_bwd(lib, x, x[:, :-1], w, mean, rstd), lambda: ops_raw.add_norm_bwd(lib, x, x.double(), w, mean, rstd),
                lambda: ops_raw.add_norm_bwd(lib, x, x, w, mean, rstd, x.to(torch.bfloat16)),
                lambda: ops_raw.add_norm_bwd(lib, x, x, w, mean, torch.ones(M, device="meta")),
                lambda: ops_raw.add_norm_bwd(lib, torch.zeros(2, 8193, device=dev), torch.zeros(2, 8193, device=dev), torch.ones(8193, device=dev),
                                             mean[:2], rstd[:2])):
        with pytest.raises(RuntimeError):
            bad()


def check_exports(lib):
    assert lib.missing == []
    assert all(hasattr(lib.dll, n) for n in NEW_EXPORTS) and set(NEW_EXPORTS) <= set(L.EXPORTS)
    assert lib.dll.segm_abi_version() == L.header_abi_version() == 10


# ---- 5. the public functions on the library ---------------------------------------------------------------------------------------------------
class StubMixer(nn.Module):
    """tanh(x W^T + b): the stand-in for a Mamba mixer (tests/golden/make_golden_add_norm.py holds the same definition)"""

    def __init__(self, dim):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(dim, dim))
        self.b = nn.Parameter(torch.zeros(dim))

    def forward(self, x, inference_params=None):
        return torch.tanh(x @ self.W.to(x.dtype).t() + self.b.to(x.dtype))


def fixture_cases():
    g = golden()
    for i, (M, N) in enumerate(g["shapes"]):
        for norm in ("ln", "rms"):
            for has_res in (0, 1):
                for prenorm in (0, 1):
                    for has_b in (0, 1):
                        yield i, norm, has_res, prenorm, has_b, f"s{i}.{norm}.r{has_res}.p{prenorm}.b{has_b}."


def check_functions_recorded(dev, dtype=torch.float32, tol=None, tol_w=None):
    """layer_norm_fn / rms_norm_fn under torch.autograd against the recorded float64 reference results; `dtype` is what the recorded
    inputs are cast to (float64 stays on the ATen composition: 1e-12 then shows the composition is the reference's definition)"""
    g = golden()
    tol = TOL[dtype] if tol is None else tol
    tol_w = TOL_W if tol_w is None else tol_w
    for i, norm, has_res, prenorm, has_b, key in fixture_cases():
        t = lambda n: torch.from_numpy(g[f"s{i}.{n}"]).to(dtype).to(dev)      # noqa: E731
        x, w = t("x").requires_grad_(), t("w").requires_grad_()
        r = t("residual").requires_grad_() if has_res else None
        b = t("b").requires_grad_() if has_b else None
        fn = AN.rms_norm_fn if norm == "rms" else AN.layer_norm_fn
        out = fn(x, w, b, residual=r, eps=float(g["eps"]), prenorm=bool(prenorm))
        outs, grads = ((out[0], out[1]), (t("dy"), t("dres"))) if prenorm else ((out,), (t("dy"),))
        assert all(o.dtype == dtype for o in outs)
        close(outs[0], torch.from_numpy(g[key + "y"]), tol, key + "y")
        if prenorm:
            close(outs[1], torch.from_numpy(g[key + "res_out"]), tol, key + "res_out")
        if prenorm and not has_res:
            assert outs[1].data_ptr() == x.data_ptr()                       # x itself, as in the reference
            outs = (outs[0], outs[1] * 1.0)
        names = [n for n, v in zip(("dx", "dw", "dres_in", "db"), (x, w, r, b)) if v is not None]
        for n, got in zip(names, torch.autograd.grad(outs, [v for v in (x, w, r, b) if v is not None], grads)):
            assert got.dtype == dtype
            close(got, torch.from_numpy(g[key + n]), tol_w if n in ("dw", "db") else tol, key + n)


def make_blocks(dev, dtype, fused, f32, norm_cls=None):
    g = golden()
    D = g["blk.h0"].shape[-1]
    blocks = []
    for j in range(2):
        blk = Block(D, StubMixer, norm_cls=norm_cls or (lambda d: nn.LayerNorm(d, eps=float(g["eps"]))), fused_add_norm=fused,
                    residual_in_fp32=bool(f32)).to(dev).to(dtype)
        with torch.no_grad():
            if isinstance(blk.norm, nn.LayerNorm):
                blk.norm.bias.copy_(torch.from_numpy(g[f"blk{j}.norm.bias"]))
            blk.norm.weight.copy_(torch.from_numpy(g[f"blk{j}.norm.weight"]))
            blk.mixer.W.copy_(torch.from_numpy(g[f"blk{j}.mix.W"]))
            blk.mixer.b.copy_(torch.from_numpy(g[f"blk{j}.mix.b"]))
        blocks.append(blk)
    return blocks


def run_blocks(blocks, dev, dtype):
    g = golden()
    x = torch.from_numpy(g["blk.h0"]).to(dtype).to(dev).requires_grad_()
    h, r = blocks[0](x)
    h, r = blocks[1](h, r)
    wrt = [x] + [p for blk in blocks for p in ((blk.norm.weight, blk.norm.bias, blk.mixer.W) if blk.norm.bias is not None
                                                  else (blk.norm.weight, blk.mixer.W))]
    dh, dr = torch.from_numpy(g["blk.dh"]).to(h.dtype).to(dev), torch.from_numpy(g["blk.dr"]).to(r.dtype).to(dev)
    return h, r, torch.autograd.grad((h, r), wrt, (dh, dr))


def check_block_recorded(dev, dtype=torch.float32, tol=None, tol_w=None, flags=(0, 1)):
    """Block(fused_add_norm=True) over two chained blocks, residual_in_fp32 both ways, against the recorded reference Block and against
    the non-fused Block of this package; dresidual flows from the second block into the first"""
    g = golden()
    tol = TOL[dtype] if tol is None else tol
    tol_w = TOL_W if tol_w is None else tol_w
    for f32 in flags:
        key = f"blk.f{f32}."
        res = {}
        for fused in (True, False):
            h, r, grads = run_blocks(make_blocks(dev, dtype, fused, f32), dev, dtype)
            assert h.dtype == dtype and r.dtype == (torch.float32 if f32 and dtype != torch.float32 else dtype), (h.dtype, r.dtype)
            what = key + ("fused." if fused else "aten.")
            close(h, torch.from_numpy(g[key + "h"]), tol, what + "h")
            close(r, torch.from_numpy(g[key + "r"]), tol, what + "r")
            close(grads[0], torch.from_numpy(g[key + "dh0"]), tol, what + "dh0")
            for j in range(2):
                close(grads[1 + 3 * j], torch.from_numpy(g[key + f"dnw{j}"]), tol_w, what + f"dnw{j}")
                close(grads[2 + 3 * j], torch.from_numpy(g[key + f"dnb{j}"]), tol_w, what + f"dnb{j}")
                close(grads[3 + 3 * j], torch.from_numpy(g[key + f"dW{j}"]), tol_w, what + f"dW{j}")
            res[fused] = (h, r, grads)
        close(res[True][0], res[False][0], tol, key + "fused vs aten h")
        close(res[True][2][0], res[False][2][0], tol, key + "fused vs aten dh0")


def check_api_rules(dev):
    """returned dtypes and Nones, RMSNorm, prenorm against non-prenorm, slices, a non-unit inner stride, zero rows, 16-bit blocks"""
    torch.manual_seed(2)
    B, Ln, D = 2, 5, 48
    for dtype in DTYPES:
        x = torch.randn(B, Ln, D, device=dev).to(dtype)
        w = (1 + 0.1 * torch.randn(D, device=dev)).to(dtype).requires_grad_()        # a 16-bit weight is cast for the kernel
        b = torch.zeros(D, device=dev, dtype=dtype).requires_grad_()
        for f32 in (False, True):
            xg = x.clone().requires_grad_()
            y, r = AN.layer_norm_fn(xg, w, b, prenorm=True, residual_in_fp32=f32)
            assert y.shape == r.shape == x.shape and y.dtype == dtype
            if f32 and dtype != torch.float32:
                assert r.dtype == torch.float32
                same_bits(r.detach(), x.float(), "the fp32 stream of a first block")
            else:
                assert r.dtype == dtype and r.data_ptr() == xg.data_ptr()
            y2 = AN.layer_norm_fn(xg, w, b, prenorm=False, residual_in_fp32=f32)
            same_bits(y.detach(), y2.detach(), "prenorm and non-prenorm y")
            gx, gw, gb = torch.autograd.grad((y, r * 1.0), (xg, w, b), (torch.ones_like(y), torch.ones_like(r)))
            assert gx.dtype == dtype and gw.dtype == dtype and gb.dtype == dtype
            # with a residual stream in fp32 its gradient is fp32, with one in x's dtype it has x's dtype
            for rdt in (dtype, torch.float32):
                res = torch.randn(B, Ln, D, device=dev).to(rdt).requires_grad_()
                y, r = AN.rms_norm_fn(xg, w, None, residual=res, prenorm=True, residual_in_fp32=f32)
                assert r.dtype == rdt and y.dtype == dtype
                gx, gres = torch.autograd.grad((y, r), (xg, res), (torch.ones_like(y), torch.ones_like(r)))
                assert gx.dtype == dtype and gres.dtype == rdt and gx.shape == gres.shape == x.shape
    # the backward hands None for a residual that was not there, and for the bias of an RMSNorm
    class Ctx:
        pass
    xg = torch.randn(3, D, device=dev).requires_grad_()
    w = torch.ones(D, device=dev)
    ctx = Ctx()
    ctx.save_for_backward = lambda *t: setattr(ctx, "saved_tensors", t)
    y = AN.LayerNormFn.forward(ctx, xg.detach(), w, None, None, 1e-5, False, False, True)
    out = AN.LayerNormFn.backward(ctx, torch.ones_like(y))
    assert len(out) == 8 and out[2] is None and all(o is None for o in out[3:]) and out[0].shape == xg.shape

    # RMSNorm: one parameter, bias registered as None; forward works (the reference's raises TypeError)
    norm = AN.RMSNorm(D, device=dev)
    assert [n for n, _ in norm.named_parameters()] == ["weight"] and norm.bias is None and norm.eps == 1e-5
    assert bool((norm.weight == 1).all())
    x = torch.randn(B, Ln, D, device=dev)
    yr, _, _, rstd = R.forward(x.reshape(-1, D), norm.weight.detach(), None, None, 1e-5, True)
    close(norm(x).reshape(-1, D), yr, TOL[torch.float32], "RMSNorm.forward")
    y, r = norm(x, residual=x, prenorm=True)
    same_bits(r, x + x, "RMSNorm prenorm residual")
    # a (B, L, D) slice of a wider tensor keeps its row stride; a non-unit inner stride arrives as a contiguous copy
    wide = torch.randn(B, Ln, D + 16, device=dev).to(torch.bfloat16)
    wv = torch.ones(D, device=dev)
    for view in (wide[..., :D], wide[..., 3:D + 3], torch.randn(B, D, Ln, device=dev).to(torch.bfloat16).transpose(1, 2)):
        assert not view.is_contiguous()
        y1, r1 = AN.layer_norm_fn(view, wv, None, residual=view, prenorm=True, residual_in_fp32=True)
        y2, r2 = AN.layer_norm_fn(view.contiguous(), wv, None, residual=view.contiguous(), prenorm=True, residual_in_fp32=True)
        same_bits(y1, y2, "a view of x: y")
        same_bits(r1, r2, "a view of x: residual_out")
    # zero rows: empty results, nothing launched
    e = torch.zeros(0, D, device=dev, requires_grad=True)
    wg = torch.ones(D, device=dev, requires_grad=True)
    y, r = AN.layer_norm_fn(e, wg, None, prenorm=True, residual_in_fp32=True)
    assert y.shape == (0, D) and r.shape == (0, D)
    ge, gwz = torch.autograd.grad(y.sum(), (e, wg))
    assert ge.shape == (0, D) and bool((gwz == 0).all())
    # 16-bit blocks with an fp32 residual stream, LayerNorm and RMSNorm, fused and not: dtypes and finite values
    for dtype in (torch.bfloat16, torch.float16):
        for norm_cls in (None, AN.RMSNorm):
            for fused in (True, False):
                h, r, grads = run_blocks(make_blocks(dev, dtype, fused, 1, norm_cls), dev, dtype)
                assert h.dtype == dtype and r.dtype == torch.float32
                assert all(bool(torch.isfinite(t.float()).all()) for t in (h, r) + tuple(grads))
    with pytest.raises(AssertionError):
        Block(D, StubMixer, norm_cls=nn.BatchNorm1d, fused_add_norm=True)


# ---- 6. one large case, GPU only --------------------------------------------------------------------------------------------------------------
def check_large(lib, dev, M=524288, N=48):
    """SegMamba's stage-0 token shape at 2 x 128^3 in bf16 with an fp32 residual stream, forward and backward, against the float64
    restatement evaluated on the device"""
    gen = torch.Generator(device=dev).manual_seed(4)
    t = lambda *s: torch.randn(*s, device=dev, generator=gen)      # noqa: E731
    c = {"x": t(M, N).to(torch.bfloat16), "residual": t(M, N), "w": 1 + 0.3 * t(N), "b": 0.5 * t(N), "dy": t(M, N).to(torch.bfloat16),
         "dres": t(M, N), "residual_dtype": None}
    o = run(lib, c, False, True, True)
    yr, s, meanr, rstdr = R.forward(c["x"], c["w"], c["b"], c["residual"], EPS, False)
    same_bits(o["res_out"], c["x"].float() + c["residual"], "large residual_out")
    close(o["y"], yr, TOL[torch.bfloat16], "large y")
    dxr, dwr, dbr = R.backward(c["dy"], o["res_out"], c["w"], meanr, rstdr, c["dres"], False)
    close(o["dx"], dxr, TOL[torch.bfloat16], "large dx")
    close(o["dres_in"], dxr, TOL[torch.bfloat16], "large dresidual_in")
    close(o["dw"], dwr, TOL_W, "large dweight")
    close(o["db"], dbr, TOL_W, "large dbias")
