"""Checks of the Mamba inner pipeline's two autograd nodes (segmamba_amd/selective_scan_interface.py), shared by the CPU emulation
build (tests/test_emu_mamba_inner.py) and the HIP library (tests/test_gpu_mamba_inner.py):

  * `check_nodes_agree`: a Mamba(v3) block through three `MambaInnerCore` nodes (SEGM_MAMBA_FUSED3=0) and through one
    `MambaInnerCore3` node compute the same thing direction by direction - every per-direction parameter gradient bit for bit;
  * `check_projection_biases`: `B_proj_bias` / `C_proj_bias` of `MambaInnerCore` against the oracle's `mamba_inner_ref`."""
import functools

import torch

from tests import helpers as H
from segmamba_amd import lib as L
from segmamba_amd import ops_raw

# name -> (d_model, input shape, nslices).  "general": the scans take the general kernels; "regular": the library's regular-shape
# condition holds for all three time orders, so MambaInnerCore3's scans run as one grid
SHAPES = {"general": (16, (2, 24, 16), 4), "regular": (48, (2, 128, 48), 8)}
# (dtype, row-streaming projections, segm_add3)
CASES = [(dtype, rows, add3) for dtype in (torch.float32, torch.bfloat16) for rows in (False, True) for add3 in (False, True)]


def case_id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else str(v)


def _run_block(monkeypatch, dev, shape, dtype, one_node):
    """forward + backward of the block -> (y, dx, {parameter name: gradient}); the one-node form needs device tensors, which is
    what the CPU build is told its host tensors are"""
    from mamba_ssm import Mamba
    from tests.golden.make_golden import named_fill
    import segmamba_amd.mamba_simple as MS
    d_model, xs, nslices = SHAPES[shape]
    m = Mamba(d_model=d_model, d_state=16, d_conv=4, expand=2, bimamba_type="v3", nslices=nslices)
    m.load_state_dict(named_fill(m.state_dict()))
    m = m.to(dev, dtype)
    g = torch.Generator().manual_seed(2)
    x = torch.randn(*xs, generator=g).to(dev, dtype).requires_grad_()
    dy = torch.randn(*xs, generator=g).to(dev, dtype)
    launches = []
    real1, real3 = ops_raw.scan_fwd, ops_raw.scan_fwd_multi
    with monkeypatch.context() as mp:
        mp.setattr(MS, "_FUSED3", one_node)
        if one_node and dev == "cpu":
            mp.setattr(L, "on_device", lambda t: True)
        mp.setattr(ops_raw, "scan_fwd", lambda *a, **k: (launches.append(1), real1(*a, **k))[1])
        mp.setattr(ops_raw, "scan_fwd_multi", lambda lib, calls: (launches.append(len(calls)), real3(lib, calls))[1])
        y = m(x)
        y.backward(dy)
    assert launches == ([3] if one_node else [1, 1, 1]), launches        # the form asked for is the form that ran
    return y.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()}


def check_nodes_agree(monkeypatch, dev, shape, dtype, rows, add3):
    from segmamba_amd import linear as LN
    from segmamba_amd import selective_scan_interface as SSI
    d_model, (batch, seqlen, _), nslices = SHAPES[shape]
    if shape == "regular":
        for order in SSI.MambaInnerCore3.ORDERS:
            ns = nslices if order == L.TIME_INTERLEAVED else 1
            assert ops_raw.scan_fused_conv_supported(L.get_lib(), batch, 2 * d_model, seqlen, ns, order), order
    monkeypatch.setattr(SSI, "_ADD3", add3)
    monkeypatch.setattr(LN, "_ROWS_HIP", rows)
    monkeypatch.setattr(LN, "_ROWS_MIN", 1)
    if dev == "cpu":
        monkeypatch.setattr(LN, "_on_device", lambda t: True)
    y3, dx3, gp3 = _run_block(monkeypatch, dev, shape, dtype, one_node=False)
    y1, dx1, gp1 = _run_block(monkeypatch, dev, shape, dtype, one_node=True)
    assert y1.dtype == y3.dtype == dtype and dx1.dtype == dx3.dtype == dtype
    for k in gp3:
        if not k.startswith(("in_proj", "out_proj")):
            assert gp1[k].dtype == gp3[k].dtype and torch.equal(gp1[k], gp3[k]), k
    if dtype == torch.float32 or not add3:
        assert torch.equal(y1, y3)
        assert torch.equal(gp1["out_proj.weight"], gp3["out_proj.weight"])
    # dx and in_proj.weight's gradient differ only in the order of the three-way sum of the dxz contributions: the bounds of
    # test_mamba_block_with_library_projections_on_emulated_kernels for the same quantities between routes
    dx1, dx3 = dx1.float(), dx3.float()
    err, bound = float((dx1 - dx3).abs().max()), 3e-2 * max(1.0, float(dx3.abs().max()))
    print(f"dx: {err:.3e} <= {bound:.3e}")
    assert err <= bound
    w1, w3 = gp1["in_proj.weight"].float(), gp3["in_proj.weight"].float()
    err, bound = float((w1 - w3).abs().max()), 5e-2 * max(1e-2, float(w3.abs().max()))
    print(f"in_proj.weight grad: {err:.3e} <= {bound:.3e}")
    assert err <= bound


# ---- projection biases ----------------------------------------------------------------------------------------------------
BIAS_NAMES = ("xz", "conv_w", "conv_b", "x_proj_w", "dt_proj_w", "A", "D", "delta_bias", "B_proj_bias", "C_proj_bias")


def _bias_inputs():
    f = H.load_golden("inner_no_out_proj.npz")
    t = {k: f[k].clone() for k in BIAS_NAMES[:8]}
    t["B_proj_bias"] = 0.3 * torch.randn(16, generator=torch.Generator().manual_seed(5))
    t["C_proj_bias"] = 0.3 * torch.randn(16, generator=torch.Generator().manual_seed(6))
    return t, f["g"].transpose(1, 2).contiguous(), torch.eye(f["conv_w"].shape[0])


def _bias_run(fn, dev):
    t, g, eye = _bias_inputs()
    t = {k: v.to(dev).requires_grad_() for k, v in t.items()}
    out = fn(t["xz"], t["conv_w"], t["conv_b"], t["x_proj_w"], t["dt_proj_w"], eye.to(dev), None, t["A"], None, None, t["D"],
             delta_bias=t["delta_bias"], B_proj_bias=t["B_proj_bias"], C_proj_bias=t["C_proj_bias"], delta_softplus=True)
    out.backward(g.to(dev))
    return out.detach(), {k: v.grad for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _bias_reference():
    from oracle import ref_ops
    return _bias_run(ref_ops.mamba_inner_ref, "cpu")


def check_projection_biases(dev, out_tol, grad_tol):
    """`mamba_inner_fn` (identity output projection) with both projection biases on the tensors of inner_no_out_proj.npz: the
    output and all ten gradients against the oracle.  `out_tol` = (rtol, atol); `grad_tol` = t: rtol t, atol t * max(1, max|ref|)"""
    from mamba_ssm.ops.selective_scan_interface import mamba_inner_fn
    ref_out, ref_grads = _bias_reference()
    out, grads = _bias_run(mamba_inner_fn, dev)
    H.assert_close(out, ref_out, *out_tol, "out")
    assert set(grads) == set(BIAS_NAMES)
    for k in BIAS_NAMES:
        H.assert_close(grads[k], ref_grads[k], grad_tol, grad_tol * max(1.0, float(ref_grads[k].abs().max())), "d" + k)
