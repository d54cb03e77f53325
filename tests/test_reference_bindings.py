"""`segmamba_amd.native_stubs.{selective_scan_cuda, causal_conv1d_cuda}` - the two native module names
the reference's `mamba_ssm/ops/selective_scan_interface.py` imports (:9-11) - driven with the call sequences of that file's
autograd Functions (SelectiveScanFn :36-67, MambaInnerFnNoOutProj :155-289), against what the reference's own
`selective_scan_ref` / `mamba_inner_ref` computed on the same inputs (tests/golden/make_golden.py):

  * without a GPU: on the CPU emulation build of the kernels (tests/emu), output and every gradient;
  * on the GPU (-m gpu): on the HIP library, against the oracle, with the in-place / recompute variants of the backward.
"""
import pytest
import torch
import torch.nn.functional as F


class _ScanFn(torch.autograd.Function):
    """the native calls of SelectiveScanFn: fwd -> (out, x, out_z); bwd(..., dout, x, out, dz=None, softplus, False)"""

    @staticmethod
    def forward(ctx, u, delta, A, B, C, D, z, delta_bias):
        from segmamba_amd.native_stubs import selective_scan_cuda
        if B.dim() == 3:                                                  # "b dstate l -> b 1 dstate l"
            B, C = B.unsqueeze(1).contiguous(), C.unsqueeze(1).contiguous()
            ctx.squeeze = True
        else:
            ctx.squeeze = False
        out, x, out_z = selective_scan_cuda.fwd(u, delta, A, B, C, D, z, delta_bias, True)
        ctx.save_for_backward(u, delta, A, B, C, D, z, delta_bias, x, out)
        return out_z, x[:, :, -1, 1::2]                                  # last state: the odd entries of the final checkpoint

    @staticmethod
    def backward(ctx, dout, dlast):
        from segmamba_amd.native_stubs import selective_scan_cuda
        u, delta, A, B, C, D, z, delta_bias, x, out = ctx.saved_tensors
        du, ddelta, dA, dB, dC, dD, ddb, dz = selective_scan_cuda.bwd(u, delta, A, B, C, D, z, delta_bias, dout.contiguous(), x,
                                                                        out, None, True, False)
        if ctx.squeeze:
            dB, dC = dB.squeeze(1), dC.squeeze(1)
        return du, ddelta, dA, dB, dC, dD, dz, ddb


class _ConvFn(torch.autograd.Function):
    """the native calls of the depthwise causal convolution with SiLU: causal_conv1d_fwd / causal_conv1d_bwd(dx=None)"""

    @staticmethod
    def forward(ctx, x, weight, bias):
        from segmamba_amd.native_stubs import causal_conv1d_cuda
        ctx.save_for_backward(x, weight, bias)
        return causal_conv1d_cuda.causal_conv1d_fwd(x, weight, bias, True)

    @staticmethod
    def backward(ctx, dout):
        from segmamba_amd.native_stubs import causal_conv1d_cuda
        x, weight, bias = ctx.saved_tensors
        dx, dw, db = causal_conv1d_cuda.causal_conv1d_bwd(x, weight, bias, dout.contiguous(), None, True)
        return dx, dw, db


def _inner_no_out_proj(xz, conv_w, conv_b, x_proj_w, dt_proj_w, A, D, delta_bias):
    """MambaInnerFnNoOutProj's data flow around the two native modules (the projections as torch ops)"""
    L_ = xz.shape[-1]
    R_, N_ = dt_proj_w.shape[1], A.shape[1]
    x, z = xz.chunk(2, dim=1)
    conv = _ConvFn.apply(x.contiguous(), conv_w[:, 0], conv_b)
    x_dbl = F.linear(conv.transpose(1, 2).reshape(-1, conv.shape[1]), x_proj_w)                    # (b l) (r + 2n)
    delta = (dt_proj_w @ x_dbl[:, :R_].t()).reshape(-1, xz.shape[0], L_).transpose(0, 1).contiguous()   # b d l
    Bm = x_dbl[:, R_:R_ + N_].reshape(xz.shape[0], L_, N_).transpose(1, 2).contiguous()             # b n l
    Cm = x_dbl[:, R_ + N_:].reshape(xz.shape[0], L_, N_).transpose(1, 2).contiguous()
    return _ScanFn.apply(conv, delta, A, Bm, Cm, D, z.contiguous(), delta_bias)[0]


def _check_grads(leaves, f, names):
    for t, name in zip(leaves, names):
        ref = f["d" + name]
        scale = max(1.0, float(ref.abs().max()))
        assert (t.grad - ref).abs().max() <= 1e-3 * scale, name


def test_stub_modules_with_the_reference_call_sequences_on_the_emulator(monkeypatch):
    from tests import emu_util
    from tests import helpers as H
    if not emu_util.emu_available():
        pytest.skip("no host clang for the emulation build")
    from segmamba_amd import lib as L
    monkeypatch.setattr(L, "_lib", emu_util.emu_lib())
    monkeypatch.setattr(L, "on_device", lambda t: True)
    # --- standalone op at the reference test's distributions, G = 1 and 2
    for G in (1, 2):
        f = H.load_golden(f"scan_L256_G{G}.npz")
        names = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")
        leaves = [f[k].clone().requires_grad_() for k in names]
        out, last = _ScanFn.apply(*leaves)
        assert torch.allclose(out, f["out"], rtol=1e-3, atol=1e-3)
        assert torch.allclose(last, f["last_state"], rtol=1e-3, atol=1e-3)
        out.backward(f["g"])
        _check_grads(leaves, f, names)
    # --- the fused function SegMamba uses, against mamba_inner_ref without the out-projection
    f = H.load_golden("inner_no_out_proj.npz")
    names = ("xz", "conv_w", "conv_b", "x_proj_w", "dt_proj_w", "A", "D", "delta_bias")
    leaves = [f[k].clone().requires_grad_() for k in names]
    y = _inner_no_out_proj(*leaves)
    assert torch.allclose(y, f["out"], rtol=1e-3, atol=1e-3)
    y.backward(f["g"])
    _check_grads(leaves, f, names)


@pytest.mark.gpu
def test_stub_modules_with_the_reference_call_sequences_on_the_gpu():
    """what SelectiveScanFn.forward / backward and MambaInnerFnNoOutProj do with the native modules, on the HIP library"""
    from oracle import ref_ops
    from segmamba_amd.native_stubs import causal_conv1d_cuda, selective_scan_cuda
    from tests import helpers as H
    dev = "cuda"
    c = H.scan_case(2, 96, 16, 1536, seed=5)
    ref = H.scan_oracle(c)
    t = {k: (v.to(dev) if v is not None else None) for k, v in c.items()}
    B4, C4 = t["B"][:, None].contiguous(), t["C"][:, None].contiguous()            # "b dstate l -> b 1 dstate l" (:31-36)
    out, x, out_z = selective_scan_cuda.fwd(t["u"], t["delta"], t["A"], B4, C4, t["D"], t["z"], t["delta_bias"], True)
    assert isinstance(x, torch.Tensor)                                             # ctx.save_for_backward(..., x, out)
    last = x[:, :, -1, 1::2]                                                       # :40
    H.assert_close(out_z, ref["out"], 1e-3, 1e-3, "stub fwd out_z")
    H.assert_close(last, ref["last_state"], 1e-3, 1e-3, "stub fwd last_state")
    x_saved = x.detach()[...]                                                      # what autograd hands back: same storage
    du, ddelta, dA, dB, dC, dD, ddb, dz = selective_scan_cuda.bwd(t["u"], t["delta"], t["A"], B4, C4, t["D"], t["z"],
                                                                    t["delta_bias"], t["g"], x_saved, out, None, True, False)
    res = {"out": out_z, "last_state": last, "du": du, "ddelta": ddelta, "dA": dA, "dB": dB.squeeze(1), "dC": dC.squeeze(1),
           "dD": dD, "dz": dz, "ddelta_bias": ddb}
    H.check_scan(res, ref, torch.float32, "stub modules")
    # dz pre-allocated as a view into a (B, 2D, L) buffer + recompute_out_z (:244-247)
    dxz = torch.empty(2, 192, 1536, device=dev)
    r2 = selective_scan_cuda.bwd(t["u"], t["delta"], t["A"], B4, C4, t["D"], t["z"], t["delta_bias"], t["g"], x_saved, out,
                                 dxz[:, 96:], True, True)
    assert len(r2) == 9 and r2[7].data_ptr() == dxz[:, 96:].data_ptr()
    H.assert_close(dxz[:, 96:], ref["dz"], 1e-3, 1e-3, "dz in place")
    H.assert_close(r2[8], ref["out"], 1e-3, 1e-3, "recomputed out_z")
    # conv module: fwd, bwd with pre-allocated dx, 16-bit weights (causal_conv1d.cpp:136-137)
    g = torch.Generator().manual_seed(3)
    xx = torch.randn(2, 64, 300, generator=g)
    w, b = torch.randn(64, 4, generator=g), torch.randn(64, generator=g)
    go = torch.randn(2, 64, 300, generator=g)
    xr, wr, br = xx.clone().requires_grad_(), w.clone().requires_grad_(), b.clone().requires_grad_()
    yr = ref_ops.causal_conv1d_ref(xr, wr, br, "silu")
    yr.backward(go)
    y = causal_conv1d_cuda.causal_conv1d_fwd(xx.to(dev), w.to(dev), b.to(dev), True)
    H.assert_close(y, yr, 1e-3, 1e-3, "conv stub fwd")
    dxbuf = torch.empty(2, 128, 300, device=dev)
    dx, dw, dbias = causal_conv1d_cuda.causal_conv1d_bwd(xx.to(dev), w.to(dev), b.to(dev), go.to(dev), dxbuf[:, :64], True)
    assert dx.data_ptr() == dxbuf.data_ptr()
    H.assert_close(dx, xr.grad, 1e-3, 1e-3, "conv stub dx")
    H.assert_close(dw, wr.grad, 1e-3, 1e-3 * float(wr.grad.abs().max()), "conv stub dw")
    H.assert_close(dbias, br.grad, 1e-3, 1e-3 * float(br.grad.abs().max()), "conv stub db")
    y16 = causal_conv1d_cuda.causal_conv1d_fwd(xx.to(dev).bfloat16(), w.to(dev).bfloat16(), b.to(dev).bfloat16(), True)
    yr16 = ref_ops.causal_conv1d_ref(xx.bfloat16(), w.bfloat16().float(), b.bfloat16().float(), "silu")
    H.assert_close(y16, yr16, 1e-2, 1e-2, "conv stub fwd, bf16 weights")
    with pytest.raises(RuntimeError):
        selective_scan_cuda.fwd(t["u"], t["delta"], torch.randn(96, 32, device=dev), B4, C4, t["D"], t["z"], t["delta_bias"], True)
