"""CPU-only checks of the host side: the C ABI exports, the drop-in names and the checkpoint-compatibility contract."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    from segmamba_amd import build
    return build.build(verbose=False)


def test_library_exports_every_declared_symbol(built_lib):
    """include/segmamba_hip.h is the contract: every function it declares must be exported (no compute call here)."""
    hdr = open(os.path.join(ROOT, "include", "segmamba_hip.h")).read()
    declared = set(re.findall(r"\b(segm_[a-z0-9_]+)\s*\(", hdr))
    declared -= {"segm_dtype", "segm_status", "segm_time_order"}
    assert {"segm_selective_scan_fwd", "segm_selective_scan_bwd", "segm_causal_conv1d_fwd",
            "segm_causal_conv1d_bwd"} <= declared
    dll = ctypes.CDLL(built_lib)
    missing = [n for n in sorted(declared) if not hasattr(dll, n)]
    assert not missing, missing
    from segmamba_amd import lib
    assert lib.SegmLib(built_lib).missing == []
    assert set(lib.EXPORTS) == declared


def test_abi_queries_without_gpu(built_lib):
    from segmamba_amd import lib
    l = lib.SegmLib(built_lib)
    assert l.dll.segm_abi_version() == 10 == lib.header_abi_version()
    assert l.dll.segm_status_string(-3).decode().startswith("dstate")
    # SegMamba stage 0: B=2, D=96, L=64^3 -> 256-step work items, 8-step checkpoints
    assert l.dll.segm_selective_scan_default_chunk(2, 96, 262144) == 256
    # which geometries run on the regular-shape kernels (one grid for three directions, conv_weight option): every SegMamba stage does
    for dim, Lq, ns in ((96, 64 ** 3, 64), (192, 32 ** 3, 32), (384, 16 ** 3, 16), (768, 8 ** 3, 8)):
        for order, n in ((lib.TIME_FORWARD, 1), (lib.TIME_REVERSED, 1), (lib.TIME_INTERLEAVED, ns)):
            assert l.dll.segm_selective_scan_regular_shape(2, dim, 16, Lq, 0, order, n) == 1, (dim, Lq, order)
    assert l.dll.segm_selective_scan_regular_shape(2, 96, 16, 64 ** 3 - 3, 0, lib.TIME_FORWARD, 1) == 0      # ragged last chunk
    assert l.dll.segm_selective_scan_regular_shape(2, 96, 8, 64 ** 3, 0, lib.TIME_FORWARD, 1) == 0           # 8 states: general kernels
    assert l.dll.segm_selective_scan_regular_shape(2, 20, 16, 4096, 0, lib.TIME_FORWARD, 1) == 0             # 20 channels
    assert l.dll.segm_selective_scan_regular_shape(2, 96, 16, 64 ** 3, 0, lib.TIME_INTERLEAVED, 5) == 0      # 5 slices: not affine in a sub-tile
    assert l.dll.segm_selective_scan_ckpt_bytes(2, 96, 16, 262144) == 2 * (262144 // 8) * 16 * 96 * 4
    assert l.dll.segm_selective_scan_fwd_workspace_bytes(2, 96, 16, 262144, 0) > 0
    # argument errors are reported without touching the device
    a = lib.ScanFwdArgs()
    assert l.dll.segm_selective_scan_fwd(a) == -2        # SEGM_E_SHAPE
    a.batch, a.dim, a.dstate, a.n_groups, a.seqlen = 1, 8, 17, 1, 16
    assert l.dll.segm_selective_scan_fwd(a) == -3        # SEGM_E_DSTATE
    c = lib.Conv1dArgs()
    c.batch, c.dim, c.width, c.seqlen = 1, 8, 5, 16
    assert l.dll.segm_causal_conv1d_fwd(c) == -5         # SEGM_E_WIDTH


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: no module of the product may import it."""
    for pkg in ("segmamba_amd", "mamba_ssm", "causal_conv1d", "model_segmamba"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, pkg)):
            for fn in files:
                if fn.endswith(".py"):
                    src = open(os.path.join(dirpath, fn)).read()
                    assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), os.path.join(dirpath, fn)
                    assert "emu" not in re.findall(r"^\s*(?:from|import)\s+(\S+)", src, re.M)


def test_missing_library_fails_loudly(monkeypatch):
    from segmamba_amd import lib
    monkeypatch.setattr(lib, "_lib", None)
    monkeypatch.setattr(lib, "LIB_PATH", os.path.join(ROOT, "does_not_exist.so"))
    with pytest.raises(RuntimeError, match="no CPU / PyTorch fallback"):
        lib.get_lib()


def test_dropin_names_import():
    from mamba_ssm import Mamba                                                          # segmamba.py:19
    from causal_conv1d import causal_conv1d_fn, causal_conv1d_update                    # mamba_simple.py:14
    from mamba_ssm.ops.selective_scan_interface import (selective_scan_fn, mamba_inner_fn, bimamba_inner_fn,   # :19
                                                        mamba_inner_fn_no_out_proj)
    from model_segmamba.segmamba import SegMamba                                         # 0_inference.py:4
    assert all(callable(f) for f in (Mamba, causal_conv1d_fn, causal_conv1d_update, selective_scan_fn, mamba_inner_fn,
                                     bimamba_inner_fn, mamba_inner_fn_no_out_proj, SegMamba))


def test_segmamba_state_dict_matches_reference_keys(golden_dir):
    """291 keys / shapes / 67 416 196 parameters: the checkpoint-compatibility contract."""
    from model_segmamba.segmamba import SegMamba
    m = SegMamba(in_chans=4, out_chans=4, depths=[2, 2, 2, 2], feat_size=[48, 96, 192, 384])
    ours = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    ref = {}
    for line in open(os.path.join(golden_dir, "segmamba_state_dict_keys.txt")):
        k, shape = line.rstrip("\n").split(" ", 1)
        ref[k] = eval(shape)
    assert set(ours) == set(ref), (sorted(set(ref) - set(ours))[:5], sorted(set(ours) - set(ref))[:5])
    assert all(ours[k] == ref[k] for k in ref)
    assert len(ours) == 291
    assert sum(p.numel() for p in m.parameters()) == 67416196


def test_mamba_constructor_contract():
    from mamba_ssm import Mamba
    with pytest.raises(AssertionError):
        Mamba(d_model=16)                                 # reference mamba_simple.py:125: only v3 constructs
    m = Mamba(d_model=48, bimamba_type="v3", nslices=64)
    assert m.d_inner == 96 and m.dt_rank == 3
    assert m.A_log._no_weight_decay and m.D._no_weight_decay and m.dt_proj.bias._no_reinit
    assert torch.allclose(m.A_s_log.exp()[0], torch.arange(1, 17, dtype=torch.float32))
    sp = torch.nn.functional.softplus(m.dt_proj.bias)
    assert (sp >= 1e-3 * 0.99).all() and (sp <= 0.1 * 1.01).all()
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 100, 48))                        # L % nslices != 0


def test_split_k_projection_gemms_match_torch(monkeypatch):
    """linear.py: split-K weight gradients / layout-agnostic 1x1x1 convolution == F.linear / F.conv3d autograd."""
    import torch.nn.functional as F
    from segmamba_amd import linear as Lm
    monkeypatch.setattr(Lm, "_FORCE_SPLIT", True)
    monkeypatch.setattr(Lm, "_MIN_K", 16)
    monkeypatch.setattr(Lm, "_SLAB", 8)
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(96, 5, generator=g), torch.randn(96, 3, generator=g)
    assert Lm._split(96) == 12
    assert torch.allclose(Lm.tn_matmul(a, b), a.t() @ b, atol=1e-4)
    assert torch.allclose(Lm.tn_matmul(a[:, 1:4], b[:, :2]), a[:, 1:4].t() @ b[:, :2], atol=1e-4)      # column slices
    x = torch.randn(2, 5, 4, 4, 4, generator=g, requires_grad=True)
    w = torch.randn(7, 5, generator=g, requires_grad=True)
    bias = torch.randn(7, generator=g, requires_grad=True)
    ref = F.conv3d(x, w.view(7, 5, 1, 1, 1), bias)
    gy = torch.randn(ref.shape, generator=g)
    gref = torch.autograd.grad(ref, (x, w, bias), gy)
    for xin in (x, x.detach().permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3).requires_grad_()):
        y = Lm.pointwise(xin, w, bias)
        assert y.is_contiguous() and torch.allclose(y, ref, atol=1e-5)
        for got, want in zip(torch.autograd.grad(y, (xin, w, bias), gy), gref):
            assert torch.allclose(got, want, atol=1e-4)
    xl = torch.randn(3, 32, 5, generator=g, requires_grad=True)
    y, ref = Lm.linear_cl(xl, w, bias), F.linear(xl, w, bias)
    gy = torch.randn(ref.shape, generator=g)
    for got, want in zip(torch.autograd.grad(y, (xl, w, bias), gy), torch.autograd.grad(ref, (xl, w, bias), gy)):
        assert torch.allclose(got, want, atol=1e-4)


def test_patch_convs_match_torch():
    import torch.nn.functional as F
    from segmamba_amd import fused_norm
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 4, 6, 8, generator=g, requires_grad=True)
    w = torch.randn(5, 3, 2, 2, 2, generator=g, requires_grad=True)
    b = torch.randn(5, generator=g, requires_grad=True)
    y, ref = fused_norm.patch_conv3d(x, w, b, 2), F.conv3d(x, w, b, 2)
    gy = torch.randn(ref.shape, generator=g)
    assert torch.allclose(y, ref, atol=1e-5)
    for got, want in zip(torch.autograd.grad(y, (x, w, b), gy), torch.autograd.grad(ref, (x, w, b), gy)):
        assert torch.allclose(got, want, atol=1e-4)
    wt = torch.randn(3, 5, 2, 2, 2, generator=g, requires_grad=True)
    y, ref = fused_norm.patch_conv_transpose3d(x, wt, b, 2), F.conv_transpose3d(x, wt, b, 2)
    gy = torch.randn(ref.shape, generator=g)
    assert torch.allclose(y, ref, atol=1e-5)
    for got, want in zip(torch.autograd.grad(y, (x, wt, b), gy), torch.autograd.grad(ref, (x, wt, b), gy)):
        assert torch.allclose(got, want, atol=1e-4)


def test_conv_dispatcher_routings_are_the_same_convolution():
    """conv3d.py: the vendor routes of the data and the weight gradient, the cat-free decoder convolution and the bias path equal
    torch's conv3d autograd."""
    import torch.nn.functional as F
    from segmamba_amd import conv3d as C3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(1, 96, 4, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(48, 96, 3, 3, 3, generator=g, dtype=torch.float64, requires_grad=True) * 0.1
    ref = F.conv3d(x, w, None, 1, 1)
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    gx, gw = torch.autograd.grad(ref, (x, w), dy)
    xd, wd = x.detach(), w.detach()
    assert torch.allclose(C3._dgrad_native(dy, wd, xd, 1), gx, atol=1e-10)
    assert torch.allclose(C3._wgrad_native(xd, dy, wd, 1), gw, atol=1e-10)
    # cat-free decoder convolution == convolution of the concatenation (unetr_block.py:82-84), values and gradients
    a = torch.randn(1, 48, 4, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(1, 48, 4, 5, 6, generator=g, dtype=torch.float64, requires_grad=True)
    y = C3.conv3d_same_cat((a, b), w)
    ref2 = F.conv3d(torch.cat((a, b), 1), w, None, 1, 1)
    assert torch.allclose(y, ref2, atol=1e-10)
    for got, want in zip(torch.autograd.grad(y, (a, b, w), dy), torch.autograd.grad(ref2, (a, b, w), dy)):
        assert torch.allclose(got, want, atol=1e-10)
    # bias path of the autograd node (CPU tensors take the plain library call)
    bias = torch.randn(48, generator=g, dtype=torch.float64, requires_grad=True)
    yb = C3.conv3d_same(x, w, bias)
    assert torch.allclose(yb, F.conv3d(x, w, bias, 1, 1), atol=1e-10)


def test_fused_clip_sgd_host_logic_matches_torch_sgd():
    """FusedClipSGD (ATen path on CPU tensors): clip_grad_norm_ + SGD(nesterov) semantics, torch-compatible state."""
    from segmamba_amd.train_ops import FusedClipSGD, cross_entropy
    torch.manual_seed(0)
    net_a = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    net_b = torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))
    net_b.load_state_dict(net_a.state_dict())
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-2, nesterov=True)
    opt_a = torch.optim.SGD(net_a.parameters(), **kw)
    opt_b = FusedClipSGD(net_b.parameters(), max_norm=0.3, **kw)
    for step in range(4):
        x, y = torch.randn(8, 6), torch.randint(0, 3, (8,))
        for net, opt in ((net_a, opt_a), (net_b, opt_b)):
            opt.zero_grad(set_to_none=True)
            loss = torch.nn.functional.cross_entropy(net(x), y) if net is net_a else cross_entropy(net(x), y)
            loss.backward()
            if net is net_a:
                torch.nn.utils.clip_grad_norm_(net.parameters(), 0.3)
            opt.step()
    for pa, pb in zip(net_a.parameters(), net_b.parameters()):
        assert (pa - pb).abs().max() <= 1e-6
    opt_c = torch.optim.SGD(net_a.parameters(), **kw)
    opt_c.load_state_dict(opt_b.state_dict())              # checkpoints interchange with torch.optim.SGD
    bufs = [opt_c.state[p]["momentum_buffer"] for p in net_a.parameters()]
    assert all((b - opt_b.state[p]["momentum_buffer"]).abs().max() == 0 for b, p in zip(bufs, net_b.parameters()))


def test_argument_errors_of_the_newer_entry_points_without_gpu(built_lib):
    """every entry point validates its arguments on the host and returns a SEGM_E_* code before touching the device"""
    from segmamba_amd import lib
    l = lib.SegmLib(built_lib)
    d = l.dll
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    p16 = (p + 15) & ~15

    a = lib.Conv3dFwdArgs()
    a.batch, a.cin, a.cout, a.depth, a.height, a.width, a.dtype = 1, 48, 32, 2, 2, 8, lib.SEGM_BF16
    a.x = a.y = a.w_packed = p16
    a.x_stride_b = a.x_stride_c = a.x_stride_z = a.x_stride_y = 8
    a.y_stride_b = a.y_stride_c = a.y_stride_z = a.y_stride_y = 8
    for flags in (2, 8, 1 | 2, 4, 2 | 8, 64):              # chain / chain32 / accumulate need cout % 48 == 0; pitch48 needs chain; unknown bit
        a.flags = flags
        assert d.segm_conv3d_k3_fwd(a) == -2, flags
    a.flags, a.dtype = 0, lib.SEGM_F32
    assert d.segm_conv3d_k3_fwd(a) == -4                   # 16-bit only

    s = lib.SgdArgs()
    assert d.segm_sgd_clip_step(s) == 0                    # no tensors: nothing to do
    s.ntensors = 1
    assert d.segm_sgd_clip_step(s) == -1                   # NULL lists
    ne = (ctypes.c_int64 * 1)(100)
    ptrs = (ctypes.c_void_p * 1)(p16)
    s.params = s.grads = s.momenta = ctypes.cast(ptrs, ctypes.c_void_p)
    s.numel = ctypes.cast(ne, ctypes.c_void_p)
    assert d.segm_sgd_clip_step(s) == -6                   # workspace missing
    assert d.segm_sgd_clip_step_workspace_bytes(1, ctypes.cast(ne, ctypes.c_void_p)) == (1 + 4) * 4

    c = lib.CrossEntropyArgs()
    c.batch, c.classes, c.dtype, c.spatial = 1, 17, lib.SEGM_F32, 8
    assert d.segm_cross_entropy(c) == -2                   # at most 16 classes
    c.classes = 4
    assert d.segm_cross_entropy(c) == -1                   # NULL tensors
    assert d.segm_cross_entropy_partials(2, 1000) == (2000 + 255) // 256

    u = lib.Conv1dUpdateArgs()
    u.batch, u.dim, u.width, u.dtype = 1, 8, 5, lib.SEGM_F32
    assert d.segm_causal_conv1d_update(u) == -5            # width outside [2, 4]
    t = lib.StateUpdateArgs()
    t.batch, t.dim, t.dstate, t.dtype, t.state_dtype = 1, 8, 257, lib.SEGM_F32, lib.SEGM_F32
    assert d.segm_selective_state_update(t) == -3          # dstate above the reference's 256
    t.dstate, t.state_dtype = 16, 9
    assert d.segm_selective_state_update(t) == -4

    g = lib.LinearArgs()
    g.rows, g.k, g.n, g.dtype = 64, 2056, 48, lib.SEGM_BF16
    assert d.segm_linear_rows(g) == -2                     # k <= 2048 (round 6; 192 before)
    g.k, g.n = 48, 50
    assert d.segm_linear_rows(g) == -2                     # n % 4
    g.n, g.dtype = 48, lib.SEGM_F32
    assert d.segm_linear_rows(g) == -4
    g.dtype = lib.SEGM_BF16
    assert d.segm_linear_rows(g) == -1                     # NULL tensors
    g.x = g.w = g.y = p16
    g.x_stride_row, g.y_stride_row = 40, 48
    assert d.segm_linear_rows(g) == -2                     # x rows shorter than k

    q = lib.PointwiseArgs()
    q.batch, q.cin, q.cout, q.dtype, q.spatial, q.w_stride = 1, 48, 48, lib.SEGM_BF16, 100, 48
    assert d.segm_pointwise_cf(q) == -2                    # voxels not a multiple of 64
    q.spatial, q.cin, q.w_stride = 128, 100, 104
    assert d.segm_pointwise_cf(q) == -2                    # cin <= 96
    q.cin, q.w_stride = 48, 44
    assert d.segm_pointwise_cf(q) == -2                    # weight rows shorter than cin / not a multiple of 8
    q.w_stride, q.dtype = 48, lib.SEGM_F32
    assert d.segm_pointwise_cf(q) == -4
    q.dtype = lib.SEGM_BF16
    assert d.segm_pointwise_cf(q) == -1                    # NULL tensors
    q.x = q.w = q.y = p16
    q.x_stride_b, q.x_stride_c, q.y_stride_b, q.y_stride_c = 48 * 128, 130, 48 * 128, 128
    assert d.segm_pointwise_cf(q) == -2                    # channel rows of x not 16-byte aligned

    m = lib.StemArgs()
    m.batch, m.cout, m.din, m.hin, m.win, m.dtype = 1, 48, 4, 4, 48, lib.SEGM_BF16
    assert d.segm_stem_conv_fwd(m) == -2                   # width not a multiple of 32
    m.win, m.cout = 64, 64
    assert d.segm_stem_conv_fwd(m) == -2                   # cout <= 48
    m.cout, m.hin = 48, 6
    assert d.segm_stem_conv_fwd(m) == -2                   # 8 tiles = TX x TY must tile the output rows (wout 32: TY 4, hout 3)
    m.hin, m.dtype = 8, lib.SEGM_F32
    assert d.segm_stem_conv_fwd(m) == -4
    m.dtype = lib.SEGM_BF16
    assert d.segm_stem_conv_fwd(m) == -1                   # NULL tensors

    q = lib.WgradGemmArgs()
    q.layout, q.dtype, q.m, q.n, q.k, q.batch = 2, lib.SEGM_BF16, 48, 48, 4096, 1
    assert d.segm_wgrad_gemm(q) == -2                      # unknown layout
    q.layout, q.m = 1, 128
    assert d.segm_wgrad_gemm(q) == -2                      # NT: m, n <= 96
    q.m, q.k = 48, 4100
    assert d.segm_wgrad_gemm(q) == -2                      # NT: k % 32 == 0
    q.k, q.dtype = 4096, lib.SEGM_F32
    assert d.segm_wgrad_gemm(q) == -4
    q.dtype, q.layout = lib.SEGM_BF16, 0
    q.a_stride_row, q.b_stride_row = 40, 48
    assert d.segm_wgrad_gemm(q) == -2                      # TN: a row shorter than m
    q.a_stride_row = 48
    assert d.segm_wgrad_gemm(q) == -1                      # NULL tensors
    q.a = q.b = q.out = p16
    need = d.segm_wgrad_gemm_workspace_bytes(0, 48, 48, 4096, 1)
    assert need > 0 and need % (48 * 48 * 4) == 0          # whole per-wave partials
    q.workspace, q.workspace_bytes = p16, need - 1
    assert d.segm_wgrad_gemm(q) == -6                      # workspace too small

    g = lib.StemWgradArgs()
    g.batch, g.cout, g.din, g.hin, g.win, g.dtype = 1, 48, 4, 4, 96, lib.SEGM_BF16
    assert d.segm_stem_conv_wgrad(g) == -2                 # rows of 1, 2 or 4 k-steps: width 64, 128 or 256
    g.win, g.din = 64, 3
    assert d.segm_stem_conv_wgrad(g) == -2                 # even extents
    g.din, g.dtype = 4, lib.SEGM_F32
    assert d.segm_stem_conv_wgrad(g) == -4
    g.dtype = lib.SEGM_BF16
    assert d.segm_stem_conv_wgrad(g) == -1                 # NULL tensors
    g.x4 = g.dy = g.dw_packed = p16
    need = d.segm_stem_conv_wgrad_workspace_bytes(1, 48, 4, 4)
    assert need == 1 * 7 * 7 * 48 * 32 * 4                 # 4 output rows: one slab of partials
    g.workspace, g.workspace_bytes = p16, need - 1
    assert d.segm_stem_conv_wgrad(g) == -6                 # workspace too small


def test_conv_routing_is_a_table_not_a_timing_run():
    """which kernel a 3x3x3 layer takes must not depend on a per-process timing run (ranks could differ, results
    were not reproducible run to run, nothing of it can happen under graph capture).  Routing is a pure function of the shape
    (conv3d._table_choice, from profiles/r02_bench_variants.log); the module has no timing run and no state one could fill."""
    import inspect
    from segmamba_amd import conv3d
    lib = [(False, False, False), (True, False, False), (True, True, False), (False, False, True)]
    fwd = [None, None] + lib                                  # native, blocked, the four library variants
    for width, want in ((128, (True, True, False)), (64, (False, False, True)), (32, (False, False, True)), (16, (False, False, True))):     # 64^3: the 32-wide kernel since round 4
        assert fwd[conv3d._table_choice("fwd", width, fwd)] == want
        assert ([None] + fwd)[conv3d._table_choice("dgrad", width, [None] + fwd)] == want
    assert conv3d._table_choice("fwd", 8, fwd) == 0 and conv3d._table_choice("dgrad", 8, [None] + fwd) == 0     # 8^3: vendor GEMM route
    assert conv3d._table_choice("fwd", 64, [None]) == 0                          # nothing of the library applies: vendor route
    assert conv3d._table_choice("fwd", 64, [None, lib[0]]) == 1                  # only the plain library kernel applies
    assert conv3d._table_choice("wgrad", 128, [None, None, "mfma"]) == 2 and conv3d._table_choice("wgrad", 16, [None, "mfma"]) == 1
    assert conv3d._table_choice("wgrad", 8, [None, None, "mfma"]) == 0
    # the same decision in every process: there is no timing state to consult and nothing that could time a kernel
    assert not any(hasattr(conv3d, name) for name in ("_TUNE", "_cache", "_time"))
    source = inspect.getsource(conv3d)
    assert "synchronize" not in source and "elapsed_time" not in source


_ROUTE_NAMES = {None: "vendor", (False, False, False): "plain", (True, False, False): "chain", (True, True, False): "chain_pitch48",
                (False, False, True): "chain32", "mfma": "mfma", "cube": "cube"}


def test_conv_routes_equal_the_recorded_table(monkeypatch):
    """Which kernel a 3x3x3 layer takes is what it was before the routing became one function: for every (width, Cin, Cout) of the
    grid the forward / data-gradient / weight-gradient routes equal tests/conv_routes_recorded.json, recorded from the dispatcher
    that still built closures per call ("W:Cin>Cout" -> "fwd/dgrad/wgrad").  Sections: bf16 over the whole grid (channels capped per
    width so that the untouched torch.empty volumes stay below ~0.5 GB); fp16; fp32 (vendor everywhere); x with a padded channel
    stride (ops_raw.volume_empty's 192 elements, which the kernels take, and 4 elements, which they do not); the cube kernels
    switched off.  No GPU: the applicability predicates read shapes, strides and dtypes only."""
    import json
    from segmamba_amd import conv3d as C3
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_routes_recorded.json")) as f:
        recorded = json.load(f)

    def volume(c, width, dtype, pad=0):
        s = width ** 3
        return torch.empty(1, c, s + pad, dtype=dtype)[:, :, :s].view(1, c, width, width, width)

    def routes(width, cin, cout, dtype, pad):
        x, dy, w = volume(cin, width, dtype, pad), volume(cout, width, dtype), torch.empty(cout, cin, 3, 3, 3, dtype=dtype)
        lists = (("fwd", C3._fwd_variants(x, w)), ("dgrad", C3._fwd_variants(dy, w, flipped=True)), ("wgrad", C3._wgrad_variants(x, dy, w)))
        for _, variants in lists:                        # the lists themselves: vendor first, no duplicates
            assert variants[0] is None and len(set(variants)) == len(variants)
        return "/".join(_ROUTE_NAMES[variants[C3._table_choice(kind, width, variants)]] for kind, variants in lists)

    sections = {"bf16": (torch.bfloat16, 0, True), "fp16": (torch.float16, 0, True), "fp32": (torch.float32, 0, True),
                "bf16_x_channel_pad_192": (torch.bfloat16, 192, True), "bf16_x_channel_pad_4": (torch.bfloat16, 4, True),
                "bf16_cube_off": (torch.bfloat16, 0, False)}
    assert set(recorded) == set(sections)
    caps = {128: 96, 64: 192, 32: 384, 24: 96}
    grid = {f"{width}:{cin}>{cout}" for width in (128, 64, 32, 24, 16, 8, 4) for cin in (4, 32, 48, 64, 96, 192, 384, 768)
            for cout in (16, 48, 64, 96, 192, 384, 768) if max(cin, cout) <= caps.get(width, 768)}
    assert set(recorded["bf16"]) == grid and set(recorded["bf16_cube_off"]) == grid
    for name, (dtype, pad, cube) in sections.items():
        monkeypatch.setattr(C3, "_CUBE", cube)
        monkeypatch.setattr(C3, "_CUBE_WGRAD", cube)
        for shape, want in recorded[name].items():
            width, cin, cout = (int(t) for t in re.split("[:>]", shape))
            assert routes(width, cin, cout, dtype, pad) == want, (name, shape)
    spot = {"16:64>16": "vendor/plain/vendor", "16:96>16": "plain/chain32/vendor", "16:96>48": "chain32/chain32/mfma",
            "16:96>96": "cube/cube/mfma", "16:384>384": "cube/cube/cube", "8:48>96": "vendor/vendor/vendor",
            "8:32>96": "cube/vendor/vendor", "8:96>96": "cube/cube/vendor", "8:96>192": "cube/cube/cube"}
    assert all(recorded["bf16"][k] == v for k, v in spot.items())
    assert {v for k, v in recorded["bf16"].items() if k.startswith("4:")} == {"vendor/vendor/vendor"}
    assert set(recorded["fp32"].values()) == {"vendor/vendor/vendor"}


def test_conv_table_small_volumes_follow_the_logged_winners():
    """conv3d._table_choice sends 3x3x3 layers narrower than 16 voxels to candidate 0 (the vendor convolution) - which is what the
    timing-based dispatcher had chosen for every 8^3 layer on the MI355X (profiles/r02_bench_variants.log: '-> 0' on each
    8x8x8 line); wider volumes take a library kernel whenever one is offered."""
    import re
    from segmamba_amd import conv3d as C3
    log = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r02_bench_variants.log")
    seen = 0
    for line in open(log):
        m = re.match(r"\[conv3d autotune\] \('(\w+)', \((\d+), (\d+), (\d+), (\d+), (\d+)\).* -> (\d+)\s*$", line)
        if not m or int(m.group(6)) >= 16 or "3, 3, 3)" not in line:
            continue
        seen += 1
        assert int(m.group(7)) == 0, line
        assert C3._table_choice(m.group(1), int(m.group(6)), [None, None, (True, True, False), "mfma"]) == 0
    assert seen >= 3
    variants = [None, None, (True, False, False), (True, True, False), (False, False, True)]
    assert variants[C3._table_choice("fwd", 128, variants)] == (True, True, False)
    assert variants[C3._table_choice("dgrad", 32, variants)] == (False, False, True)
    assert C3._table_choice("wgrad", 64, [None, None, "mfma"]) == 2


def test_graft_entry_build_runs_and_checks_the_header_abi():
    """`__graft_entry__.build()` is the driver's "does it build" check: it must pass on the tree as it is (round 4 found it
    comparing the library's ABI number with a stale literal) and take the expected number from include/segmamba_hip.h."""
    import importlib
    ge = importlib.import_module("__graft_entry__")
    ge.build()
    from segmamba_amd import lib as L
    assert L.header_abi_version() == L.SegmLib(L.LIB_PATH).dll.segm_abi_version()


def test_bench_gpu_state_parses_rocm_smi_text(monkeypatch):
    """bench.gpu_state: the clock / power lines of `rocm-smi --showclocks --showpower --showtemp --showperflevel` as the MI355X
    boxes print them (sclk level 'S' when idle, a digit under load); never raises when the tool is missing"""
    import subprocess
    import bench
    sample = ("GPU[0]\t\t: mclk clock level: 0: (2000Mhz)\nGPU[0]\t\t: sclk clock level: S: (99Mhz)\n"
              "GPU[0]\t\t: Current Socket Graphics Package Power (W): 676.0\nGPU[0]\t\t: Temperature (Sensor junction) (C): 46.0\n"
              "GPU[0]\t\t: Performance Level: auto\n")

    class R:
        stdout = sample
    monkeypatch.setattr(subprocess, "run", lambda *a, **k: R())
    st = bench.gpu_state(0)
    assert st == {"sclk_mhz": 99, "mclk_mhz": 2000, "power_w": 676.0, "temp_c": 46.0, "perf_level": "auto"}, st

    def boom(*a, **k):
        raise FileNotFoundError("rocm-smi")
    monkeypatch.setattr(subprocess, "run", boom)
    assert "error" in bench.gpu_state(0)
