"""Exact-arithmetic parity of the 3x3x3 convolution kernels (csrc/conv3d_fwd.hip, conv3d_cube.hip, conv3d_wgrad.hip and the routing in
segmamba_amd/conv3d.py), shared by tests/test_emu_conv_exact.py (the kernel sources on the CPU emulator) and
tests/test_gpu_conv_exact.py (the HIP library).

Every one of these kernels multiplies 16-bit operands exactly (MFMA) and accumulates in fp32.  With small-integer operands every
product and every partial sum is an integer below 2^24, so the fp32 result is exact in ANY summation order - any plan, split, chain
order or reduction tree - and the correct output is one bit pattern: the checks are `torch.equal`, no tolerance.  A weight element
that is never applied, one halo element from the wrong voxel, one tap masked wrongly at one border: each moves some output by at
least 1 and fails the check, where a max-norm tolerance of 1e-2 of the largest value lets it pass.

  operands    activations / gradients: integers in {-2..2}, density 0.5; weights in {-1, 0, 1} with a density per shape (`_wdens`);
              bias: integers in fp32; a fixed seed per case.  All exact in bf16 and fp16.
  reference   torch.nn.functional.conv3d and its autograd in fp64 ON THE CPU from the same integers (`_fwd_case`, `_wgrad_case`,
              `_dispatch_case`: computed once per case and shared by the checks that need it, never modified).  Not a device ATen call:
              the vendor's algorithm is not ours to know and a Winograd or FFT solver is not exact on integers.
  conditions  asserted on the REFERENCE before anything is asserted about a kernel (`_need_16bit`, `_need_stats`): 16-bit outputs
              max|ref| <= 128 (integers up to 256 are exact in bf16, 2048 in fp16); statistics: per (batch, channel) instance
              sum(ref^2) < 2^24; weight gradients max|ref| < 2^24.
  rounded     `check_*_rounded_once`: dense operands in {-8..8} x {-4..4}, |ref| in the thousands: the 16-bit result must be the
              exact sum rounded ONCE (round to nearest even), `ref.float().to(dtype)`; in accumulate mode (old + conv) rounded once.

A mismatch raises with the count of differing elements and the first few indices with got / want and their position inside the
8 x 8 x 8 cube or the row kernels' x block (`_same`).
"""
import functools

import torch
import torch.nn.functional as F

from segmamba_amd import lib as L, ops_raw

BF16, F16 = torch.bfloat16, torch.float16

# the row kernels: name -> flags of ops_raw.conv3d_k3_fwd / the routing tuple (chain, pitch48, chain32) of conv3d.py
ROW_VARIANTS = {"default": {}, "chain": dict(chain=True), "chain48": dict(chain=True, pitch48=True), "chain32": dict(chain32=True)}
ROW_ROUTES = {"default": (False, False, False), "chain": (True, False, False), "chain48": (True, True, False), "chain32": (False, False, True)}
ROW_STATS = ("chain48", "chain32")                       # the variants with the statistics epilogue

# (B, cin, cout, D, H, W), nt, splits (0 = the plan's own choice): the smallest shapes at which each mechanism of the cube kernel runs
CUBE_CASES = [
    ((1, 32, 64, 8, 8, 8), 2, 1),        # one cube, one round, every halo is padding, direct store
    ((2, 96, 64, 8, 16, 24), 0, 0),      # y and x neighbours, an interior cube in x, batch 2
    ((1, 96, 192, 16, 8, 8), 3, 3),      # z neighbour, 96-channel blocks
    ((1, 64, 128, 8, 8, 16), 4, 1),      # 128-channel blocks, direct store
    ((1, 96, 64, 8, 8, 16), 2, 2),       # uneven: 3 rounds in 2 splits
    ((2, 160, 128, 8, 8, 8), 4, 2),      # uneven: 5 rounds in 2 splits
    ((1, 160, 96, 8, 16, 8), 3, 3),      # uneven: 5 rounds in 3 splits
    ((1, 384, 384, 8, 8, 8), 0, 0),      # a layer the table routes to the cube kernel
]
CUBE_CASES_GPU = [((2, 128, 256, 16, 16, 16), 0, 0)]    # many workgroups
CUBE_SWEEP = [((1, 96, 192, 16, 8, 8), nt, s) for nt in (2, 3) for s in (1, 2, 3)]    # one layer under every valid plan
CUBE_FP16 = [((1, 64, 128, 8, 8, 16), 4, 1), ((1, 96, 64, 8, 8, 16), 2, 2)]            # a direct store; an uneven split + the reduction
CUBE_ROUNDED = [((1, 96, 64, 8, 8, 16), 2, 1), ((1, 96, 64, 8, 8, 16), 2, 2)]

# (B, cout, D, H, W) of the row kernels (48 input channels)
ROW_CASES_ALL = [(2, 48, 3, 20, 72), (1, 48, 2, 2, 16), (1, 48, 1, 16, 8), (1, 96, 2, 3, 72)]       # every variant
ROW_CASES_DEFAULT = [(1, 16, 3, 9, 72), (2, 32, 5, 7, 64)]                                         # Cout % 48 != 0: the first kernel only
ROW_CASE_GPU = (1, 48, 2, 16, 128)                       # width 128: where (chain, pitch48) is the table's choice
ROW_ROUNDED = (1, 48, 2, 3, 72)

WGRAD_ROW_CASES = [(1, 48, 48, 3, 4, 32), (1, 96, 48, 2, 3, 64), (1, 48, 48, 1, 20, 64), (1, 48, 48, 2, 3, 40), (1, 48, 48, 1, 3, 128),
                   (2, 48, 96, 5, 7, 64), (1, 4, 48, 2, 5, 16)]
WGRAD_CUBE_CASES = [(2, 32, 64, 8, 8, 16), (1, 64, 128, 8, 16, 24), (3, 32, 64, 16, 8, 8), (1, 96, 192, 8, 8, 8)]

# through the dispatcher: name -> (channels per part, cout, (D, H, W), forward / data-gradient routes, weight-gradient routes)
DISPATCH = {"row": (48, 48, (2, 4, 64), tuple(ROW_VARIANTS), ("mfma",)), "cube": (96, 192, (8, 8, 8), ("cube",), ("cube", "mfma"))}


# ---------------------------------------------------------------------------------------------------------------------------------
# operands, conditions, the comparison
# ---------------------------------------------------------------------------------------------------------------------------------
def _ints(g, shape, amp, density=1.0):
    """fp64 integers in {-amp..amp}, non-zero with probability ~density"""
    v = torch.randint(-amp, amp + 1, shape, generator=g)
    if density < 1.0:
        v = v * (torch.rand(shape, generator=g) < density)
    return v.double()


def _wdens(k: int) -> float:
    """density of a {-1, 0, 1} weight for a contraction of k terms: the activations have E[x^2] = 1, so a sum has variance
    k * density; 150 keeps sigma near 12 (17 with a second part accumulated) and the maximum over 10^5 - 10^6 outputs inside 128"""
    return min(0.15, 150.0 / k)


def _need_16bit(ref, what):
    m = float(ref.abs().max())
    assert m <= 128, f"{what}: the reference reaches {m}; the case must keep 16-bit outputs exact (max|ref| <= 128)"


def _need_stats(ref, what):
    m = float((ref * ref).flatten(2).sum(-1).max())
    assert m < 2 ** 24, f"{what}: sum(ref^2) of an instance reaches {m}; the statistics are exact only below 2^24"


def _where(idx, tile):
    if tile == "cube":
        b, c, z, y, x = idx
        return f" cube ({z // 8}, {y // 8}, {x // 8}) voxel ({z % 8}, {y % 8}, {x % 8}) wave {(z % 8) // 2}, channel {c % 16} of tile {c // 16}"
    if tile == "row":
        b, c, z, y, x = idx
        return f" x block {x // 64} (32-wide: {x // 32}) x tile {(x % 64) // 16} lane x {x % 16}, channel {c % 16} of tile {c // 16}"
    return ""


def _same(got, want, what, tile=None):
    """torch.equal, or an AssertionError that says where: how many elements differ, the first few with got / want and their position
    inside the 8 x 8 x 8 cube (tile="cube") or the row kernels' x block (tile="row")"""
    want = want.to(got.device)
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {tuple(got.shape)} {got.dtype}, expected {tuple(want.shape)} {want.dtype}"
    if torch.equal(got, want):
        return
    bad = (got != want) | (got != got)
    n = int(bad.sum())
    lines = []
    for idx in bad.nonzero()[:8].tolist():
        lines.append(f"  {tuple(idx)}: got {float(got[tuple(idx)])}, want {float(want[tuple(idx)])}{_where(idx, tile) if len(idx) == 5 else ''}")
    ch = sorted(set(bad.nonzero()[:, 1 if got.dim() == 5 and tile else 0].tolist()))
    names = "channels" if got.dim() == 5 and tile else "rows (dim 0)"
    raise AssertionError(f"{what}: {n} of {got.numel()} elements differ; {names} {ch[:16]}{' ...' if len(ch) > 16 else ''}\n" + "\n".join(lines))


def _untouched(buf, view_channels, W, fill, what):
    assert bool((buf[:, view_channels:] == fill).all()) and bool((buf[..., W:] == fill).all()), f"{what}: written outside the view"


def _stats_totals(st, ref, what):
    """counts, sums and sums of squares of the partials, per (batch, channel) instance, against the fp64 reference - all integers"""
    B, C = ref.shape[:2]
    vol = ref[0, 0].numel()
    assert st is not None and st.dtype == torch.float32 and tuple(st.shape[:2]) == (B, C) and st.shape[3] == 4, f"{what}: partials {None if st is None else tuple(st.shape)}"
    flat = ref.reshape(B, C, vol)
    _same(st[..., 0].double().sum(-1), torch.full((B, C), float(vol), dtype=torch.float64), what + ": counts")
    _same(st[..., 1].double().sum(-1), flat.sum(-1), what + ": sum of the partial sums")
    _same(st[..., 2].double().sum(-1), (flat * flat).sum(-1), what + ": sum of the partial sums of squares")


def _cube_stats(st, ref, splits, what):
    """the cube kernel's documented part layout: one split stores directly and writes a part per wave - cube (cz, cy, cx) x its four
    z-plane pairs, 128 voxels; otherwise the reduction launch writes a part per 512 consecutive voxels"""
    B, C, D, H, W = ref.shape
    vol = D * H * W
    chunk = 128 if splits == 1 else 512
    _stats_totals(st, ref, what)
    assert st.shape[2] == vol // chunk and bool((st[..., 0] == chunk).all()), f"{what}: {st.shape[2]} parts, expected {vol // chunk} of {chunk} voxels"
    if chunk == 512:
        parts = ref.reshape(B, C, vol // 512, 512)
    else:
        parts = ref.reshape(B, C, D // 8, 4, 2, H // 8, 8, W // 8, 8).permute(0, 1, 2, 5, 7, 3, 4, 6, 8).reshape(B, C, vol // 128, 128)
    _same(st[..., 1].double(), parts.sum(-1), what + f": part sums ({chunk} voxels)")
    _same(st[..., 2].double(), (parts * parts).sum(-1), what + f": part sums of squares ({chunk} voxels)")


def _conv(x, w, bias=None):
    return F.conv3d(x, w, bias, 1, 1)


@functools.lru_cache(maxsize=None)
def _fwd_case(B, cin, cout, D, H, W, amp_x=2, amp_w=1, seed=0):
    """fp64 operands and references of one forward / data-gradient case: y = conv(x, w) + bias, dx = the gradient of x for dy,
    y2 = y + conv(x2, w2) (a second input part accumulated in place); amp_x / amp_w > defaults: the dense rounded-once operands"""
    g = torch.Generator().manual_seed(1000 * seed + B + cin + cout + D + H + W)
    dense = amp_w > 1
    dx_, dw_ = (1.0, 1.0) if dense else (0.5, _wdens(27 * max(cin, cout)))
    x, x2 = _ints(g, (B, cin, D, H, W), amp_x, dx_), _ints(g, (B, cin, D, H, W), amp_x, dx_)
    w, w2 = _ints(g, (cout, cin, 3, 3, 3), amp_w, dw_), _ints(g, (cout, cin, 3, 3, 3), amp_w, dw_)
    bias, dy = _ints(g, (cout,), 3), _ints(g, (B, cout, D, H, W), amp_x, dx_)
    xr = x.clone().requires_grad_()
    y = _conv(xr, w, bias)
    dx, = torch.autograd.grad(y, xr, dy)
    y = y.detach()
    return dict(x=x, x2=x2, w=w, w2=w2, bias=bias, dy=dy, y=y, dx=dx, conv2=_conv(x2, w2), y2=y + _conv(x2, w2))


@functools.lru_cache(maxsize=None)
def _wgrad_case(B, cin, cout, D, H, W):
    g = torch.Generator().manual_seed(7 + B + cin + cout + D + H + W)
    x, dy = _ints(g, (B, cin, D, H, W), 2, 0.5), _ints(g, (B, cout, D, H, W), 2, 0.5)
    w = torch.zeros(cout, cin, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    dw, = torch.autograd.grad(_conv(x, w), w, dy)
    return dict(x=x, dy=dy, dw=dw)


def _dev(t, dtype, dev):
    return t.to(dtype).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# the cube kernel: forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _cube_image(lib, w, flipped):
    """the pack kernel's image of a 16-bit weight (segm_conv3d_k3_cube_pack_multi, one descriptor), which must be the image the
    exported index map defines, element for element"""
    want = ops_raw.conv3d_cube_weight_image(lib, w, flipped, by_index=True)
    descs, nblocks = ops_raw.cube_pack_descs([(0, 0, w.shape[0], w.shape[1], w.stride(0), flipped)], w.device)
    img = ops_raw.conv3d_cube_pack_multi(lib, w.reshape(-1), torch.zeros_like(want), descs, nblocks)
    _same(img, want, f"cube weight image (flipped={flipped}) of the pack kernel against the index map")
    return img


def _plan_or_auto(lib, B, cin, cout, D, H, W, nt, splits):
    """(nt, splits) when the plan takes that request for this convolution, else (0, 0): the data gradient swaps cin and cout"""
    try:
        p = ops_raw.conv3d_cube_plan(lib, B, cin, cout, D, H, W, nt, splits)
    except RuntimeError:
        return 0, 0
    return (nt, splits) if (nt == 0 or p[0] == nt) and (splits == 0 or p[1] == splits) else (0, 0)


def _padded(t, dtype, dev, extra_c, fill=0.0):
    """t as a view with padded batch, channel and row strides: (B, C + extra_c, D, H, W + 8)[:, :C, ..., :W] -> (buffer, view)"""
    B, C, D, H, W = t.shape
    buf = torch.full((B, C + extra_c, D, H, W + 8), fill, dtype=dtype, device=dev)
    view = buf[:, :C, :, :, :W]
    view.copy_(t.to(dtype))
    return buf, view


def check_cube(lib, dev, shape, nt=0, splits=0, dtype=BF16):
    """forward with bias and statistics; the data gradient through the flipped image; a second input part accumulated in place on
    padded strides; nothing written outside the view; the pack kernel's images"""
    B, cin, cout, D, H, W = shape
    c = _fwd_case(*shape)
    what = f"cube {shape} nt={nt} splits={splits} {dtype}"
    for k in ("y", "dx", "y2"):
        _need_16bit(c[k], f"{what}: {k}")
    _need_stats(c["y"], what)
    _need_stats(c["y2"], what)
    x, w, bias = _dev(c["x"], dtype, dev), _dev(c["w"], dtype, dev), _dev(c["bias"], torch.float32, dev)
    img = _cube_image(lib, w, False)
    pnt, ps, need = ops_raw.conv3d_cube_plan(lib, B, cin, cout, D, H, W, nt, splits)
    assert (nt == 0 or pnt == nt) and (splits == 0 or ps == splits), f"{what}: the plan answered nt={pnt} splits={ps}"
    assert need == (0 if ps == 1 else ps * B * cout * D * H * W)
    y, st = ops_raw.conv3d_k3_cube_fwd(lib, x, img, cout, bias, nt=nt, splits=splits, want_stats=True)
    _same(y, c["y"].float().to(dtype), what + ": forward", "cube")
    _cube_stats(st, c["y"].to(st.device), ps, what + ": statistics")
    # the data gradient: the same launch on dy with the image of flip(w)^T
    # (where the kernel takes it: the gradient's output channels are cin, which must be a multiple of 64 or 96)
    dy = _dev(c["dy"], dtype, dev)
    assert ops_raw.conv3d_cube_supported(dy, cin) == (cin % 64 == 0 or cin % 96 == 0)
    if ops_raw.conv3d_cube_supported(dy, cin):
        dnt, dsp = _plan_or_auto(lib, B, cout, cin, D, H, W, nt, splits)
        dx = ops_raw.conv3d_k3_cube_fwd(lib, dy, _cube_image(lib, w, True), cin, nt=dnt, splits=dsp)
        _same(dx, c["dx"].float().to(dtype), what + f": data gradient (nt={dnt} splits={dsp})", "cube")
    # a second part of the input added in place; input and output with padded batch / channel / row strides
    _, xp = _padded(c["x2"], dtype, dev, 1)
    yp, yv = _padded(c["y"], dtype, dev, 2, 7.0)
    y2, st2 = ops_raw.conv3d_k3_cube_fwd(lib, xp, _cube_image(lib, _dev(c["w2"], dtype, dev), False), cout, None, out=yv, accumulate=True,
                                         nt=nt, splits=splits, want_stats=True)
    assert y2 is yv
    _same(yv, c["y2"].float().to(dtype), what + ": accumulate on padded views", "cube")
    _untouched(yp, cout, W, 7.0, what)
    _cube_stats(st2, c["y2"].to(st2.device), ps, what + ": statistics of the accumulating launch")


def check_cube_rounded_once(lib, dev, shape, nt, splits, dtype=BF16):
    """dense operands in {-8..8} x {-4..4}: the exact sum (thousands) rounded to the 16-bit dtype ONCE, also with several splits (fp32
    partial sums are exact) and in accumulate mode ((old + conv) rounded once)"""
    B, cin, cout, D, H, W = shape
    c = _fwd_case(*shape, amp_x=8, amp_w=4, seed=1)
    what = f"cube rounded once {shape} nt={nt} splits={splits} {dtype}"
    assert 1024 <= float(c["y"].abs().max()) < 2 ** 15 and float(c["y2"].abs().max()) < 2 ** 15
    x, w, bias = _dev(c["x"], dtype, dev), _dev(c["w"], dtype, dev), _dev(c["bias"], torch.float32, dev)
    y = ops_raw.conv3d_k3_cube_fwd(lib, x, _cube_image(lib, w, False), cout, bias, nt=nt, splits=splits)
    want = c["y"].float().to(dtype)
    _same(y, want, what + ": forward", "cube")
    yp, yv = _padded(want, dtype, dev, 2, 7.0)
    ops_raw.conv3d_k3_cube_fwd(lib, _dev(c["x2"], dtype, dev), _cube_image(lib, _dev(c["w2"], dtype, dev), False), cout, None, out=yv,
                               accumulate=True, nt=nt, splits=splits)
    _same(yv, (want.double() + c["conv2"]).float().to(dtype), what + ": accumulate", "cube")
    _untouched(yp, cout, W, 7.0, what)


def check_cube_refusals(lib, dev):
    """ops_raw.conv3d_k3_cube_fwd and conv3d_k3_fwd_cl check `out` and `w_image` before the kernel sees their pointers: a wrong-shape
    out, an fp32 out, an out with stride(4) != 1, a short image and an image of another dtype each raise and leave `out` untouched"""
    B, cin, cout, D, H, W = 1, 32, 64, 8, 8, 8
    g = torch.Generator().manual_seed(3)
    x = _dev(_ints(g, (B, cin, D, H, W), 2, 0.5), BF16, dev)
    w = _dev(_ints(g, (cout, cin, 3, 3, 3), 1, 0.1), BF16, dev)
    img = ops_raw.conv3d_cube_weight_image(lib, w, by_index=True)
    good = torch.full((B, cout, D, H, W), 7.0, dtype=BF16, device=dev)
    outs = {"a smaller out": torch.full((B, cout - 16, D, H, W), 7.0, dtype=BF16, device=dev),
            "a larger out": torch.full((B, cout, D, H, W + 8), 7.0, dtype=BF16, device=dev),
            "an fp32 out": torch.full((B, cout, D, H, W), 7.0, dtype=torch.float32, device=dev),
            "an out with stride(4) = 2": torch.full((B, cout, D, H, 2 * W), 7.0, dtype=BF16, device=dev)[..., ::2],
            "an out with rows off 16 bytes": torch.full((B, cout, D, H, W + 4), 7.0, dtype=BF16, device=dev)[..., :W]}
    if torch.device(dev).type != "cpu":
        outs["an out on the host"] = torch.full((B, cout, D, H, W), 7.0, dtype=BF16)
    for name, out in outs.items():
        for acc in (False, True):
            try:
                ops_raw.conv3d_k3_cube_fwd(lib, x, img, cout, None, out=out, accumulate=acc)
            except RuntimeError:
                pass
            else:
                raise AssertionError(f"conv3d_k3_cube_fwd took {name}")
            assert bool((out == 7.0).all()), f"conv3d_k3_cube_fwd wrote to {name}"
    images = {"a short w_image": img[:-8], "an fp16 w_image": img.to(F16), "a strided w_image": torch.stack((img, img), 1)[:, 0],
              "a long w_image": torch.cat((img, img[:8]))}
    for name, bad in images.items():
        try:
            ops_raw.conv3d_k3_cube_fwd(lib, x, bad, cout, None, out=good)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"conv3d_k3_cube_fwd took {name}")
        assert bool((good == 7.0).all()), f"conv3d_k3_cube_fwd wrote to out with {name}"
    ops_raw.conv3d_k3_cube_fwd(lib, x, img, cout, None, out=good)                   # and the valid call still runs
    want = _conv(x.double().cpu(), w.double().cpu())
    _need_16bit(want, "refusals: the valid call")
    _same(good, want.float().to(BF16), "cube forward into a valid out", "cube")
    # the channel-last prototype: the same checks
    xc = _dev(_ints(g, (1, 2, 4, 16, 48), 2, 0.5), BF16, dev)
    wc = _dev(_ints(g, (48, 48, 3, 3, 3), 1, 0.1), BF16, dev)
    imgc = ops_raw.conv3d_cl_weight_image(lib, wc)
    goodc = torch.full((1, 2, 4, 16, 48), 7.0, dtype=BF16, device=dev)
    for name, out in {"a smaller out": torch.full((1, 2, 4, 8, 48), 7.0, dtype=BF16, device=dev),
                      "an fp32 out": torch.full((1, 2, 4, 16, 48), 7.0, dtype=torch.float32, device=dev),
                      "an out with stride(4) = 2": torch.full((1, 2, 4, 16, 96), 7.0, dtype=BF16, device=dev)[..., ::2]}.items():
        try:
            ops_raw.conv3d_k3_fwd_cl(lib, xc, imgc, out=out)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"conv3d_k3_fwd_cl took {name}")
        assert bool((out == 7.0).all()), f"conv3d_k3_fwd_cl wrote to {name}"
    for name, bad in {"a short w_image": imgc.reshape(-1)[:-8], "an fp16 w_image": imgc.to(F16)}.items():
        try:
            ops_raw.conv3d_k3_fwd_cl(lib, xc, bad, out=goodc)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"conv3d_k3_fwd_cl took {name}")
        assert bool((goodc == 7.0).all()), f"conv3d_k3_fwd_cl wrote to out with {name}"


# ---------------------------------------------------------------------------------------------------------------------------------
# the row kernels: forward and data gradient
# ---------------------------------------------------------------------------------------------------------------------------------
def _row_fwd(lib, x, w, bias, kw, want_stats=False, out=None, flipped=False):
    """the convolution of x with w through 48-channel input blocks, as conv3d._fwd_hip launches them: later blocks accumulate in
    place; `flipped`: the data gradient (x is dy, w the forward weight)"""
    pack = ops_raw.pack_conv3d_weight_for_dgrad if flipped else ops_raw.pack_conv3d_weight
    cin = x.shape[1]
    blocks = [slice(i, min(i + 48, cin)) for i in range(0, cin, 48)]
    st, into = None, out is not None
    for i, ib in enumerate(blocks):
        wp = pack(w[ib] if flipped else w[:, ib], x.dtype)
        last = want_stats and i + 1 == len(blocks)
        res = ops_raw.conv3d_k3_fwd(lib, x[:, ib], wp, bias if i == 0 else None, out=out, accumulate=i > 0 or into, want_stats=last, **kw)
        out, st = res if last else (res, None)
    return (out, st) if want_stats else out


def check_row(lib, dev, shape, variant, dtype=BF16, cin=48, sliced=False):
    """forward with bias (and the statistics of the variants that have the epilogue), the data gradient through
    pack_conv3d_weight_for_dgrad, a second 48-channel block accumulated in place.  cin < 48: a narrow first layer, zero-padded by
    pack_conv3d_weight; sliced: the input is the channel slice x96[:, 48:] of a wider tensor"""
    B, cout, D, H, W = shape
    kw = ROW_VARIANTS[variant]
    c = _fwd_case(B, cin, cout, D, H, W)
    what = f"row {variant} {shape} cin={cin} {dtype}{' sliced' if sliced else ''}"
    for k in ("y", "dx", "y2"):
        _need_16bit(c[k], f"{what}: {k}")
    x, w, bias = _dev(c["x"], dtype, dev), _dev(c["w"], dtype, dev), _dev(c["bias"], torch.float32, dev)
    if sliced:
        x = torch.cat((_dev(c["x2"], dtype, dev), x), 1)[:, cin:]
        assert not x.is_contiguous() or B == 1
    stats = variant in ROW_STATS
    res = _row_fwd(lib, x, w, bias, kw, want_stats=stats)
    y, st = res if stats else (res, None)
    _same(y, c["y"].float().to(dtype), what + ": forward", "row")
    if stats:
        _need_stats(c["y"], what)
        _stats_totals(st, c["y"].to(st.device), what + ": statistics")
    if cin % 16 == 0:                                     # (the data gradient of a narrow first layer is never asked for)
        dx = _row_fwd(lib, _dev(c["dy"], dtype, dev), w, None, kw, flipped=True)
        _same(dx, c["dx"].float().to(dtype), what + ": data gradient", "row")
    if cout % 48 or cin != 48:
        return
    ya = y.clone()
    res = _row_fwd(lib, _dev(c["x2"], dtype, dev), _dev(c["w2"], dtype, dev), None, kw, want_stats=stats, out=ya)
    _same(ya, c["y2"].float().to(dtype), what + ": second block accumulated in place", "row")
    if stats:
        _need_stats(c["y2"], what)
        _stats_totals(res[1], c["y2"].to(res[1].device), what + ": statistics of the accumulating launch")


def check_row_rounded_once(lib, dev, variant, dtype=BF16):
    B, cout, D, H, W = ROW_ROUNDED
    kw = ROW_VARIANTS[variant]
    c = _fwd_case(B, 48, cout, D, H, W, amp_x=8, amp_w=4, seed=1)
    what = f"row rounded once {variant} {dtype}"
    assert 1024 <= float(c["y"].abs().max()) < 2 ** 15 and float(c["y2"].abs().max()) < 2 ** 15
    y = _row_fwd(lib, _dev(c["x"], dtype, dev), _dev(c["w"], dtype, dev), _dev(c["bias"], torch.float32, dev), kw)
    want = c["y"].float().to(dtype)
    _same(y, want, what + ": forward", "row")
    ya = want.to(dev).clone()
    _row_fwd(lib, _dev(c["x2"], dtype, dev), _dev(c["w2"], dtype, dev), None, kw, out=ya)
    _same(ya, (want.double() + c["conv2"]).float().to(dtype), what + ": accumulate", "row")


# ---------------------------------------------------------------------------------------------------------------------------------
# the weight-gradient kernels
# ---------------------------------------------------------------------------------------------------------------------------------
def _check_dw(fn, x, dy, ref, dtype, what):
    assert float(ref.abs().max()) < 2 ** 24
    dw = fn(x, dy, torch.float32)
    _same(dw, ref.float(), what + ": fp32 result")
    _same(fn(x, dy, dtype), ref.float().to(dtype), what + ": 16-bit result, rounded once")
    return dw


def check_wgrad_row(lib, dev, shape, dtype=BF16):
    """segm_conv3d_k3_wgrad against fp64 autograd"""
    c = _wgrad_case(*shape)
    assert ops_raw.conv3d_k3_wgrad_supported(_dev(c["x"], dtype, dev), _dev(c["dy"], dtype, dev))
    _check_dw(lambda a, b, t: ops_raw.conv3d_k3_wgrad(lib, a, b, t), _dev(c["x"], dtype, dev), _dev(c["dy"], dtype, dev), c["dw"], dtype,
              f"wgrad {shape} {dtype}")


def check_wgrad_row_slices(lib, dev, dtype=BF16):
    """channel-slice views of wider tensors, as the decoder without the concatenation passes them"""
    c = _wgrad_case(1, 96, 96, 2, 2, 32)
    x, dy = _dev(c["x"], dtype, dev)[:, 48:], _dev(c["dy"], dtype, dev)[:, :48]
    _check_dw(lambda a, b, t: ops_raw.conv3d_k3_wgrad(lib, a, b, t), x, dy, c["dw"][:48, 48:], dtype, f"wgrad channel slices {dtype}")


def check_wgrad_cube(lib, dev, shape, dtype=BF16):
    """segm_conv3d_k3_cube_wgrad against fp64 autograd; the same on views with padded batch / channel / row strides"""
    B, cin, cout, D, H, W = shape
    c = _wgrad_case(*shape)
    x, dy = _dev(c["x"], dtype, dev), _dev(c["dy"], dtype, dev)
    assert ops_raw.conv3d_cube_wgrad_supported(x, dy)
    fn = lambda a, b, t: ops_raw.conv3d_k3_cube_wgrad(lib, a, b, t)
    _check_dw(fn, x, dy, c["dw"], dtype, f"cube wgrad {shape} {dtype}")
    xp = torch.zeros(B, cin + 3, D, H, W + 8, dtype=dtype, device=dev)[:, :cin, :, :, :W]
    xp.copy_(x)
    dyp = torch.zeros(B + 1, cout, D, H, W + 16, dtype=dtype, device=dev)[:B, :, :, :, :W]
    dyp.copy_(dy)
    _check_dw(fn, xp, dyp, c["dw"], dtype, f"cube wgrad {shape} {dtype} on padded views")


# ---------------------------------------------------------------------------------------------------------------------------------
# through the dispatcher (segmamba_amd/conv3d.py)
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dispatch_case(config):
    """two input parts, fp32 master weights of a 3x3x3 and a 1x1x1 convolution on their concatenation, bias, output gradients; fp64
    autograd of the concatenated convolutions: y, y3, the gradient of every part, dW, dW3, db - and the same for part 0 alone"""
    c, cout, (D, H, W), _, _ = DISPATCH[config]
    g = torch.Generator().manual_seed(11 + c + cout)
    xs = [_ints(g, (1, c, D, H, W), 2, 0.5) for _ in range(2)]
    w1 = _ints(g, (cout, 2 * c, 3, 3, 3), 1, _wdens(27 * max(2 * c, cout)))
    w3 = _ints(g, (cout, 2 * c, 1, 1, 1), 1, 0.1)
    bias = _ints(g, (cout,), 3)
    dy1, dy3 = _ints(g, (1, cout, D, H, W), 2, 0.5), _ints(g, (1, cout, D, H, W), 2, 0.25)
    out = dict(xs=xs, w1=w1, w3=w3, bias=bias, dy1=dy1, dy3=dy3)
    # one part with bias (conv3d_same)
    a, wa, ba = xs[0].clone().requires_grad_(), w1[:, :c].clone().requires_grad_(), bias.clone().requires_grad_()
    y = _conv(a, wa, ba)
    out["one"] = (y.detach(),) + torch.autograd.grad(y, (a, wa, ba), dy1)
    # both parts (conv3d_same_cat), and with the 1x1x1 convolution (res_front)
    parts = [x.clone().requires_grad_() for x in xs]
    v1, v3 = w1.clone().requires_grad_(), w3.clone().requires_grad_()
    xc = torch.cat(parts, 1)
    y1, y3 = _conv(xc, v1), F.conv3d(xc, v3)
    out["cat"] = (y1.detach(),) + torch.autograd.grad(y1, (v1, *parts), dy1, retain_graph=True)
    out["front"] = (y1.detach(), y3.detach()) + torch.autograd.grad([y1, y3], (v1, v3, *parts), [dy1, dy3])
    return out


def check_dispatch(lib, dev, monkeypatch, config, fwd_route, wgrad_route, dtype=BF16):
    """conv3d_same (bias, statistics), conv3d_same_cat and res_front (two parts) with every 3x3x3 launch forced onto one library
    route: y, y3, every dx, dW, dW3, db and the statistics against fp64 autograd of the concatenated convolution"""
    from segmamba_amd import conv3d as C3, linear as LN
    c, cout, (D, H, W), fwd_routes, wgrad_routes = DISPATCH[config]
    assert fwd_route in fwd_routes and wgrad_route in wgrad_routes
    fv = ROW_ROUTES.get(fwd_route, fwd_route)
    emulated = torch.device(dev).type == "cpu"
    if emulated:
        monkeypatch.setattr(L, "get_lib", lambda: lib)
        monkeypatch.setattr(L, "on_device", lambda t: True)
        monkeypatch.setattr(LN, "_PW_MIN", 64)
    monkeypatch.setattr(C3, "_CAT_FUSED", True)
    monkeypatch.setattr(C3, "_RES_FRONT", True)
    monkeypatch.setattr(C3, "_STATS", True)
    r = _dispatch_case(config)
    what = f"dispatcher {config} fwd/dgrad={fwd_route} wgrad={wgrad_route} {dtype}"
    tile = "cube" if fv == "cube" else "row"
    xs = [_dev(x, dtype, dev) for x in r["xs"]]
    w1, w3, bias = (_dev(r[k], torch.float32, dev) for k in ("w1", "w3", "bias"))      # fp32 masters
    dy1, dy3 = _dev(r["dy1"], dtype, dev), _dev(r["dy3"], dtype, dev)
    # the routes being forced are really offered for these operands ...
    w16 = w1.to(dtype)
    assert fv in C3._fwd_variants(xs[0], w16[:, :c]) and fv in C3._fwd_variants(dy1, w16[:, :c], flipped=True), what
    assert wgrad_route in C3._wgrad_variants(xs[0], dy1, w16[:, :c]), what
    calls = []

    def route(kind, width, variants):
        """... and no launch takes another one: every route decision is recorded"""
        want = wgrad_route if kind == "wgrad" else fv
        assert want in variants, (kind, variants)
        calls.append((kind, want))
        return want
    monkeypatch.setattr(C3, "_route", route)
    has_stats = fv == "cube" or fwd_route in ROW_STATS

    def stats_of(st, ref, name):
        if not has_stats:
            assert st is None, f"{what}: {name}: partials from a launch without the epilogue"
            return
        _need_stats(ref, what)
        _stats_totals(st, ref.to(st.device), f"{what}: {name}: statistics")

    def exact16(ref, name):
        _need_16bit(ref, f"{what}: {name}")
        return ref.float().to(dtype)

    # ---- conv3d_same: one part, bias, statistics
    y_r, dx_r, dw_r, db_r = r["one"]
    a, wa, ba = xs[0].clone().requires_grad_(), w1[:, :c].clone().requires_grad_(), bias.clone().requires_grad_()
    y, st = C3.conv3d_same(a, wa, ba, want_stats=True)
    assert type(y.grad_fn).__name__ == "_ConvSameBackward"
    dx, dw, db = torch.autograd.grad(y, (a, wa, ba), dy1)
    _same(y.detach(), exact16(y_r, "conv3d_same y"), what + ": conv3d_same y", tile)
    stats_of(st, y_r, "conv3d_same")
    _same(dx, exact16(dx_r, "conv3d_same dx"), what + ": conv3d_same dx", tile)
    _same(dw, dw_r.float(), what + ": conv3d_same dW")
    _same(db, db_r.float(), what + ": conv3d_same db")
    assert calls == [("fwd", fv), ("dgrad", fv), ("wgrad", wgrad_route)], calls
    # ---- conv3d_same_cat: two parts, the second added in place
    del calls[:]
    y_r, dw_r, *dx_r = r["cat"]
    parts, v1 = [x.clone().requires_grad_() for x in xs], w1.clone().requires_grad_()
    y, st = C3.conv3d_same_cat(tuple(parts), v1, want_stats=True)
    assert type(y.grad_fn).__name__ == "_ConvSameCatBackward"
    dw, *dx = torch.autograd.grad(y, (v1, *parts), dy1)
    _same(y.detach(), exact16(y_r, "conv3d_same_cat y"), what + ": conv3d_same_cat y", tile)
    stats_of(st, y_r, "conv3d_same_cat")
    for i in range(2):
        _same(dx[i], exact16(dx_r[i], f"conv3d_same_cat dx[{i}]"), what + f": conv3d_same_cat dx[{i}]", tile)
    _same(dw, dw_r.float(), what + ": conv3d_same_cat dW")
    assert sorted(calls) == sorted([("fwd", fv), ("dgrad", fv), ("wgrad", wgrad_route)] * 2), calls
    # ---- res_front: the 3x3x3 and the 1x1x1 convolution of the two parts as one node
    del calls[:]
    y1_r, y3_r, dw1_r, dw3_r, *dx_r = r["front"]
    # below linear._MIN_K voxels the 1x1x1 weight gradient is a BLAS product in the 16-bit dtype: exact while its integers are
    assert float(dw3_r.abs().max()) <= 256
    parts, v1, v3 = [x.clone().requires_grad_() for x in xs], w1.clone().requires_grad_(), w3.clone().requires_grad_()
    res = C3.res_front(tuple(parts), v1, v3, want_stats=True)
    assert res is not None
    y1, st, y3 = res
    assert type(y1.grad_fn).__name__ == "_ResFrontBackward"
    dw1, dw3, *dx = torch.autograd.grad([y1, y3], (v1, v3, *parts), [dy1, dy3])
    _same(y1.detach(), exact16(y1_r, "res_front y1"), what + ": res_front y1", tile)
    _same(y3.detach(), exact16(y3_r, "res_front y3"), what + ": res_front y3")
    stats_of(st, y1_r, "res_front")
    for i in range(2):
        _same(dx[i], exact16(dx_r[i], f"res_front dx[{i}]"), what + f": res_front dx[{i}]", tile)
    _same(dw1, dw1_r.float(), what + ": res_front dW")
    _same(dw3.reshape(dw3_r.shape), dw3_r.float(), what + ": res_front dW3")
    assert sorted(calls) == sorted([("fwd", fv), ("dgrad", fv), ("wgrad", wgrad_route)] * 2), calls


def check_add_part_after_vendor_route(lib, dev, monkeypatch):
    """conv3d._add_part: part 0 of a concatenated convolution on the vendor route with a result whose channels are NOT dense (a
    channel- and row-padded view), part 1 on a library route: the library kernel's accumulate mode must not be handed that tensor
    as `into` - the part is added by an ordinary add, and the sum is the convolution (non-integer data, the dispatcher tests' tolerance)"""
    from segmamba_amd import conv3d as C3
    if torch.device(dev).type == "cpu":
        monkeypatch.setattr(L, "get_lib", lambda: lib)
        monkeypatch.setattr(L, "on_device", lambda t: True)
    monkeypatch.setattr(C3, "_CAT_FUSED", True)
    g = torch.Generator().manual_seed(17)
    a, b = (torch.randn(2, 48, 2, 3, 64, generator=g).bfloat16().to(dev) for _ in range(2))
    w = (0.05 * torch.randn(48, 96, 3, 3, 3, generator=g)).to(dev)
    ref = _conv(torch.cat((a, b), 1).double().cpu(), w.bfloat16().double().cpu())
    real, seen = C3._run_fwd, []

    def run_fwd(v, x, w_, pad, bias=None, into=None, **kw):
        seen.append((v, into is not None))
        y = real(v, x, w_, pad, bias, into=into, **kw)
        if v is not None:
            return y
        buf = torch.full((y.shape[0], y.shape[1] + 2, *y.shape[2:4], y.shape[4] + 8), 7.0, dtype=y.dtype, device=y.device)
        view = buf[:, :y.shape[1], :, :, :y.shape[4]]
        view.copy_(y)
        assert not ops_raw.channel_dense(view)
        return view
    monkeypatch.setattr(C3, "_run_fwd", run_fwd)
    for lib_route in C3._HIP_VARIANTS:
        del seen[:]
        order = []

        def route(kind, width, variants, lib_route=lib_route, order=order):
            order.append(None if not order else lib_route)
            assert order[-1] in variants
            return order[-1]
        monkeypatch.setattr(C3, "_route", route)
        y = C3.conv3d_same_cat((a, b), w)
        assert seen == [(None, False), (lib_route, False)], seen       # no `into` for the library launch: an ordinary add
        assert (y.double().cpu() - ref).abs().max() <= 2e-2 * float(ref.abs().max()), lib_route
