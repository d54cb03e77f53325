"""Checks shared by tests/test_emu_stitch.py (kernel sources on the CPU emulator) and tests/test_gpu_stitch.py (the HIP library): the
kernel route of the predictor's stitching (csrc/stitch.hip, `stitch="hip"`) against the ATen route of segmamba_amd/predictor.py.

The two routes perform the same fp32 operations in the same order - one rounded product and one sum per window and voxel, one
correctly rounded division, the sums of the mirror passes in the reference's order, a division by a power of two - so every
comparison between them is `torch.equal`.  The reference's fixture (tests/golden/predict.npz) is met at the tolerances
tests/test_predictor.py uses for the ATen route."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from segmamba_amd import lib as L
from segmamba_amd import ops_raw
from segmamba_amd import predictor as P
from tests.golden.make_golden_predict import CASES, toy_net

NEW_EXPORTS = ("segm_window_gather", "segm_window_count", "segm_window_blend", "segm_window_finish")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "predict.npz"))

# name: (input shape, roi, sw_batch, overlap, mode, mirror axes)
EQUAL_CASES = dict(CASES)
EQUAL_CASES.update({
    "pad_mirror": ((2, 2, 10, 19, 13), (16, 16, 16), 3, 0.5, "gaussian", [0, 1, 2]),     # asymmetric padding, chunks that span samples
    "odd_roi": ((1, 3, 21, 9, 30), (8, 12, 16), 5, 0.6, "gaussian", [1, 2]),
    "packet_x": ((1, 2, 16, 16, 64), (16, 16, 32), 4, 0.5, "gaussian", [0, 1, 2]),       # aligned rows: packets, reversed by the x-flip
    "many_jobs": ((1, 1, 12, 12, 12), (4, 4, 4), 100, 0.5, "gaussian", [2]),             # 125 windows in one chunk: the split at 64
    "const_pad_all": ((1, 1, 5, 6, 7), (8, 8, 8), 1, 0.25, "constant", [0, 1, 2]),        # padding on every axis
})
ENTRY_CASES = ("pad_mirror", "packet_x")
COUT = 3


def case_input(name, dev):
    shape = EQUAL_CASES[name][0]
    return torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape))).to(dev)


class RampNet(torch.nn.Module):
    """pointwise and position dependent: out[:, k] = win[:, k % C] * R[k] + S[k] with fixed random roi-shaped R and S, optionally
    cast to bf16.  Independent of how windows are batched, and not flip-equivariant: a wrong start, pad offset, mirror bit or pass
    order changes values."""

    def __init__(self, roi, cast=None, cout=COUT):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        self.register_buffer("R", torch.rand((cout,) + tuple(roi), generator=g) + 0.5)
        self.register_buffer("S", torch.rand((cout,) + tuple(roi), generator=g) - 0.5)
        self.cast = cast

    def forward(self, win):
        C = win.shape[1]
        out = torch.stack([win[:, k % C] * self.R[k] + self.S[k] for k in range(self.R.shape[0])], dim=1)
        return out if self.cast is None else out.to(self.cast)


def ramp_net(roi, cast=None):
    return RampNet(roi, cast).eval()


def inferers(name):
    _, roi, swb, ov, mode, _ = EQUAL_CASES[name]
    return tuple(P.SlidingWindowInferer(roi_size=roi, sw_batch_size=swb, overlap=ov, mode=mode, stitch=s) for s in ("aten", "hip"))


def geometry(name):
    shape, roi = EQUAL_CASES[name][0], EQUAL_CASES[name][1]
    size = shape[2:]
    image = tuple(max(s, r) for s, r in zip(size, roi))
    pad0 = tuple((i - s) // 2 for i, s in zip(image, size))
    ov = P._tuple3(EQUAL_CASES[name][3], 3)
    interval = tuple(r if r == s else max(int(r * (1 - o)), 1) for r, s, o in zip(roi, image, ov))
    return size, roi, image, pad0, P.dense_patch_starts(image, roi, interval)


def flip_dims(mask, first=0):
    return tuple(first + ax for ax in range(3) if mask >> ax & 1)


# ---- 1. bit-equality with the ATen route ----------------------------------------------------------------------------------------------------
def check_equal_to_aten(name, dev):
    """`maybe_mirror_and_predict` and the bare inferer call, both routes, `ramp_net` in fp32 and with the bf16 cast: torch.equal"""
    axes = EQUAL_CASES[name][5]
    x = case_input(name, dev)
    aten, hip = inferers(name)
    roi = geometry(name)[1]
    for cast in (None, torch.bfloat16):
        net = ramp_net(roi, cast).to(dev)
        want = P.Predictor(aten, axes, autocast_dtype=torch.float32).maybe_mirror_and_predict(x, net, device=torch.device(dev))
        got = P.Predictor(hip, axes, autocast_dtype=torch.float32).maybe_mirror_and_predict(x, net, device=torch.device(dev))
        assert got.dtype == torch.float32 and got.shape == want.shape and got.device == want.device and got.is_contiguous()
        assert torch.equal(got, want), (name, cast, float((got - want).abs().max()))
        with torch.no_grad():
            want, got = aten(x, net), hip(x, net)
        assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got, want), (name, cast, "window", float((got - want).abs().max()))
        via_function = P.sliding_window_inference(x, roi, EQUAL_CASES[name][2], net, EQUAL_CASES[name][3], EQUAL_CASES[name][4],
                                                  stitch="hip")
        assert torch.equal(via_function, want)


# ---- 2. the reference's fixture -------------------------------------------------------------------------------------------------------------
def check_golden(name, dev):
    """the kernel route with `toy_net` against tests/golden/predict.npz, at the tolerances of tests/test_predictor.py: atol 2e-6 on
    the host; on the GPU relative 2e-5 in fp32 and 2e-2 under bf16 autocast"""
    shape, roi, swb, ov, mode, axes = CASES[name]
    x = case_input(name, dev)
    net = toy_net(shape[1], 3).to(dev)
    hip = P.SlidingWindowInferer(roi_size=roi, sw_batch_size=swb, overlap=ov, mode=mode, stitch="hip")
    device = torch.device(dev)
    with torch.no_grad():
        win = hip(x, net)
    if device.type == "cpu":
        assert np.allclose(win.numpy(), GOLD[name + "_window"], atol=2e-6)
        tta = P.Predictor(hip, axes).maybe_mirror_and_predict(x, net)
        assert np.allclose(tta.numpy(), GOLD[name + "_tta"], atol=2e-6)
        return

    def err(got, key):
        ref = GOLD[key]
        return float(np.abs(got.cpu().numpy() - ref).max()) / max(1.0, float(np.abs(ref).max()))
    e_win = err(win, name + "_window")
    print(f"{name}: window {e_win:.3e}")
    assert win.is_cuda and e_win <= 2e-5, f"window prediction: relative error {e_win:.3e}"
    e32 = err(P.Predictor(hip, axes, autocast_dtype=torch.float32).maybe_mirror_and_predict(x, net, device=device), name + "_tta")
    print(f"{name}: mirror TTA fp32 {e32:.3e}")
    assert e32 <= 2e-5, f"mirror TTA without autocast: relative error {e32:.3e}"
    tta = P.Predictor(hip, axes).maybe_mirror_and_predict(x, net, device=device)
    e_tta = err(tta, name + "_tta")
    print(f"{name}: mirror TTA bf16 {e_tta:.3e}")
    assert tta.is_cuda and tta.dtype == torch.float32 and e_tta <= 2e-2, f"mirror TTA: relative error {e_tta:.3e}"


# ---- 3. each entry on its own ---------------------------------------------------------------------------------------------------------------
def _launches(jobs):
    return [jobs[k:k + L.STITCH_MAX_WINDOWS] for k in range(0, len(jobs), L.STITCH_MAX_WINDOWS)]


def _slices(st, roi):
    return tuple(slice(s, s + r) for s, r in zip(st, roi))


def _aten_windows(x, roi, pad0, image, jobs, mask, cval):
    size = x.shape[2:]
    dims = flip_dims(mask, 2)
    xin = torch.flip(x, dims) if dims else x
    pad = []
    for d in (2, 1, 0):
        pad.extend([pad0[d], image[d] - size[d] - pad0[d]])
    if any(pad):
        xin = F.pad(xin, pad, mode="constant", value=cval)
    return torch.cat([xin[(slice(b, b + 1), slice(None)) + _slices(st, roi)] for b, *st in jobs])


def check_gather(lib, name, dev):
    """against torch.flip + F.pad + slicing under all eight masks, on a dense volume and on a channel slice of a larger buffer"""
    size, roi, image, pad0, starts = geometry(name)
    x = case_input(name, dev)
    B, C = x.shape[:2]
    big = torch.full((B, C + 2) + tuple(size), -7.0, device=dev)
    big[:, 1:1 + C] = x
    sliced = big[:, 1:1 + C]
    assert sliced.data_ptr() != big.data_ptr() and sliced.stride(0) != x.stride(0)                  # strides of the larger buffer
    jobs = [(b,) + tuple(st) for b in range(B) for st in starts]
    for mask, cval in itertools.product(range(8), (0.0, -1.5)):
        for part in _launches(jobs):
            want = _aten_windows(x, roi, pad0, image, part, mask, cval)
            got = ops_raw.window_gather(lib, x, roi, part, mask, cval)
            assert got.dtype == torch.float32 and got.is_contiguous() and torch.equal(got, want), (name, mask, cval)
            assert torch.equal(ops_raw.window_gather(lib, sliced, roi, part, mask, cval), want), (name, mask, "channel slice")
            assert torch.equal(ops_raw.window_gather(lib, x, roi, part, mask, cval), got)          # two calls are bit-equal
    assert torch.equal(big[:, 0], torch.full_like(big[:, 0], -7.0)) and torch.equal(big[:, 1:1 + C], x)


def check_count(lib, name, dev):
    """against the slice-add loop of `sliding_window_inference`"""
    size, roi, image, pad0, starts = geometry(name)
    mode = EQUAL_CASES[name][4]
    weight = P.importance_map(roi, mode, 0.125, dev, torch.float32)
    want = torch.zeros(image, dtype=torch.float32, device=dev)
    for st in starts:
        want[_slices(st, roi)] += weight
    axis_starts = [sorted(set(st[d] for st in starts)) for d in range(3)]
    got = ops_raw.window_count(lib, weight, size, axis_starts)
    assert tuple(got.shape) == image and torch.equal(got, want), name
    assert torch.equal(ops_raw.window_count(lib, weight, size, axis_starts), got)
    # the weight map of the kernel route (its clamp bound stays on the device): the bits of `importance_map`, clamp active or not
    for m, sigma in (("gaussian", 0.125), ("gaussian", 1.0), ("constant", 0.125)):
        assert torch.equal(P._importance_map_no_sync(roi, m, sigma, dev), P.importance_map(roi, m, sigma, dev, torch.float32)), (m, sigma)


def check_blend(lib, name, dev):
    """one launch whose windows overlap (and span samples) against the sequential loop, for fp32, bf16 and fp16 predictions, on an
    accumulator that is not zero"""
    size, roi, image, pad0, starts = geometry(name)
    B = EQUAL_CASES[name][0][0]
    jobs = [(b,) + tuple(st) for b in range(B) for st in starts][:L.STITCH_MAX_WINDOWS]
    assert len(jobs) > 1
    g = torch.Generator().manual_seed(5)
    weight = P.importance_map(roi, "gaussian", 0.125, dev, torch.float32)
    base = (torch.rand((B, COUT) + image, generator=g) - 0.5).to(dev)
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        pred = ((torch.rand((len(jobs), COUT) + tuple(roi), generator=g) - 0.3) * 4).to(dtype).to(dev)
        want = base.clone()
        scaled = pred.to(torch.float32) * weight[None, None]
        for i, (b, *st) in enumerate(jobs):
            want[(slice(b, b + 1), slice(None)) + _slices(st, roi)] += scaled[i:i + 1]
        got = ops_raw.window_blend(lib, base.clone(), pred, weight, jobs)
        assert torch.equal(got, want), (name, dtype, float((got - want).abs().max()))
        assert torch.equal(ops_raw.window_blend(lib, base.clone(), pred, weight, jobs), got)
        # an unaligned window batch: the views of a split chunk start anywhere
        odd = torch.cat([pred.flatten()[:1], pred.flatten()])[1:].view(pred.shape)
        assert torch.equal(ops_raw.window_blend(lib, base.clone(), odd, weight, jobs), want), (name, dtype, "offset")


def check_finish(lib, name, dev):
    """two passes under different masks against (flip(a0 / c) + flip(a1 / c)) / 2 without the padding; acc is zero afterwards.  One
    pass without a flip: acc / count, cropped."""
    size, roi, image, pad0, starts = geometry(name)
    B = EQUAL_CASES[name][0][0]
    g = torch.Generator().manual_seed(9)
    count = (torch.rand(image, generator=g) * 3 + 0.25).to(dev)
    crop = (slice(None), slice(None)) + tuple(slice(p, p + s) for p, s in zip(pad0, size))

    def one(a, mask):
        q = (a / count)[crop]
        dims = flip_dims(mask, 2)
        return torch.flip(q, dims) if dims else q
    for m0, m1 in ((0, 7), (5, 2), (4, 4), (3, 6), (1, 0)):
        a0 = ((torch.rand((B, COUT) + image, generator=g) - 0.5) * 9).to(dev)
        a1 = ((torch.rand((B, COUT) + image, generator=g) - 0.5) * 9).to(dev)
        want = (one(a0, m0) + one(a1, m1)) / 2
        twice = []
        for _ in range(2):
            acc = a0.clone()
            total = torch.full((B, COUT) + tuple(size), float("nan"), device=dev)
            ops_raw.window_finish(lib, acc, count, total, roi, m0, 0, 2)
            assert torch.equal(acc, torch.zeros_like(acc)) and torch.equal(total, one(a0, m0)), (name, m0)
            acc.copy_(a1)
            got = ops_raw.window_finish(lib, acc, count, total, roi, m1, 1, 2)
            assert got is total and torch.equal(total, want), (name, m0, m1, float((total - want).abs().max()))
            assert torch.equal(acc, torch.zeros_like(acc))
            twice.append(total)
        assert torch.equal(twice[0], twice[1])
    acc = a0.clone()
    total = torch.empty((B, COUT) + tuple(size), device=dev)
    ops_raw.window_finish(lib, acc, count, total, roi)
    assert torch.equal(total, (a0 / count)[crop])


# ---- 4. no host round trip (GPU) ------------------------------------------------------------------------------------------------------------
def check_no_sync(dev):
    """one mirrored prediction on the kernel route with every synchronising call an error"""
    name = "gauss_half"
    x = case_input(name, dev)
    net = ramp_net(geometry(name)[1]).to(dev)
    aten, hip = inferers(name)
    axes = EQUAL_CASES[name][5]
    pred = P.Predictor(hip, axes, autocast_dtype=torch.float32)
    pred.maybe_mirror_and_predict(x, net, device=torch.device(dev))          # the library is loaded, the allocator is warm
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = pred.maybe_mirror_and_predict(x, net, device=torch.device(dev))
    finally:
        torch.cuda.set_sync_debug_mode(before)
    want = P.Predictor(aten, axes, autocast_dtype=torch.float32).maybe_mirror_and_predict(x, net, device=torch.device(dev))
    assert torch.equal(got, want)


# ---- 5. refusals and exports ----------------------------------------------------------------------------------------------------------------
def _base_args(t, kind):
    """valid arguments of one C entry on the tensors of `t`"""
    a = L.StitchArgs()
    a.batch, a.channels = 2, 2
    a.size[:], a.roi[:] = (6, 7, 8), (4, 4, 4)
    a.n_windows, a.passes = 2, 1
    a.window[0][:] = (0, 0, 0, 0)
    a.window[1][:] = (1, 2, 3, 4)
    for d, n in enumerate((2, 2, 2)):
        a.n_starts[d] = n
        a.starts[d][0], a.starts[d][1] = 0, (6, 7, 8)[d] - 4
    a.stride_b, a.stride_c, a.stride_z, a.stride_y, a.stride_x = t["volume"].stride()
    for key in ("volume", "windows_out", "weight", "count", "pred", "acc", "total"):
        setattr(a, key, t[key].data_ptr())
    return a


def check_c_refusals(lib, dev):
    """every refusal of the C entries returns its status with nothing launched: the output buffers keep their sentinel"""
    dll = lib.dll
    sentinel = -3.0
    t = {"volume": torch.full((2, 2, 6, 7, 8), sentinel, device=dev), "windows_out": torch.full((2, 2, 4, 4, 4), sentinel, device=dev),
         "weight": torch.full((4, 4, 4), sentinel, device=dev), "count": torch.full((6, 7, 8), sentinel, device=dev),
         "pred": torch.full((2, 2, 4, 4, 4), sentinel, device=dev), "acc": torch.full((2, 2, 6, 7, 8), sentinel, device=dev),
         "total": torch.full((2, 2, 6, 7, 8), sentinel, device=dev)}
    entries = {"gather": dll.segm_window_gather, "count": dll.segm_window_count, "blend": dll.segm_window_blend,
               "finish": dll.segm_window_finish}
    pointers = {"gather": ("volume", "windows_out"), "count": ("weight", "count"), "blend": ("pred", "weight", "acc"),
                "finish": ("acc", "count", "total")}

    def sets(**fields):
        def change(a):
            for k, v in fields.items():
                setattr(a, k, v)
        return change

    def item(field, index, value):
        def change(a):
            getattr(a, field)[index] = value
        return change

    def window(j, d, value):
        def change(a):
            a.window[j][d] = value
        return change

    def start(d, i, value):
        def change(a):
            a.starts[d][i] = value
        return change

    def plane_2_31(a):
        a.size[:] = (2048, 1024, 1024)

    shape, dtype, null = -2, -4, -1
    table = [("gather blend", sets(n_windows=0), shape), ("gather blend", sets(n_windows=65), shape),
             ("gather count blend finish", item("roi", 1, 0), shape), ("gather count blend finish", item("size", 2, 0), shape),
             ("gather count blend finish", item("size", 0, -1), shape), ("gather count blend finish", plane_2_31, shape),
             ("gather blend finish", sets(batch=0), shape), ("gather blend finish", sets(channels=0), shape),
             ("gather blend", window(1, 3, 5), shape), ("gather blend", window(0, 1, -1), shape), ("gather blend", window(1, 0, 2), shape),
             ("gather blend", window(1, 0, -1), shape),
             ("count", item("n_starts", 0, 0), shape), ("count", item("n_starts", 2, 65), shape), ("count", start(1, 1, 4), shape),
             ("count", start(2, 0, -1), shape),
             ("gather", sets(stride_x=2), shape), ("gather", sets(stride_z=-56), shape),
             ("gather finish", sets(mirror=8), shape), ("gather finish", sets(mirror=-1), shape),
             ("finish", sets(passes=0), shape), ("finish", sets(pass_=1), shape), ("finish", sets(pass_=-1), shape),
             ("blend", sets(dtype=3), dtype), ("blend", sets(dtype=-1), dtype)]
    for names, change, status in table:
        for kind in names.split():
            a = _base_args(t, kind)
            change(a)
            assert entries[kind](a) == status, (kind, status)
    for kind, fn in entries.items():
        assert fn(None) == null
        for key in pointers[kind]:
            a = _base_args(t, kind)
            setattr(a, key, None)
            assert fn(a) == null, (kind, key)
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    for key, v in t.items():
        assert torch.equal(v, torch.full_like(v, sentinel)), key


def check_wrapper_refusals(lib, dev):
    """the argument checks of segmamba_amd.ops_raw: shape, dtype, device, strides; the tensors stay what they were"""
    x = torch.rand((2, 2, 6, 7, 8), device=dev)
    keep = x.clone()
    roi = (4, 4, 4)
    ok = [(0, 0, 0, 0), (1, 2, 3, 4)]
    weight = torch.ones(roi, device=dev)
    acc = torch.zeros((2, 3, 6, 7, 8), device=dev)
    pred = torch.ones((2, 3) + roi, device=dev)
    count = torch.ones((6, 7, 8), device=dev)
    total = torch.zeros((2, 3, 6, 7, 8), device=dev)
    starts = [[0, 2], [0, 3], [0, 4]]
    for call in (lambda: ops_raw.window_gather(lib, x[0], roi, ok),                                       # wrong rank
                 lambda: ops_raw.window_gather(lib, x.half(), roi, ok),                                   # wrong dtype
                 lambda: ops_raw.window_gather(lib, x[..., ::2], roi, ok),                                # non-unit x stride
                 lambda: ops_raw.window_gather(lib, x, (4, 4), ok),
                 lambda: ops_raw.window_gather(lib, x, (4, 0, 4), ok),
                 lambda: ops_raw.window_gather(lib, x, roi, []),
                 lambda: ops_raw.window_gather(lib, x, roi, ok * 33),                                     # 66 windows
                 lambda: ops_raw.window_gather(lib, x, roi, [(0, 0, 0, 5)]),                              # leaves the image
                 lambda: ops_raw.window_gather(lib, x, roi, [(2, 0, 0, 0)]),                              # no such sample
                 lambda: ops_raw.window_gather(lib, x, roi, [(0, 0, 0)]),
                 lambda: ops_raw.window_gather(lib, x, roi, ok, mirror=8),
                 lambda: ops_raw.window_gather(lib, x, roi, ok, mirror=True),
                 lambda: ops_raw.window_count(lib, weight[0], (6, 7, 8), starts),
                 lambda: ops_raw.window_count(lib, weight.double(), (6, 7, 8), starts),
                 lambda: ops_raw.window_count(lib, weight[..., ::2], (6, 7, 8), starts),
                 lambda: ops_raw.window_count(lib, weight, (6, 7, 8), starts[:2]),
                 lambda: ops_raw.window_count(lib, weight, (6, 7, 8), [[0, 3], [0, 3], [0, 4]]),
                 lambda: ops_raw.window_count(lib, weight, (6, 7, 8), [[], [0, 3], [0, 4]]),
                 lambda: ops_raw.window_count(lib, weight, (6, 7, 8), [list(range(3)) * 22, [0, 3], [0, 4]]),
                 lambda: ops_raw.window_blend(lib, acc, pred[:1], weight, ok),                            # one prediction for two windows
                 lambda: ops_raw.window_blend(lib, acc, pred[:, :2], weight, ok),                         # channels differ
                 lambda: ops_raw.window_blend(lib, acc, pred.double(), weight, ok),
                 lambda: ops_raw.window_blend(lib, acc, pred.transpose(3, 4), weight, ok),                # not dense
                 lambda: ops_raw.window_blend(lib, acc.half(), pred, weight, ok),
                 lambda: ops_raw.window_blend(lib, acc, pred, weight[:2], ok),
                 lambda: ops_raw.window_blend(lib, acc, pred, weight, [(0, 0, 0, 0), (1, 3, 0, 0)]),
                 lambda: ops_raw.window_blend(lib, acc[..., :3], pred, weight, ok),
                 lambda: ops_raw.window_finish(lib, acc, count, total[0], roi),
                 lambda: ops_raw.window_finish(lib, acc[:, :2], count, total, roi),
                 lambda: ops_raw.window_finish(lib, acc, count[:5], total, roi),
                 lambda: ops_raw.window_finish(lib, acc, count.double(), total, roi),
                 lambda: ops_raw.window_finish(lib, acc, count, total, (4, 4, 9)),                        # image != acc's
                 lambda: ops_raw.window_finish(lib, acc, count, total, roi, mirror=9),
                 lambda: ops_raw.window_finish(lib, acc, count, total, roi, 0, 2, 2),
                 lambda: ops_raw.window_finish(lib, acc, count, total, roi, 0, 0, 0)):
        with pytest.raises(RuntimeError):
            call()
    if torch.device(dev).type == "cuda":
        for call in (lambda: ops_raw.window_blend(lib, acc, pred.cpu(), weight, ok),
                     lambda: ops_raw.window_finish(lib, acc, count.cpu(), total, roi)):
            with pytest.raises(RuntimeError):
                call()
    assert torch.equal(x, keep) and not acc.any() and not total.any()


def check_route_refusals(dev):
    """what `stitch="hip"` does not take raises with the reason; an unknown route is a ValueError; the default route is the ATen one"""
    x = torch.rand((1, 2, 10, 12, 12), device=dev)
    net = ramp_net((8, 8, 8)).to(dev)

    def hip(**kw):
        return P.SlidingWindowInferer(**dict(dict(roi_size=(8, 8, 8), sw_batch_size=2, overlap=0.5, mode="gaussian", stitch="hip"), **kw))
    with pytest.raises(NotImplementedError, match="float32"):
        hip()(x.half(), net)
    with pytest.raises(NotImplementedError, match="3-D"):
        P.SlidingWindowInferer(roi_size=(8, 8), sw_batch_size=2, stitch="hip")(x[:, :, 0], lambda w: w)
    with pytest.raises(NotImplementedError, match="padding_mode"):
        hip(padding_mode="reflect")(x, net)
    with pytest.raises(NotImplementedError, match="float32"):
        P.sliding_window_inference(x.double(), (8, 8, 8), 2, net, stitch="hip")
    with pytest.raises(RuntimeError, match="window's spatial size"):
        hip()(x, lambda w: w[..., :4])
    with pytest.raises(ValueError, match="cosine"):
        P.SlidingWindowInferer(roi_size=(8, 8, 8), stitch="cosine")
    with pytest.raises(ValueError, match="cosine"):
        P.sliding_window_inference(x, (8, 8, 8), 2, net, stitch="cosine")
    with pytest.raises(ValueError):
        hip(overlap=1.0)(x, net)
    default = P.SlidingWindowInferer(roi_size=(8, 8, 8), sw_batch_size=2, overlap=0.5, mode="gaussian")
    aten = P.SlidingWindowInferer(roi_size=(8, 8, 8), sw_batch_size=2, overlap=0.5, mode="gaussian", stitch="aten")
    assert default.stitch == "aten"
    with torch.no_grad():
        assert torch.equal(default(x, net), aten(x, net))
        assert torch.equal(P.sliding_window_inference(x, (8, 8, 8), 2, net, 0.5, "gaussian"),
                           P.sliding_window_inference(x, (8, 8, 8), 2, net, 0.5, "gaussian", stitch="aten"))
    both = [P.Predictor(i, [0, 2], autocast_dtype=torch.float32).maybe_mirror_and_predict(x, net, device=torch.device(dev))
            for i in (default, aten)]
    assert torch.equal(both[0], both[1])


def check_needs_the_device():
    """host tensors without the emulated library: the kernel route says why it refuses"""
    x = torch.rand((1, 1, 8, 8, 8))
    hip = P.SlidingWindowInferer(roi_size=(4, 4, 4), sw_batch_size=2, stitch="hip")
    with pytest.raises(RuntimeError, match="GPU"):
        hip(x, lambda w: w)
    with pytest.raises(RuntimeError, match="GPU"):
        P.Predictor(hip, [0]).maybe_mirror_and_predict(x, torch.nn.Identity())


def check_exports(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "segmamba_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name + "(" in hdr and name in L.EXPORTS and hasattr(lib.dll, name), name
    assert lib.missing == []
    assert lib.dll.segm_abi_version() == 10 == L.header_abi_version()
    assert os.path.exists(os.path.join(root, "segmamba_amd", "csrc", "stitch.hip"))
    for name in ("window_gather", "window_count", "window_blend", "window_finish"):
        assert callable(getattr(ops_raw, name))
    assert L.STITCH_MAX_WINDOWS == 64 and "#define SEGM_STITCH_MAX_WINDOWS 64" in hdr
