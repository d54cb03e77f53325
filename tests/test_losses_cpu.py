"""Host side of the Dice + cross-entropy loss (segmamba_amd/losses.py) without a GPU: the float64 restatement (tests/loss_ref.py)
against the reference's own recorded values, the CPU path of every class against the restatement, the refusals, the all-ignored rule,
DeepSupervisionWrapper, build_training_state(loss_fn=...), and ddp=True with batch_dice=True in two gloo processes."""
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from segmamba_amd import lib as L
from segmamba_amd.losses import (DC_and_CE_loss, DeepSupervisionWrapper, MemoryEfficientSoftDiceLoss, RobustCrossEntropyLoss,
                                 SoftDiceLoss, softmax_helper_dim1)
from tests import loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dice_ce.npz")
# fp32 resolution: what the reference's own fp32 run and the ATen path are held to against float64
LOSS_RTOL, GRAD_TOL = 1e-6, 1e-6


def _golden():
    g = np.load(GOLDEN)
    return g, json.loads(str(g["cases"]))


def _module(c):
    kw = dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"], ddp=False)
    if c.get("clip_tp") is not None:
        kw["clip_tp"] = c["clip_tp"]
    return DC_and_CE_loss(kw, {}, weight_ce=c.get("weight_ce", 1), weight_dice=c.get("weight_dice", 1), ignore_label=c.get("ignore_label"),
                          dice_class=SoftDiceLoss if c["kind"] == "soft" else MemoryEfficientSoftDiceLoss)


def _ref(c, x, y):
    return R.value_and_grad(R.dc_and_ce, x, y, c["kind"], c["batch_dice"], c["do_bg"], c["smooth"], c.get("weight_ce", 1),
                            c.get("weight_dice", 1), c.get("ignore_label"), c.get("clip_tp"))


def _run(mod, x, target):
    xt = torch.as_tensor(x).clone().requires_grad_(True)
    loss = mod(xt, target)
    loss.backward()
    return float(loss.detach()), xt.grad.numpy().astype(np.float64)


def test_restatement_equals_the_recorded_reference():
    """tests/loss_ref.py in float64 against the reference's DC_and_CE_loss run in fp32 (14 recorded configurations)"""
    g, cases = _golden()
    assert len(cases) == 14 and os.path.getsize(GOLDEN) < 100 * 1000
    assert {c["kind"] for c in cases} == {"soft", "mem"} and any(c["clip_tp"] for c in cases) and any(c["ignore_label"] == 4 for c in cases)
    assert any(c["weight_ce"] == 0 for c in cases) and any(c["weight_dice"] == 0 for c in cases)
    assert (g["target_ignore"] == 4).sum() == 42 + 35 and g["target"].shape == (2, 1, 5, 6, 7)
    for i, c in enumerate(cases):
        y = (g["target_ignore"] if c["ignore_label"] is not None else g["target"])[:, 0].astype(np.int64)
        v, gr = _ref(c, g["logits"], y)
        assert abs(v - g["loss"][i]) <= LOSS_RTOL * abs(g["loss"][i]), c
        assert np.abs(gr - g["grad"][i]).max() <= GRAD_TOL * np.abs(g["grad"][i]).max(), c


def test_cpu_path_equals_the_recorded_reference_and_the_restatement():
    g, cases = _golden()
    for i, c in enumerate(cases):
        tgt = g["target_ignore"] if c["ignore_label"] is not None else g["target"]
        loss, grad = _run(_module(c), g["logits"], torch.as_tensor(tgt))
        assert abs(loss - g["loss"][i]) <= 2 * LOSS_RTOL * abs(g["loss"][i]), c                 # fp32 on both sides
        assert np.abs(grad - g["grad"][i]).max() <= 2 * GRAD_TOL * np.abs(g["grad"][i]).max(), c
        v, gr = _ref(c, g["logits"], tgt[:, 0].astype(np.int64))
        assert abs(loss - v) <= LOSS_RTOL * abs(v) and np.abs(grad - gr).max() <= GRAD_TOL * np.abs(gr).max(), c


@pytest.mark.parametrize("kind", ["soft", "mem"])
def test_dice_classes_cpu_path(kind):
    """the Dice classes on their own: every batch_dice / do_bg, smooth 0 / 1e-5 / 1, a loss_mask in three dtypes, labels as
    (B, 1, ...) float and (B, ...) int64, and apply_nonlin=None honoured on CPU tensors (the input is taken as probabilities)"""
    rng = np.random.default_rng(11)
    x = (2 * rng.standard_normal((2, 5, 4, 6, 9))).astype(np.float32)
    y = rng.integers(0, 5, (2, 4, 6, 9))
    y[1][y[1] == 3] = 0                                     # class 3 never occurs in sample 1
    m = rng.random(y.shape) < 0.6
    cls = SoftDiceLoss if kind == "soft" else MemoryEfficientSoftDiceLoss
    for batch_dice in (False, True):
        for do_bg in (False, True):
            for smooth in (0.0, 1e-5, 1.0):
                mod = cls(apply_nonlin=softmax_helper_dim1, batch_dice=batch_dice, do_bg=do_bg, smooth=smooth, ddp=True)   # no group: ddp is idle
                v, gr = R.value_and_grad(R.dice, x, y, kind, batch_dice, do_bg, smooth)
                for tgt in (torch.as_tensor(y.astype(np.float32))[:, None], torch.as_tensor(y)):
                    loss, grad = _run(mod, x, tgt)
                    assert abs(loss - v) <= LOSS_RTOL * abs(v) and np.abs(grad - gr).max() <= GRAD_TOL * np.abs(gr).max()
                vm, _ = R.value_and_grad(R.dice, x, y, kind, batch_dice, do_bg, smooth, mask=m)
                for dt in (torch.bool, torch.uint8, torch.float32):
                    lm = float(mod(torch.as_tensor(x), torch.as_tensor(y), loss_mask=torch.as_tensor(m)[:, None].to(dt)))
                    assert abs(lm - vm) <= LOSS_RTOL * abs(vm)
    p = torch.softmax(torch.as_tensor(x), 1)
    raw = cls(apply_nonlin=None, batch_dice=True, do_bg=False, smooth=1e-5, ddp=False)(p, torch.as_tensor(y))
    v, _ = R.value_and_grad(R.dice, x, y, kind, True, False, 1e-5)
    assert abs(float(raw) - v) <= LOSS_RTOL * abs(v)
    if kind == "soft":
        tp1 = float(R.sums(torch.as_tensor(x, dtype=torch.float64), y)[0].sum(0)[1])
        v, gr = R.value_and_grad(R.dice, x, y, "soft", True, True, 1e-5, clip_tp=tp1 + 1.0)
        loss, grad = _run(SoftDiceLoss(softmax_helper_dim1, True, True, 1e-5, False, clip_tp=tp1 + 1.0), x, torch.as_tensor(y))
        assert abs(loss - v) <= LOSS_RTOL * abs(v) and np.abs(grad - gr).max() <= GRAD_TOL * np.abs(gr).max()


def test_robust_cross_entropy_cpu_path():
    rng = np.random.default_rng(12)
    x = (2 * rng.standard_normal((2, 4, 3, 5, 7))).astype(np.float32)
    y = rng.integers(0, 4, (2, 3, 5, 7))
    y.reshape(-1)[::7] = 4
    v, gr = R.value_and_grad(R.cross_entropy, x, y, 4)
    mod = RobustCrossEntropyLoss(ignore_index=4)
    assert mod.ignore_index == 4 and RobustCrossEntropyLoss().ignore_index == -100
    for tgt in (torch.as_tensor(y.astype(np.float32))[:, None], torch.as_tensor(y)):
        loss, grad = _run(mod, x, tgt)
        assert abs(loss - v) <= LOSS_RTOL * abs(v) and np.abs(grad - gr).max() <= GRAD_TOL * np.abs(gr).max()


def test_refusals(monkeypatch):
    for kw in (dict(weight=torch.ones(4)), dict(label_smoothing=0.1), dict(reduction="sum"), dict(reduction="none"),
               dict(size_average=True), dict(reduce=False)):
        with pytest.raises(NotImplementedError):
            RobustCrossEntropyLoss(**kw)
        with pytest.raises(NotImplementedError):
            DC_and_CE_loss({}, kw)
    ce_kwargs = {}
    mod = DC_and_CE_loss({"ddp": False}, ce_kwargs, ignore_label=3)
    assert mod.ce.ignore_index == 3 and mod.dc.apply_nonlin is softmax_helper_dim1 and isinstance(mod.dc, SoftDiceLoss)
    assert DC_and_CE_loss({}, {"ignore_index": 7}).ce.ignore_index == 7
    x = torch.zeros(2, 4, 3, 5, 7)
    with pytest.raises(NotImplementedError, match="one-hot"):
        MemoryEfficientSoftDiceLoss(softmax_helper_dim1, ddp=False)(x, torch.zeros_like(x))
    with pytest.raises(ValueError):
        SoftDiceLoss(softmax_helper_dim1, ddp=False)(x, torch.zeros(2, 3, 5, 8))
    with pytest.raises(TypeError):
        DeepSupervisionWrapper(lambda a, b: a)(x, x)
    with pytest.raises(NotImplementedError, match="one-hot"):
        DC_and_CE_loss({"ddp": False}, {})(x, torch.zeros_like(x))
    zero = DC_and_CE_loss({"ddp": False}, {}, weight_ce=0, weight_dice=0)(x, torch.zeros(2, 1, 3, 5, 7))
    assert torch.is_tensor(zero) and float(zero) == 0.0


def test_device_tensors_are_refused_not_served_by_aten(monkeypatch):
    """the repository's rule: no quiet fall-back to eager PyTorch on the device.  The Dice sums have no kernel, so whatever needs them
    refuses a tensor the library would take; RobustCrossEntropyLoss is not affected (it has train_ops.cross_entropy)."""
    monkeypatch.setattr(L, "on_device", lambda t: True)
    x, y = torch.zeros(2, 4, 3, 5, 7), torch.zeros(2, 1, 3, 5, 7)
    for mod in (SoftDiceLoss(softmax_helper_dim1, ddp=False), MemoryEfficientSoftDiceLoss(None, ddp=False), DC_and_CE_loss({"ddp": False}, {})):
        with pytest.raises(NotImplementedError):
            mod(x, y)


def test_wrong_labels_give_nan_not_a_silent_value():
    """a label outside [0, classes) that is not ignored, and a float label that is no integer: NaN in the loss, for both Dice classes
    and the CE term; the same label as ignore_label is fine; the other sample's sums stay finite"""
    from segmamba_amd.losses import dice_ce_sums
    rng = np.random.default_rng(13)
    x = torch.as_tensor((2 * rng.standard_normal((2, 4, 3, 5, 7))).astype(np.float32))
    y = rng.integers(0, 4, (2, 1, 3, 5, 7))
    for bad, dtype in ((7, torch.int64), (-1, torch.int16), (1.5, torch.float32), (float("nan"), torch.float32)):
        t = torch.as_tensor(y.astype(np.float64))
        t[0, 0, 1, 2, 3] = bad
        t = t.to(dtype)
        I, P, G, ce, n = dice_ce_sums(x, t)
        assert torch.isnan(I[0]).all() and torch.isnan(P[0]).all() and torch.isnan(ce[0]) and int(n[0]) == 105
        assert torch.isfinite(I[1]).all() and torch.isfinite(P[1]).all() and torch.isfinite(ce[1]) and int(G[1].sum()) == 105
        for cls in (SoftDiceLoss, MemoryEfficientSoftDiceLoss):
            assert torch.isnan(DC_and_CE_loss(dict(batch_dice=True, ddp=False), {}, dice_class=cls)(x, t))
            assert torch.isnan(cls(softmax_helper_dim1, ddp=False)(x, t))
    t = torch.as_tensor(y.astype(np.float32))
    t[0, 0, 1, 2, 3] = 7
    assert torch.isfinite(DC_and_CE_loss({"ddp": False}, {}, ignore_label=7)(x, t))
    v, _ = R.value_and_grad(R.dc_and_ce, x.numpy(), t[:, 0].numpy().astype(np.int64), "soft", False, True, 1.0, ignore=7)
    assert abs(float(DC_and_CE_loss({"ddp": False}, {}, ignore_label=7)(x, t)) - v) <= LOSS_RTOL * abs(v)


def test_all_ignored_batch_gives_zero_ce_and_a_finite_loss():
    x = torch.randn(2, 4, 3, 5, 7, generator=torch.Generator().manual_seed(1))
    tgt = torch.full((2, 1, 3, 5, 7), 4.0)
    ce_only = DC_and_CE_loss({"ddp": False}, {}, weight_dice=0, ignore_label=4)
    assert float(ce_only(x, tgt)) == 0.0
    both = DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, ignore_label=4, dice_class=MemoryEfficientSoftDiceLoss)
    loss, grad = _run(both, x.numpy(), tgt)
    assert np.isfinite(loss) and not grad.any()


def test_deep_supervision_wrapper_weights():
    calls = []

    def loss(a, b):
        calls.append((a, b))
        return a.sum() - b.sum()
    outs = [torch.full((2,), float(i + 1)) for i in range(3)]
    tgts = [torch.full((2,), 0.5 * i) for i in range(3)]
    w = [1.0, 0.5, 0.25]
    got = DeepSupervisionWrapper(loss, w)(outs, tgts)
    assert float(got) == sum(wi * float(o.sum() - t.sum()) for wi, o, t in zip(w, outs, tgts)) and len(calls) == 3
    assert float(DeepSupervisionWrapper(loss)(tuple(outs), tuple(tgts))) == sum(float(o.sum() - t.sum()) for o, t in zip(outs, tgts))
    mod = DeepSupervisionWrapper(DC_and_CE_loss({"ddp": False}, {}), [1.0, 0.0])
    x = torch.randn(1, 3, 4, 4, 4, generator=torch.Generator().manual_seed(2))
    y = torch.zeros(1, 1, 4, 4, 4)
    assert torch.equal(mod([x, x[..., :2]], [y, y[..., :2]]), mod.loss(x, y))


def test_build_training_state_uses_the_given_loss():
    from segmamba_amd.trainer import build_training_state, train_step
    torch.manual_seed(0)
    net = nn.Sequential(nn.Conv3d(4, 8, 3, padding=1), nn.LeakyReLU(0.01), nn.Conv3d(8, 4, 1))
    mod = DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, dice_class=MemoryEfficientSoftDiceLoss)
    st = build_training_state(torch.device("cpu"), model=net, loss_fn=mod)
    assert st.loss_fn is mod
    g = torch.Generator().manual_seed(3)
    img, lab = torch.rand(2, 4, 8, 8, 8, generator=g), torch.randint(0, 4, (2, 8, 8, 8), generator=g)     # (B, D, H, W) int64
    with torch.no_grad():
        want = float(mod(net(img), lab))
    assert abs(float(train_step(st, img, lab)) - want) <= 3e-2 * abs(want)        # autocast bf16 inside the step
    default = build_training_state(torch.device("cpu"), model=net)
    assert isinstance(default.loss_fn, nn.CrossEntropyLoss)


# ---- ddp=True, batch_dice=True over two gloo ranks --------------------------------------------------------------------------------------
def _ddp_case():
    rng = np.random.default_rng(21)
    x = (2 * rng.standard_normal((4, 4, 3, 5, 7))).astype(np.float32)
    y = rng.integers(0, 4, (4, 1, 3, 5, 7)).astype(np.float32)
    return x, y


def _ddp_worker(rank, world, port, out, kind):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, y = _ddp_case()
    mod = DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=True), {}, weight_ce=0,
                         dice_class=SoftDiceLoss if kind == "soft" else MemoryEfficientSoftDiceLoss)
    loss, grad = _run(mod, x[2 * rank:2 * rank + 2], torch.as_tensor(y[2 * rank:2 * rank + 2]))
    out[rank] = (loss, grad)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["soft", "mem"])
def test_two_process_batch_dice_sums_over_the_ranks(kind):
    """the loss on both ranks is the single-process loss on the concatenated batch; the gradient is the world size times that loss's
    gradient on the rank's own half - what the reference's AllGatherGrad.apply(t).sum(0) gives (its backward all-reduces)"""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_ddp_worker, args=(2, port, out, kind), nprocs=2, join=True)
    x, y = _ddp_case()
    v, gr = R.value_and_grad(R.dice, x, y[:, 0].astype(np.int64), kind, True, False, 1e-5)
    for rank in (0, 1):
        loss, grad = out[rank]
        assert abs(loss - v) <= LOSS_RTOL * abs(v)
        want = 2 * gr[2 * rank:2 * rank + 2]
        assert np.abs(grad - want).max() <= GRAD_TOL * np.abs(want).max()
    assert out[0][0] == out[1][0]
