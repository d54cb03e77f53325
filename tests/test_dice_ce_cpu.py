"""Host side of softmax Dice + cross entropy on the device (segmamba_amd/losses.py: softmax_dice_sums, the device_sums keyword) without
a GPU: softmax_dice_sums on CPU tensors against dice_ce_sums and the float64 restatement, the keyword's plumbing through the four
classes, the unchanged behaviour of the default, and one step of a tiny SegMamba through
build_training_state(loss_fn=DC_and_CE_loss(..., device_sums=True)) on the emulated library."""
import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd.losses import (DC_and_CE_loss, DC_and_topk_loss, MemoryEfficientSoftDiceLoss, SoftDiceLoss, dice_ce_sums,
                                 softmax_dice_sums, softmax_helper_dim1)
from tests import dice_ce_checks as K
from tests import loss_ref as R


def test_softmax_dice_sums_on_cpu_tensors_equals_dice_ce_sums():
    rs = np.random.RandomState(71)
    logits, labels, m = K.make_case(rs, 2, 4, (3, 5, 7), True, True)
    x = torch.from_numpy(logits)
    want = R.sums(x.double(), labels, m, K.IGNORE)
    for tgt in (torch.from_numpy(labels), torch.from_numpy(labels).float().unsqueeze(1), torch.from_numpy(labels).to(torch.int16)):
        for mask in (torch.from_numpy(m), torch.from_numpy(m).bool().unsqueeze(1), torch.from_numpy(m).float()):
            got = softmax_dice_sums(x, tgt, mask, K.IGNORE)
            ref = dice_ce_sums(x, tgt, mask, K.IGNORE)
            assert len(got) == 5
            for a, b in zip(got, ref):
                assert torch.equal(a, b)
            for name, a, w in zip("IPGCN", got, want):          # fp32 sums on this path: 1e-5 of the float64 restatement
                assert np.allclose(a.double().numpy(), w.numpy(), rtol=1e-5, atol=0), name
    grads = []
    for fn in (softmax_dice_sums, dice_ce_sums):            # differentiable through I, P and CE alike
        xg = x.clone().requires_grad_(True)
        I, P, G, CE, N = fn(xg, torch.from_numpy(labels), None, K.IGNORE)
        assert I.requires_grad and P.requires_grad and CE.requires_grad and not G.requires_grad and not N.requires_grad
        (I.sum() + 2 * P.sum() + 0.5 * CE.sum()).backward()
        grads.append(xg.grad)
    assert torch.equal(grads[0], grads[1]) and grads[0].abs().max() > 0
    with pytest.raises(ValueError):
        softmax_dice_sums(x[0, 0, 0], torch.from_numpy(labels))
    with pytest.raises(NotImplementedError, match="one-hot"):
        softmax_dice_sums(x, torch.zeros_like(x))


def test_device_sums_keyword_plumbing():
    kw = dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False)
    for cls in (SoftDiceLoss, MemoryEfficientSoftDiceLoss):
        assert cls(softmax_helper_dim1).device_sums is False and cls(softmax_helper_dim1, device_sums=True).device_sums is True
    assert SoftDiceLoss(softmax_helper_dim1, True, False, 1e-5, False, 0.5, True).device_sums is True        # after clip_tp
    assert MemoryEfficientSoftDiceLoss(softmax_helper_dim1, True, False, 1e-5, False, True).device_sums is True
    ce = DC_and_CE_loss(kw, {}, device_sums=True)
    assert ce.device_sums is True and DC_and_CE_loss(kw, {}).device_sums is False
    assert DC_and_CE_loss(kw, {}, 1, 1, None, MemoryEfficientSoftDiceLoss, True).device_sums is True
    tk = DC_and_topk_loss(kw, {}, device_sums=True)
    assert tk.device_sums is True and tk.dc.device_sums is True
    plain = DC_and_topk_loss(kw, {})
    assert plain.device_sums is False and plain.dc.device_sums is False
    assert DC_and_topk_loss(kw, {}, 1, 1, None, True).device_sums is True


def test_device_sums_changes_nothing_for_cpu_tensors():
    """CPU tensors take the ATen formulas whatever the keyword says: the same bits, value and gradient, dtype included"""
    g = K.golden()
    for i, c in enumerate(g["cases"]):
        tgt = torch.from_numpy(g["target_ignore"] if c["ignore_label"] is not None else g["target"])
        out = []
        for flag in (False, True):
            x = torch.from_numpy(g["logits"]).clone().requires_grad_(True)
            loss = K.class_of(c, device_sums=flag)(x, tgt)
            loss.backward()
            out.append((loss.detach(), x.grad))
        assert out[0][0].dtype == out[1][0].dtype and torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), c
    x, y = torch.from_numpy(g["logits"]), torch.from_numpy(g["target"])
    kw = dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False)
    assert torch.equal(DC_and_topk_loss(kw, dict(k=10), device_sums=True)(x, y), DC_and_topk_loss(kw, dict(k=10))(x, y))
    # a non-softmax apply_nonlin stays honoured on CPU tensors
    assert torch.equal(SoftDiceLoss(None, ddp=False, device_sums=True)(torch.softmax(x, 1), y), SoftDiceLoss(None, ddp=False)(torch.softmax(x, 1), y))


def test_the_default_still_refuses_a_device_and_device_sums_asks_for_the_kernel(monkeypatch):
    """with on_device forced and no library behind it: the default raises NotImplementedError as before; device_sums=True goes for
    the wrappers of the two entries (replaced here, nothing is launched) and refuses a non-softmax apply_nonlin"""
    from segmamba_amd import ops_raw
    monkeypatch.setattr(L, "on_device", lambda t: True)
    x, y = torch.zeros(2, 4, 3, 5, 7), torch.zeros(2, 1, 3, 5, 7)
    kw = {"ddp": False}
    for mod in (SoftDiceLoss(softmax_helper_dim1, ddp=False), MemoryEfficientSoftDiceLoss(softmax_helper_dim1, ddp=False),
                DC_and_CE_loss(kw, {}), DC_and_CE_loss(kw, {}, device_sums=False)):
        with pytest.raises(NotImplementedError):
            mod(x, y)
    with pytest.raises(NotImplementedError):
        dice_ce_sums(x, y)
    for mod in (SoftDiceLoss(torch.sigmoid, ddp=False, device_sums=True), MemoryEfficientSoftDiceLoss(None, ddp=False, device_sums=True)):
        with pytest.raises(NotImplementedError, match="softmax"):
            mod(x, y)
    calls = []

    def fake_fwd(lib, logits, labels, mask=None, ignore_label=None, workspace=None):
        calls.append((tuple(labels.shape), labels.dtype, None if mask is None else mask.dtype, ignore_label))
        B, Cc = logits.shape[:2]
        return tuple(torch.ones(B, Cc, dtype=torch.float64) for _ in range(3)) + tuple(torch.ones(B, dtype=torch.float64) for _ in range(2))
    monkeypatch.setattr(ops_raw, "softmax_dice_fwd", fake_fwd)
    monkeypatch.setattr(L, "get_lib", lambda: None)
    out = DC_and_CE_loss(kw, {}, ignore_label=4, device_sums=True)(x, y)
    assert out.dtype == torch.float32 and calls[-1] == ((2, 3, 5, 7), torch.float32, None, 4)
    out = SoftDiceLoss(softmax_helper_dim1, ddp=False, device_sums=True)(x, y.long()[:, 0], loss_mask=torch.ones(2, 1, 3, 5, 7, dtype=torch.bool))
    assert out.dtype == torch.float32 and calls[-1] == ((2, 3, 5, 7), torch.int64, torch.uint8, None)


def test_build_training_state_trains_with_the_device_sums(monkeypatch):
    """SegMamba(out_chans=4) takes one step with DC_and_CE_loss(device_sums=True) from the (B, D, H, W) int64 labels the feeders
    produce; trainer.py is as it was.  The model has no CPU kernels of its own, so it runs on the emulated library, and so does the
    loss."""
    from tests import emu_util
    if not emu_util.emu_available():
        pytest.skip("no host clang for the emulation build")
    monkeypatch.setattr(L, "_lib", emu_util.emu_lib())
    monkeypatch.setattr(L, "on_device", lambda t: True)
    from segmamba_amd.segmamba import SegMamba
    from segmamba_amd.trainer import build_training_state, train_step
    torch.manual_seed(0)
    net = SegMamba(in_chans=4, out_chans=4, depths=[1, 1, 1, 1], feat_size=[48, 8, 16, 32], hidden_size=32)
    fn = DC_and_CE_loss(dict(batch_dice=True, do_bg=False, smooth=1e-5, ddp=False), {}, dice_class=MemoryEfficientSoftDiceLoss,
                        device_sums=True)
    st = build_training_state(torch.device("cpu"), model=net, loss_fn=fn)
    assert st.loss_fn is fn
    g = torch.Generator().manual_seed(3)
    img, lab = torch.rand(1, 4, 32, 32, 32, generator=g), torch.randint(0, 4, (1, 32, 32, 32), generator=g)
    before = [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        want = float(fn(net(img), lab))
    loss = float(train_step(st, img, lab))
    # the step computes with the parameter bank's bf16 copies of the weights, `want` with the fp32 weights: every weight is off by up
    # to 2^-9 relative, through some twenty layers; 3e-2 is the width tests/test_losses_cpu.py and tests/test_region_loss_cpu.py give
    # the same comparison of a step with a no-grad forward
    assert np.isfinite(loss) and abs(loss - want) <= 3e-2 * abs(want)
    assert any((a - b.detach()).abs().max() > 0 for a, b in zip(before, net.parameters()))
