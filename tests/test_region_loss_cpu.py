"""Host side of the region-based loss (segmamba_amd/losses.py: DC_and_BCE_loss, region_sums, region_targets) without a GPU: the float64
restatement (tests/region_loss_ref.py) against the reference's own recorded values (tests/golden/region_bce.npz), the CPU path of the
class against both, region_targets, DeepSupervisionWrapper, build_training_state(loss_fn=...) on a tiny SegMamba(out_chans=3), and the
refusal of the Dice classes for a "device"."""
import numpy as np
import pytest
import torch

from segmamba_amd import lib as L
from segmamba_amd.losses import (BRATS_REGIONS, DC_and_BCE_loss, DeepSupervisionWrapper, MemoryEfficientSoftDiceLoss, SoftDiceLoss,
                                 region_sums, region_targets)
from tests import region_loss_checks as K
from tests import region_loss_ref as R

LOSS_RTOL, GRAD_TOL = 1e-6, 1e-6


def _mask_of(g, c):
    return (1 - g["ignore"][:, None]).astype(bool) if c["use_ignore_label"] else None


def test_restatement_equals_the_recorded_reference():
    """tests/region_loss_ref.py in float64 against the reference's DC_and_BCE_loss run in fp32 (13 recorded configurations): loss 1e-6
    relative, gradient 1e-6 x max |gradient|"""
    g = K.golden()
    assert len(g["cases"]) == 13
    for i, c in enumerate(g["cases"]):
        tgt = g["target_soft"] if c["soft_target"] else g["target"]
        v, gr = R.value_and_grad(R.dc_and_bce, g["logits"], tgt, _mask_of(g, c), c["kind"], c["batch_dice"], c["do_bg"], c["smooth"],
                                 c["weight_ce"], c["weight_dice"])
        assert abs(v - float(g["loss"][i])) <= LOSS_RTOL * abs(float(g["loss"][i])), (c, v, float(g["loss"][i]))
        assert np.abs(gr - g["grad"][i]).max() <= GRAD_TOL * np.abs(g["grad"][i]).max(), c


def test_cpu_path_equals_the_recorded_reference_and_the_restatement():
    """measured for the sums formulation against the reference on CPU: <= 1.4e-7 absolute on losses of 0.56 - 2.7"""
    g = K.golden()
    worst = 0.0
    for i, c in enumerate(g["cases"]):
        loss, grad = K.run(K.class_of(c), g["logits"], K.golden_target(g, c), torch.float32, "cpu")
        worst = max(worst, abs(loss - float(g["loss"][i])))
        assert abs(loss - float(g["loss"][i])) <= K.LOSS_RTOL * abs(float(g["loss"][i])), (c, loss)
        assert np.abs(grad - g["grad"][i]).max() <= GRAD_TOL * np.abs(g["grad"][i]).max(), c
        tgt = g["target_soft"] if c["soft_target"] else g["target"]
        v, gr = R.value_and_grad(R.dc_and_bce, g["logits"], tgt, _mask_of(g, c), c["kind"], c["batch_dice"], c["do_bg"], c["smooth"],
                                 c["weight_ce"], c["weight_dice"])
        assert abs(loss - v) <= K.LOSS_RTOL * abs(v) and np.abs(grad - gr).max() <= GRAD_TOL * np.abs(gr).max(), c
    print(f"CPU path against the recording: worst absolute loss difference {worst:.2e}")


def test_cpu_label_mode_edge_cases_and_strides():
    K.check_label_mode_equals_plane_mode("cpu")
    K.check_classes_edge_cases("cpu")
    K.check_strided_logits_through_the_class("cpu")


def test_region_sums_cpu_against_the_definition():
    """the five sums on CPU tensors: every label dtype, a plane target with the ignore plane, wrong labels give NaN in their sample"""
    rs = np.random.RandomState(51)
    logits, labels, masks, m, planes = K.make_case(rs, 2, 3, (3, 5, 7), True)
    regions = [[l for l in range(32) if (mk >> l) & 1] for mk in masks]
    want = R.sums(logits, planes, m)
    lab = labels.copy()
    lab[m == 0] = 40
    for dt in K.LABEL_DTYPES:
        got = region_sums(torch.from_numpy(logits), torch.from_numpy(lab).to(dt), regions, ignore_label=40)
        K.assert_sums(got, want, dt)
    pl = torch.from_numpy(np.concatenate([planes, 1.0 - m[:, None]], 1))
    for dt in K.PLANE_DTYPES:
        K.assert_sums(region_sums(torch.from_numpy(logits), pl.to(dt), use_ignore_label=True), want, dt)
    for value, dt in ((32, torch.int64), (-3, torch.int16), (1.5, torch.float32)):
        bad = torch.from_numpy(lab.copy()).to(dt)
        bad[1].view(-1)[16] = value
        I, P, G, E, N = region_sums(torch.from_numpy(logits), bad, regions, ignore_label=40)
        for s in (I, P, E):
            assert torch.isnan(s[1]).all() and torch.isfinite(s[0]).all()
        assert torch.isfinite(G).all() and torch.equal(N, torch.from_numpy(want[4]))


def test_region_targets_equals_the_three_compares():
    labels = torch.randint(0, 5, (2, 5, 6, 7), generator=torch.Generator().manual_seed(2))
    want = torch.stack([(labels == 1) | (labels == 3), (labels == 1) | (labels == 3) | (labels == 2), labels == 3], 1).float()
    got = region_targets(labels)
    assert got.dtype == torch.float32 and torch.equal(got, want) and torch.equal(region_targets(labels, BRATS_REGIONS), want)
    assert torch.equal(region_targets(labels.float()), want)
    assert torch.equal(region_targets(labels, ((0,), (4, 2))), torch.stack([labels == 0, (labels == 4) | (labels == 2)], 1).float())


def test_refusals_on_cpu_tensors(monkeypatch):
    K.check_refusals_host("cpu")


def test_deep_supervision_wrapper_weights():
    g = K.golden()
    x, y = torch.from_numpy(g["logits"]), torch.from_numpy(g["labels"])
    fn = DC_and_BCE_loss({}, dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False), regions=BRATS_REGIONS)
    mod = DeepSupervisionWrapper(fn, weight_factors=(1.0, 0.5, 0.25))
    xs, ys = [x, x[..., ::2], x[..., ::4]], [y, y[..., ::2], y[..., ::4]]
    want = sum(w * fn(a, b) for w, a, b in zip((1.0, 0.5, 0.25), xs, ys))
    assert torch.allclose(mod(xs, ys), want, rtol=1e-6, atol=0)


def test_build_training_state_trains_a_region_model(monkeypatch):
    """SegMamba(out_chans=3) takes one step from the (B, D, H, W) int64 labels the feeders produce; trainer.py is as it was.  The model
    has no CPU kernels of its own, so it runs on the emulated library, and so does the loss."""
    from tests import emu_util
    if not emu_util.emu_available():
        pytest.skip("no host clang for the emulation build")
    monkeypatch.setattr(L, "_lib", emu_util.emu_lib())
    monkeypatch.setattr(L, "on_device", lambda t: True)
    from segmamba_amd.segmamba import SegMamba
    from segmamba_amd.trainer import build_training_state, train_step
    torch.manual_seed(0)
    net = SegMamba(in_chans=4, out_chans=3, depths=[1, 1, 1, 1], feat_size=[48, 8, 16, 32], hidden_size=32)
    fn = DC_and_BCE_loss({}, dict(batch_dice=True, do_bg=True, smooth=1e-5, ddp=False), regions=BRATS_REGIONS)
    st = build_training_state(torch.device("cpu"), model=net, loss_fn=fn)
    assert st.loss_fn is fn
    g = torch.Generator().manual_seed(3)
    img, lab = torch.rand(1, 4, 32, 32, 32, generator=g), torch.randint(0, 4, (1, 32, 32, 32), generator=g)
    before = [p.detach().clone() for p in net.parameters()]
    with torch.no_grad():
        want = float(fn(net(img), lab))
    loss = float(train_step(st, img, lab))
    # the step computes with the parameter bank's bf16 copies of the weights, `want` with the fp32 weights: every weight is off by up
    # to 2^-9 relative, through some twenty layers; 3e-2 is the width tests/test_losses_cpu.py gives the same comparison of a step
    # with a no-grad forward for DC_and_CE_loss
    assert np.isfinite(loss) and abs(loss - want) <= 3e-2 * abs(want)
    assert any((a - b.detach()).abs().max() > 0 for a, b in zip(before, net.parameters()))


def test_dice_classes_still_refuse_an_emulated_device(monkeypatch):
    monkeypatch.setattr(L, "on_device", lambda t: True)
    x, y = torch.zeros(2, 3, 3, 5, 7), torch.zeros(2, 1, 3, 5, 7)
    for mod in (SoftDiceLoss(torch.sigmoid, ddp=False), MemoryEfficientSoftDiceLoss(torch.sigmoid, ddp=False),
                DC_and_BCE_loss({}, {"ddp": False}).dc):
        with pytest.raises(NotImplementedError):
            mod(x, y)
