"""TopKLoss, DC_and_topk_loss and the reductions of train_ops.cross_entropy on CPU tensors (the ATen path, as the reference writes it)
against the float64 restatement tests/topk_ref.py and the recording tests/golden/topk_ce.npz of the reference's own classes.
Bounds, those of tests/test_losses_cpu.py: 1e-6 relative on the loss, 1e-6 x max |gradient|."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from segmamba_amd import losses, train_ops
from tests import loss_ref
from tests import topk_checks as K
from tests import topk_ref as R

CASES = list(range(len(R.CASES)))


def run(fn, logits, target):
    x = torch.from_numpy(logits).clone().requires_grad_(True)
    loss = fn(x, target)
    loss.backward()
    return float(loss.detach()), x.grad.double().numpy()


def close(loss, grad, w_loss, w_grad, what):
    assert abs(loss - w_loss) <= 1e-6 * abs(w_loss), (what, loss, w_loss)
    assert np.abs(grad - w_grad).max() <= 1e-6 * np.abs(w_grad).max(), (what, np.abs(grad - w_grad).max())


@pytest.mark.parametrize("i", CASES)
def test_restatement_matches_the_recording(i):
    shape, C, k, ignore = R.CASES[i]
    logits, labels = R.case_inputs(i)
    g = K.golden()
    assert R.boundary_gap(logits, labels, k, ignore) >= 1e-4
    loss, grad = R.topk_loss(logits, labels, k, ignore)
    close(loss, grad, float(g[f"loss_{i}"]), g[f"grad_{i}"].astype(np.float64), i)


@pytest.mark.parametrize("i", CASES)
def test_topk_loss_target_shapes_and_dtypes(i):
    """(B, 1, ...) and (B, ...) targets, float and integer, against the restatement"""
    shape, C, k, ignore = R.CASES[i]
    logits, labels = R.case_inputs(i)
    w_loss, w_grad = R.topk_loss(logits, labels, k, ignore)
    fn = losses.TopKLoss(k=k, ignore_index=K.ign_of(ignore))
    y = torch.from_numpy(labels)
    for target in (y.float().unsqueeze(1), y.unsqueeze(1), y, y.float(), y.to(torch.int16).unsqueeze(1)):
        close(*run(fn, logits, target), w_loss, w_grad, (i, target.dtype, tuple(target.shape)))


@pytest.mark.parametrize("i", CASES)
def test_dc_and_topk_without_dice_is_topk(i):
    shape, C, k, ignore = R.CASES[i]
    logits, labels = R.case_inputs(i)
    g = K.golden()
    fn = losses.DC_and_topk_loss({}, dict(k=k), weight_ce=1, weight_dice=0, ignore_label=ignore)
    close(*run(fn, logits, torch.from_numpy(labels).float().unsqueeze(1)), float(g[f"loss_{i}"]), g[f"grad_{i}"].astype(np.float64), i)


@pytest.mark.parametrize("i", R.DICE_CASES)
def test_dc_and_topk_matches_the_recording(i):
    shape, C, k, ignore = R.CASES[i]
    logits, labels = R.case_inputs(i)
    g = K.golden()
    target = torch.from_numpy(labels).float().unsqueeze(1)
    fn = losses.DC_and_topk_loss(dict(R.DICE_KWARGS), dict(k=k), weight_ce=1, weight_dice=1, ignore_label=ignore)
    close(*run(fn, logits, target), float(g[f"dc_loss_{i}"]), g[f"dc_grad_{i}"].astype(np.float64), i)
    # and against the restatements: the top-k term plus tests/loss_ref.py's Dice with the ignored voxels masked out
    kw = dict(kind="soft", batch_dice=True, do_bg=False, smooth=1e-5)
    mask = None if ignore is None else labels != ignore
    yd = labels if ignore is None else np.where(labels == ignore, 0, labels)
    d_loss, d_grad = loss_ref.value_and_grad(lambda x: loss_ref.dice(x, yd, mask=mask, **kw), logits)
    t_loss, t_grad = R.topk_loss(logits, labels, k, ignore)
    close(*run(fn, logits, target), t_loss + d_loss, t_grad + d_grad, i)
    # the weights
    fn2 = losses.DC_and_topk_loss(dict(R.DICE_KWARGS), dict(k=k), weight_ce=0.5, weight_dice=2, ignore_label=ignore)
    close(*run(fn2, logits, target), 0.5 * t_loss + 2 * d_loss, 0.5 * t_grad + 2 * d_grad, i)
    fn3 = losses.DC_and_topk_loss(dict(R.DICE_KWARGS), dict(k=k), weight_ce=0, weight_dice=1, ignore_label=ignore)
    close(*run(fn3, logits, target), d_loss, d_grad, i)


def test_refusals():
    with pytest.raises(NotImplementedError, match="TopKLoss: class weights are not supported"):
        losses.TopKLoss(weight=torch.ones(4))
    with pytest.raises(NotImplementedError, match="TopKLoss: label_smoothing is not supported"):
        losses.TopKLoss(label_smoothing=0.1)
    with pytest.raises(NotImplementedError, match="class weights"):
        losses.DC_and_topk_loss({}, dict(weight=torch.ones(4)))
    logits, labels = R.case_inputs(0)
    x, y = torch.from_numpy(logits), torch.from_numpy(labels)
    with pytest.raises(ValueError, match="target must be"):
        losses.TopKLoss()(x, y.unsqueeze(1).expand(-1, 2, -1, -1, -1))
    with pytest.raises(NotImplementedError, match="ignore_label needs a label map"):
        losses.DC_and_topk_loss({}, {}, ignore_label=4)(x, y)
    with pytest.raises(ValueError, match="reduction"):
        train_ops.cross_entropy(x, y, reduction="max")
    with pytest.raises(ValueError, match="reduction"):
        train_ops.CrossEntropyLoss(reduction="max")
    assert losses.TopKLoss(ignore_index=7, k=25).k == 25 and losses.DC_and_topk_loss({}, {}, ignore_label=4).ce.ignore_index == 4


def test_k_that_selects_no_voxel_raises():
    """kk = int(420 * 0.2 / 100) = 0: ValueError (the reference returns the NaN of an empty mean)"""
    logits, labels = R.case_inputs(0)
    with pytest.raises(ValueError, match="selects none"):
        losses.TopKLoss(k=0.2)(torch.from_numpy(logits), torch.from_numpy(labels))
    with pytest.raises(ValueError, match="selects more"):
        losses.TopKLoss(k=101)(torch.from_numpy(logits), torch.from_numpy(labels))


def test_all_ignored_batch_gives_zero():
    logits, labels = R.case_inputs(0)
    target = torch.full((2, 1, 5, 6, 7), 4.0)
    for fn in (losses.TopKLoss(ignore_index=4), losses.DC_and_topk_loss({}, {}, weight_dice=0, ignore_label=4)):
        loss, grad = run(fn, logits, target)
        assert loss == 0.0 and not grad.any()


@pytest.mark.parametrize("i", [0, 1])
def test_cross_entropy_reductions_cpu(i):
    shape, C, k, ignore = R.CASES[i]
    logits, labels = R.case_inputs(i)
    x, y = torch.from_numpy(logits), torch.from_numpy(labels)
    ign = K.ign_of(ignore)
    for red in ("none", "sum", "mean"):
        want = F.cross_entropy(x, y, ignore_index=ign, reduction=red)
        assert torch.equal(train_ops.cross_entropy(x, y, ign, reduction=red), want)
        assert torch.equal(train_ops.CrossEntropyLoss(ign, red)(x, y), want)
    assert torch.equal(train_ops.cross_entropy(x, y, ign), F.cross_entropy(x, y, ignore_index=ign))
    m = train_ops.cross_entropy(x, y, ign, reduction="none").double().numpy()
    assert np.abs(m - R.loss_map(logits, labels, ignore)).max() <= 2e-6 * (1 + m.max())
