"""Generate tests/golden/region_bce.npz by running the REFERENCE's own region-based loss.

    python tests/golden/make_golden_region_bce.py <path of the reference checkout>

`light_training/loss/` (dice.py, compound_losses.py, and what they import) needs torch and numpy only.  The modules are imported from
the checkout at generation time and `DC_and_BCE_loss` is run, as it is, on a seeded (2, 3, 5, 6, 7) fp32 case whose target holds the
BraTS regions (TC = {1, 3}, WT = {1, 2, 3}, ET = {3}) of a seeded label map as float planes.  Recorded: the inputs, and per
configuration the loss value and d loss / d logits as float32.  Configurations (ddp=False throughout): SoftDiceLoss and
MemoryEfficientSoftDiceLoss x batch_dice x do_bg, with smooth 1e-5 or 1.0 spread as in make_golden_dice_ce.py (each class and each
flag sees both); use_ignore_label under both classes, on a (2, 4, 5, 6, 7) target whose last plane ignores one slice of sample 0 and
one column of sample 1; pure Dice (weight_ce=0); pure BCE (weight_dice=0); one soft target (uniform planes in [0, 1]).  The fixture
holds numbers and the configurations' settings only; no reference code goes into this repository.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 3, 5, 6, 7)
REGIONS = ((1, 3), (1, 2, 3), (3,))


def inputs():
    g = torch.Generator().manual_seed(20261019)
    logits = (2.0 * torch.randn(SHAPE, generator=g)).float()
    labels = torch.randint(0, 4, (SHAPE[0],) + SHAPE[2:], generator=g)
    target = torch.stack([sum((labels == l) for l in reg) > 0 for reg in REGIONS], 1).float()
    ignore = torch.zeros((SHAPE[0], 1) + SHAPE[2:])
    ignore[0, 0, 1] = 1.0
    ignore[1, 0, :, 3] = 1.0
    target_ignore = torch.cat([target, ignore], 1)
    target_soft = torch.rand(SHAPE, generator=g).float()
    return logits, labels, target, target_ignore, target_soft


def configurations():
    cases = []
    for kind in ("soft", "mem"):
        for batch_dice in (False, True):
            for do_bg in (False, True):
                smooth = 1.0 if (batch_dice != do_bg) == (kind == "soft") else 1e-5
                cases.append(dict(kind=kind, batch_dice=batch_dice, do_bg=do_bg, smooth=smooth))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=True, smooth=1e-5, use_ignore_label=True))
    cases.append(dict(kind="soft", batch_dice=False, do_bg=False, smooth=1.0, use_ignore_label=True))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=True, smooth=1e-5, weight_ce=0))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=True, smooth=1e-5, weight_dice=0))
    cases.append(dict(kind="mem", batch_dice=False, do_bg=True, smooth=1e-5, soft_target=True))
    return [dict(dict(weight_ce=1, weight_dice=1, use_ignore_label=False, soft_target=False), **c) for c in cases]


def main(reference: str):
    sys.path.insert(0, reference)
    from light_training.loss.compound_losses import DC_and_BCE_loss
    from light_training.loss.dice import MemoryEfficientSoftDiceLoss, SoftDiceLoss
    logits, labels, target, target_ignore, target_soft = inputs()
    cases = configurations()
    losses, grads = [], []
    for c in cases:
        kw = dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"], ddp=False)
        fn = DC_and_BCE_loss({}, kw, weight_ce=c["weight_ce"], weight_dice=c["weight_dice"], use_ignore_label=c["use_ignore_label"],
                             dice_class=SoftDiceLoss if c["kind"] == "soft" else MemoryEfficientSoftDiceLoss)
        x = logits.clone().requires_grad_(True)
        tgt = target_ignore if c["use_ignore_label"] else target_soft if c["soft_target"] else target
        loss = fn(x, tgt.clone())
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(x.grad.numpy().astype(np.float32))
    dst = os.path.join(HERE, "region_bce.npz")
    np.savez_compressed(dst, logits=logits.numpy(), labels=labels.numpy().astype(np.int64), target=target.numpy().astype(np.uint8),
                        ignore=target_ignore[:, -1].numpy().astype(np.uint8), target_soft=target_soft.numpy(),
                        regions=np.array(json.dumps(REGIONS)), cases=np.array(json.dumps(cases)),
                        loss=np.array(losses, dtype=np.float32), grad=np.stack(grads), torch_version=np.array(torch.__version__))
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(cases), "configurations")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
