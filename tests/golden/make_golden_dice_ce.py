"""Generate tests/golden/dice_ce.npz by running the REFERENCE's own loss classes.

    python tests/golden/make_golden_dice_ce.py <path of the reference checkout>

`light_training/loss/` (dice.py, compound_losses.py, robust_ce_loss.py, helpers.py, ddp_allgather.py, tensor_utilities.py) needs torch
and numpy only.  The modules are imported from the checkout at generation time and `DC_and_CE_loss` is run, as it is, on a seeded
(2, 4, 5, 6, 7) fp32 case with the float (2, 1, 5, 6, 7) target the reference's data loader produces.  Recorded: the inputs, and per
configuration the loss value and d loss / d logits as float32.  Configurations (ddp=False throughout): SoftDiceLoss and
MemoryEfficientSoftDiceLoss x batch_dice x do_bg, with smooth 1e-5 or 1.0 (each class and each flag sees both); ignore_label=4 on a
target with two ignored slices; pure Dice (weight_ce=0); pure CE (weight_dice=0); SoftDiceLoss with a clip_tp that two of the four
classes fall under.  The fixture holds numbers and the configurations' settings only; no reference code goes into this repository.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE = (2, 4, 5, 6, 7)


def inputs():
    g = torch.Generator().manual_seed(20261018)
    logits = (2.0 * torch.randn(SHAPE, generator=g)).float()
    target = torch.randint(0, SHAPE[1], (SHAPE[0], 1) + SHAPE[2:], generator=g).float()
    target_ignore = target.clone()
    target_ignore[0, 0, 1] = 4.0
    target_ignore[1, 0, :, 3] = 4.0
    return logits, target, target_ignore


def configurations():
    cases = []
    for kind in ("soft", "mem"):
        for batch_dice in (False, True):
            for do_bg in (False, True):
                # both values of smooth under every class, every batch_dice and every do_bg; the full product would not fit 100 KB
                smooth = 1.0 if (batch_dice != do_bg) == (kind == "soft") else 1e-5
                cases.append(dict(kind=kind, batch_dice=batch_dice, do_bg=do_bg, smooth=smooth))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=False, smooth=1e-5, ignore_label=4))
    cases.append(dict(kind="soft", batch_dice=False, do_bg=True, smooth=1.0, ignore_label=4))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=False, smooth=1e-5, weight_ce=0))
    cases.append(dict(kind="soft", batch_dice=False, do_bg=True, smooth=1e-5, weight_ce=0))
    cases.append(dict(kind="mem", batch_dice=True, do_bg=False, smooth=1e-5, weight_dice=0))
    cases.append(dict(kind="soft", batch_dice=True, do_bg=True, smooth=1e-5, clip_tp=25.0))
    return [dict(dict(weight_ce=1, weight_dice=1, ignore_label=None, clip_tp=None), **c) for c in cases]


def main(reference: str):
    sys.path.insert(0, reference)
    from light_training.loss.compound_losses import DC_and_CE_loss
    from light_training.loss.dice import MemoryEfficientSoftDiceLoss, SoftDiceLoss
    logits, target, target_ignore = inputs()
    cases = configurations()
    losses, grads = [], []
    for c in cases:
        kw = dict(batch_dice=c["batch_dice"], do_bg=c["do_bg"], smooth=c["smooth"], ddp=False)
        if c["clip_tp"] is not None:
            kw["clip_tp"] = c["clip_tp"]
        fn = DC_and_CE_loss(kw, {}, weight_ce=c["weight_ce"], weight_dice=c["weight_dice"], ignore_label=c["ignore_label"],
                            dice_class=SoftDiceLoss if c["kind"] == "soft" else MemoryEfficientSoftDiceLoss)
        x = logits.clone().requires_grad_(True)
        loss = fn(x, target_ignore if c["ignore_label"] is not None else target)
        loss.backward()
        losses.append(float(loss.detach()))
        grads.append(x.grad.numpy().astype(np.float32))
    dst = os.path.join(HERE, "dice_ce.npz")
    np.savez_compressed(dst, logits=logits.numpy(), target=target.numpy(), target_ignore=target_ignore.numpy(),
                        cases=np.array(json.dumps(cases)), loss=np.array(losses, dtype=np.float32), grad=np.stack(grads),
                        torch_version=np.array(torch.__version__))
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(cases), "configurations")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
