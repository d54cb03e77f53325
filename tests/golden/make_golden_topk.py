"""Generate tests/golden/topk_ce.npz by running the REFERENCE's own TopKLoss and DC_and_topk_loss on CPU.

    python tests/golden/make_golden_topk.py <path of the reference checkout>

`light_training/loss/` (robust_ce_loss.py, compound_losses.py, dice.py, helpers.py, ddp_allgather.py, tensor_utilities.py) needs torch
and numpy only.  The modules are imported from the checkout at generation time and run, as they are, on the cases of
tests/topk_ref.py (`CASES`: shape, classes, k, ignored label; inputs from numpy's frozen legacy generator, seed 31, logits 2 N(0, 1)
in fp32, every 7th voxel ignored where a case ignores) with the float (B, 1, ...) target the reference's data loader produces.
Recorded: per case the TopKLoss value and d loss / d logits as float32, for `DICE_CASES` the same of DC_and_topk_loss with
`DICE_KWARGS`, and the float64 sum of every case's logits (a guard on the regenerated inputs).  Before recording, the script asserts
that the float64 losses on either side of every case's kk boundary differ by at least 1e-4, so that fp32 selects the same voxels and
gradients can be compared at every voxel.  The fixture holds numbers only; no reference code goes into this repository.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import topk_ref as R  # noqa: E402


def main(reference: str):
    sys.path.insert(0, reference)
    from light_training.loss.compound_losses import DC_and_topk_loss
    from light_training.loss.robust_ce_loss import TopKLoss
    out = {}
    gaps = []
    for i, (shape, C, k, ignore) in enumerate(R.CASES):
        logits, labels = R.case_inputs(i)
        gap = R.boundary_gap(logits, labels, k, ignore)
        assert gap >= 1e-4, (i, gap)
        gaps.append(gap)
        target = torch.from_numpy(labels).float().unsqueeze(1)
        kw = {} if ignore is None else dict(ignore_index=ignore)
        x = torch.from_numpy(logits).clone().requires_grad_(True)
        loss = TopKLoss(k=k, **kw)(x, target)
        loss.backward()
        out[f"loss_{i}"] = np.float32(loss.detach())
        out[f"grad_{i}"] = x.grad.numpy().astype(np.float32)
        out[f"logits_sum_{i}"] = np.float64(logits.astype(np.float64).sum())
        if i in R.DICE_CASES:
            x = torch.from_numpy(logits).clone().requires_grad_(True)
            loss = DC_and_topk_loss(dict(R.DICE_KWARGS), dict(k=k), weight_ce=1, weight_dice=1, ignore_label=ignore)(x, target)
            loss.backward()
            out[f"dc_loss_{i}"] = np.float32(loss.detach())
            out[f"dc_grad_{i}"] = x.grad.numpy().astype(np.float32)
    dst = os.path.join(HERE, "topk_ce.npz")
    np.savez_compressed(dst, torch_version=np.array(torch.__version__), **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; smallest boundary gap", min(gaps))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
