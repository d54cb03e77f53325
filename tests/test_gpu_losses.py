"""segmamba_amd/losses.py on the GPU: `RobustCrossEntropyLoss` - the one class with a kernel, train_ops.cross_entropy - against the float64
restatement (tests/loss_ref.py) with the reference's float (B, 1, ...) target, and the refusal of device tensors by the classes that
have none (no fall-back to ATen on the device)."""
import numpy as np
import pytest
import torch

from segmamba_amd import losses as LS
from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _case():
    rng = np.random.default_rng(31)
    x = (2 * rng.standard_normal((2, 4, 5, 6, 7))).astype(np.float32)
    y = rng.integers(0, 4, (2, 5, 6, 7))
    y.reshape(-1)[::7] = 4                                   # every 7th voxel ignored
    return x, y


def test_robust_cross_entropy_on_the_device():
    """bounds of tests/test_gpu_kernels.py for segm_cross_entropy: loss 1e-5 relative, gradient within 1e-6 x max |gradient|"""
    x, y = _case()
    v, gr = R.value_and_grad(R.cross_entropy, x, y, 4)
    mod = LS.RobustCrossEntropyLoss(ignore_index=4)
    for tgt in (torch.as_tensor(y.astype(np.float32))[:, None], torch.as_tensor(y)):
        xt = torch.as_tensor(x, device=DEV).requires_grad_(True)
        loss = mod(xt, tgt.to(DEV))
        loss.backward()
        assert abs(float(loss.detach()) - v) <= 1e-5 * abs(v)
        assert np.abs(xt.grad.double().cpu().numpy() - gr).max() <= 1e-6 * np.abs(gr).max()


def test_dice_classes_refuse_device_tensors():
    x, y = _case()
    xt, tgt = torch.as_tensor(x, device=DEV), torch.as_tensor(y.astype(np.float32), device=DEV)[:, None]
    for mod in (LS.SoftDiceLoss(LS.softmax_helper_dim1, ddp=False), LS.MemoryEfficientSoftDiceLoss(LS.softmax_helper_dim1, ddp=False),
                LS.DC_and_CE_loss({"ddp": False}, {})):
        with pytest.raises(NotImplementedError):
            mod(xt, tgt)
