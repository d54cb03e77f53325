"""The drop-in sentence of BASELINE.json for the TRAINING script: "keeping the mamba_ssm.Mamba / causal_conv1d and
model_segmamba.segmamba.SegMamba module API so it drops into 3_train.py ... unchanged".

What the reference's `3_train.py` asks of this repository, restated: `BraTSTrainer.__init__` builds
`from model_segmamba.segmamba import SegMamba` with `SegMamba(in_chans=4, out_chans=4, depths=[2,2,2,2], feat_size=[48, 96, 192, 384])`,
`nn.CrossEntropyLoss` and `torch.optim.SGD(lr=1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)`; its `get_input` takes
`batch["data"]` and `batch["seg"][:, 0].long()`; ONE iteration of the reference's own loop (`light_training/trainer.py:422-480` on a
CPU device: every `param.grad = None`, the script's `training_step`, backward, `clip_grad_norm_(12)`, `SGD.step()`, the logged lr)
then runs on a synthetic BraTS-shaped batch.  No GPU here: the kernels are the library's sources on the CPU emulation (tests/emu),
the way every other host-side test runs them.
"""
import os

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_script_step_runs_on_the_dropin_packages(monkeypatch):
    from tests.emu_util import emu_available, emu_lib
    if not emu_available():
        pytest.skip("no host compiler for the CPU emulation of the kernels")
    from segmamba_amd import lib as L
    monkeypatch.setattr(L, "_lib", emu_lib())
    from model_segmamba.segmamba import SegMamba                  # the import inside BraTSTrainer.__init__
    import model_segmamba.segmamba as dropin
    assert dropin.__file__.startswith(ROOT)
    torch.manual_seed(0)
    model = SegMamba(in_chans=4, out_chans=4, depths=[2, 2, 2, 2], feat_size=[48, 96, 192, 384])
    cross = nn.CrossEntropyLoss()
    optimizer = torch.optim.SGD(model.parameters(), lr=1e-2, weight_decay=3e-5, momentum=0.99, nesterov=True)
    assert type(model) is dropin.SegMamba and len(model.state_dict()) == 291
    with open(os.path.join(ROOT, "tests", "golden", "segmamba_state_dict_keys.txt")) as f:
        assert list(model.state_dict()) == [line.split()[0] for line in f if line.strip()]
    assert isinstance(optimizer, torch.optim.SGD) and optimizer.defaults["nesterov"]

    def get_input(batch):
        return batch["data"], batch["seg"][:, 0].long()

    g = torch.Generator().manual_seed(0)
    batch = {"data": torch.rand(1, 4, 32, 32, 32, generator=g), "seg": torch.randint(0, 4, (1, 1, 32, 32, 32), generator=g).float()}
    w0 = [p.detach().clone() for p in model.parameters()]
    with torch.no_grad():
        image, label = get_input({k: v.clone() for k, v in batch.items()})
        expect = float(cross(model(image), label))
    # the loop body for one step
    logged = {}
    model.train()
    for p in model.parameters():
        p.grad = None
    image, label = get_input(batch)
    loss = cross(model(image), label)
    logged["training_loss"] = loss.item()
    loss.backward()
    torch.nn.utils.clip_grad_norm_(model.parameters(), 12)
    optimizer.step()
    logged["lr"] = optimizer.state_dict()["param_groups"][0]["lr"]
    assert abs(logged["training_loss"] - expect) <= 1e-5 * abs(expect) and logged["lr"] == pytest.approx(1e-2)
    moved = [float((p.detach() - w).abs().max()) for p, w in zip(model.parameters(), w0)]
    assert all(m > 0 for m in moved), "every parameter takes part in the step"
    assert all(torch.isfinite(p).all() for p in model.parameters())
