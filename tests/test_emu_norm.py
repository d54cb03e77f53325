"""InstanceNorm3d (+ residual) (+ activation) of csrc/instnorm.hip with the kernel sources compiled for the CPU emulator, element by
element against the float64 restatement of tests/norm_ref.py under its derived bounds (half an ulp of the output type plus small
terms): every dtype, activation / residual combination, offset and streaming mode, padded instance strides, statistics summed by a
producer, the autograd chain and determinism.  The same checks run on the HIP library in tests/test_gpu_norm.py."""
import pytest
import torch

from tests import emu_util
from tests import norm_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


@pytest.fixture
def product(emu, monkeypatch):
    """segmamba_amd.fused_norm on the emulated library, host tensors taken as they are"""
    monkeypatch.setattr(L, "_lib", emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    return emu


# the modes of one (dtype, shape) run back to back: they share the references (norm_checks.case)
MATRIX = [(dtype, shape, mode) for dtype in K.DTYPES for shape in K.SHAPES for mode in (0, 1, 2)]


@pytest.mark.parametrize("dtype,shape,mode", MATRIX, ids=lambda v: K.name(v) if isinstance(v, torch.dtype) else str(v).replace(" ", ""))
def test_matrix_emulated(emu, monkeypatch, dtype, shape, mode):
    """(a) forward and isolated backward; mode 0 at r = 0.2, 3 and 30, the forced streaming modes 1 and 2 at r = 3"""
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_matrix(emu, "cpu", shape, dtype, K.OFFSETS if mode == 0 else (3.0,))


@pytest.mark.parametrize("mode", [0, 1])
def test_padded_instance_strides_emulated(emu, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_padded(emu, "cpu")


@pytest.mark.parametrize("nparts", [1, 7, 300, 4096])
def test_producer_summed_statistics_emulated(emu, nparts):
    K.check_producer_stats(emu, "cpu", nparts)


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: str(s).replace(" ", ""))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=K.name)
def test_chained_through_autograd_emulated(product, monkeypatch, shape, dtype):
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    K.check_chained(product, "cpu", shape, dtype)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_two_calls_same_bits_emulated(emu, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_determinism(emu, "cpu")
