"""InstanceNorm3d (+ residual) (+ activation) of csrc/instnorm.hip on the HIP library: the checks of tests/test_emu_norm.py on the GPU
(every output element against the float64 restatement of tests/norm_ref.py under its derived bounds), and the smallest tensors at
which the library itself picks the streaming modes 1 and 2, with the padded channel stride of the 128^3 volumes."""
import pytest
import torch

from tests import norm_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


# the modes of one (dtype, shape) run back to back: they share the references (norm_checks.case)
MATRIX = [(dtype, shape, mode) for dtype in K.DTYPES for shape in K.SHAPES for mode in (0, 1, 2)]


@pytest.mark.parametrize("dtype,shape,mode", MATRIX, ids=lambda v: K.name(v) if isinstance(v, torch.dtype) else str(v).replace(" ", ""))
def test_matrix(hip, monkeypatch, dtype, shape, mode):
    """(a) forward and isolated backward; mode 0 at r = 0.2, 3 and 30, the forced streaming modes 1 and 2 at r = 3"""
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_matrix(hip, DEV, shape, dtype, K.OFFSETS if mode == 0 else (3.0,))


@pytest.mark.parametrize("mode", [0, 1])
def test_padded_instance_strides(hip, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_padded(hip, DEV)


@pytest.mark.parametrize("nparts", [1, 7, 300, 4096])
def test_producer_summed_statistics(hip, nparts):
    K.check_producer_stats(hip, DEV, nparts)


@pytest.mark.parametrize("shape", K.SHAPES, ids=lambda s: str(s).replace(" ", ""))
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=K.name)
def test_chained_through_autograd(hip, monkeypatch, shape, dtype):
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    K.check_chained(hip, DEV, shape, dtype)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_two_calls_same_bits(hip, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    K.check_determinism(hip, DEV)


@pytest.mark.parametrize("channels", [16, 48])
def test_at_the_sizes_that_stream(hip, monkeypatch, channels):
    """1 x 16 x 128^3 bf16 (67 MB: mode 1) and 1 x 48 x 128^3 (201 MB: mode 2), nothing forced, every volume with the padded channel
    stride of ops_raw.volume_empty: LeakyReLU + residual + dresidual, forward and isolated backward under the per-element bounds"""
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    K.check_at_size(hip, DEV, channels)
    torch.cuda.empty_cache()
