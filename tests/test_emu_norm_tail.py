"""The residual tail of csrc/instnorm.hip (y = act(IN(out2) + IN(skip)) in one apply pass per direction) with the kernel sources
compiled for the CPU emulator: bit-equal to the two-call sequence on the same library for every dtype, shape class, streaming mode
and activation, with padded instance strides and producer-summed statistics, deterministic, and bit-equal through a whole residual
block with the route on and off.  The same checks run on the HIP library in tests/test_gpu_norm_tail.py."""
import pytest
import torch

from tests import emu_util
from tests import norm_checks as K
from tests import norm_tail_checks as T
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture(scope="module")
def emu():
    return emu_util.emu_lib()


MATRIX = [(dtype, shape, mode) for dtype in K.DTYPES for shape in K.SHAPES for mode in (0, 1, 2)]


@pytest.mark.parametrize("dtype,shape,mode", MATRIX, ids=lambda v: K.name(v) if isinstance(v, torch.dtype) else str(v).replace(" ", ""))
def test_tail_equals_two_calls_emulated(emu, monkeypatch, dtype, shape, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_shape(emu, "cpu", shape, dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.name)
def test_tail_offsets_emulated(emu, monkeypatch, dtype):
    """r = mean / std of 0.2 and 30 (norm_checks.OFFSETS): the statistics at their best and at their worst conditioning"""
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    T.check_shape(emu, "cpu", K.SHAPES[2], dtype, (K.OFFSETS[0], K.OFFSETS[2]))


@pytest.mark.parametrize("mode", [0, 1])
def test_tail_padded_instance_strides_emulated(emu, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_padded(emu, "cpu")


@pytest.mark.parametrize("nparts", [7, 300])
def test_tail_producer_summed_statistics_emulated(emu, nparts):
    T.check_producer_stats(emu, "cpu", nparts)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tail_two_calls_same_bits_emulated(emu, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_determinism(emu, "cpu")


@pytest.mark.parametrize("channels,shapes", T.BLOCKS, ids=lambda v: str(v).replace(" ", ""))
def test_res_block_same_bits_with_and_without_the_tail_emulated(emu, monkeypatch, channels, shapes):
    from segmamba_amd import conv3d as C3
    monkeypatch.setattr(L, "get_lib", lambda: emu)
    monkeypatch.setattr(L, "on_device", lambda t: True)
    monkeypatch.setattr(C3, "_route", lambda kind, width, variants: variants[-1])     # the library's candidates, as in test_emu_kernels.py
    T.check_block("cpu", monkeypatch, channels, shapes)


def test_tail_on_cpu_tensors_is_the_aten_expression():
    T.check_cpu_fallback()
