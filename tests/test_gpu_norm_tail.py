"""The residual tail of csrc/instnorm.hip on the HIP library: the checks of tests/test_emu_norm_tail.py on the GPU - every output
bit-equal to the two-call sequence on the same library."""
import pytest
import torch

from tests import norm_checks as K
from tests import norm_tail_checks as T
from segmamba_amd import lib as L

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def hip():
    return L.get_lib()


MATRIX = [(dtype, shape, mode) for dtype in K.DTYPES for shape in K.SHAPES for mode in (0, 1, 2)]


@pytest.mark.parametrize("dtype,shape,mode", MATRIX, ids=lambda v: K.name(v) if isinstance(v, torch.dtype) else str(v).replace(" ", ""))
def test_tail_equals_two_calls(hip, monkeypatch, dtype, shape, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_shape(hip, DEV, shape, dtype)


@pytest.mark.parametrize("dtype", K.DTYPES, ids=K.name)
def test_tail_offsets(hip, monkeypatch, dtype):
    """r = mean / std of 0.2 and 30 (norm_checks.OFFSETS): the statistics at their best and at their worst conditioning"""
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    T.check_shape(hip, DEV, K.SHAPES[2], dtype, (K.OFFSETS[0], K.OFFSETS[2]))


@pytest.mark.parametrize("mode", [0, 1])
def test_tail_padded_instance_strides(hip, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_padded(hip, DEV)


@pytest.mark.parametrize("nparts", [7, 300])
def test_tail_producer_summed_statistics(hip, nparts):
    T.check_producer_stats(hip, DEV, nparts)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_tail_two_calls_same_bits(hip, monkeypatch, mode):
    monkeypatch.setenv("SEGM_NORM_NT", str(mode))
    T.check_determinism(hip, DEV)


@pytest.mark.parametrize("channels,shapes", T.BLOCKS, ids=lambda v: str(v).replace(" ", ""))
def test_res_block_same_bits_with_and_without_the_tail(hip, monkeypatch, channels, shapes):
    monkeypatch.delenv("SEGM_NORM_NT", raising=False)
    T.check_block(DEV, monkeypatch, channels, shapes)
