"""The Mamba inner pipeline's two autograd nodes (segmamba_amd/selective_scan_interface.py) with the kernel sources compiled for
the CPU emulator: the checks of tests/mamba_inner_checks.py.  The same checks run on the HIP library in
tests/test_gpu_mamba_inner.py."""
import pytest

from tests import emu_util
from tests import mamba_inner_checks as K
from segmamba_amd import lib as L

pytestmark = pytest.mark.skipif(not emu_util.emu_available(), reason="ROCm host clang not present")


@pytest.fixture
def product(monkeypatch):
    """the host code on the emulated library"""
    monkeypatch.setattr(L, "_lib", emu_util.emu_lib())


@pytest.mark.parametrize("dtype,rows,add3", K.CASES, ids=K.case_id)
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_three_nodes_and_one_node_agree_per_direction_emulated(product, monkeypatch, shape, dtype, rows, add3):
    K.check_nodes_agree(monkeypatch, "cpu", shape, dtype, rows, add3)


def test_projection_biases_against_the_oracle_emulated(product):
    """tolerances of test_reference_layout_inner_fn_on_emulated_kernels (tests/test_emu_kernels.py)"""
    K.check_projection_biases("cpu", (1e-3, 1e-4), 1e-3)
