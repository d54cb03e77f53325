"""The Mamba inner pipeline's two autograd nodes (segmamba_amd/selective_scan_interface.py) on the HIP library: the checks of
tests/test_emu_mamba_inner.py on the GPU, the node comparison at the regular shape (the one-grid scan launches) only."""
import pytest

from tests import mamba_inner_checks as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dtype,rows,add3", K.CASES, ids=K.case_id)
def test_three_nodes_and_one_node_agree_per_direction(monkeypatch, dtype, rows, add3):
    K.check_nodes_agree(monkeypatch, DEV, "regular", dtype, rows, add3)


def test_projection_biases_against_the_oracle():
    """tolerances of tests/test_gpu_model.py::test_mamba_inner_fn_no_out_proj_golden: the same function on the same fixture"""
    K.check_projection_biases(DEV, (1e-3, 1e-3), 2e-3)
