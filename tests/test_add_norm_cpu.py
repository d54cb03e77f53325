"""The fused add + norm without a GPU: the drop-in names resolve to the segmamba_amd objects, the float64 restatement
(tests/add_norm_ref.py) meets the recorded reference results at 1e-12 relative - which ties it to the reference and not to the code
under test - and layer_norm_fn / rms_norm_fn / Block on CPU tensors (the ATen composition) meet the same fixture."""
import numpy as np
import torch

from tests import add_norm_checks as K
from tests import add_norm_ref as R


def test_dropin_names_resolve_to_the_library():
    from mamba_ssm.ops.triton.layernorm import RMSNorm, layer_norm_fn, rms_norm_fn
    from mamba_ssm.modules.mamba_simple import Block, Mamba
    import segmamba_amd.add_norm as AN
    import segmamba_amd.mamba_simple as MS
    assert RMSNorm is AN.RMSNorm and layer_norm_fn is AN.layer_norm_fn and rms_norm_fn is AN.rms_norm_fn
    assert Block is MS.Block and Mamba is MS.Mamba


def test_restatement_meets_the_recorded_reference():
    """forward and backward of tests/add_norm_ref.py against layer_norm_ref / rms_norm_ref and torch.autograd.grad in float64"""
    g = K.golden()
    eps = float(g["eps"])
    worst = 0.0
    for i, norm, has_res, prenorm, has_b, key in K.fixture_cases():
        t = lambda n: torch.from_numpy(g[f"s{i}.{n}"])      # noqa: E731
        rms = norm == "rms"
        y, s, mean, rstd = R.forward(t("x"), t("w"), t("b") if has_b else None, t("residual") if has_res else None, eps, rms,
                                     sum_dtype=torch.float64)
        dx, dw, db = R.backward(t("dy"), s, t("w"), mean, rstd, t("dres") if prenorm else None, rms)
        pairs = [(y, "y"), (dx, "dx"), (dw, "dw")] + ([(s, "res_out")] if prenorm else []) + ([(db, "db")] if has_b else []) \
            + ([(dx, "dres_in")] if has_res else [])
        for got, name in pairs:
            want = g[key + name]
            err = float(np.abs(got.numpy() - want).max()) / max(1.0, float(np.abs(want).max()))
            worst = max(worst, err)
            assert err <= 1e-12, (key + name, err)
    print(f"add_norm_ref against the fixture: worst relative error {worst:.3e}")


def test_functions_on_cpu_meet_the_recorded_reference():
    K.check_functions_recorded("cpu", torch.float64, tol=1e-12, tol_w=1e-12)
    K.check_functions_recorded("cpu", torch.float32)


def test_block_on_cpu_meets_the_recorded_reference():
    """float64 blocks differ from the reference's by the order of the float64 operations inside the norm: a few 1e-16, amplified by
    rstd and the two mixers; 1e-11 of the largest value leaves four digits of margin.  With residual_in_fp32 the fused backward
    recomputes xhat from the fp32 stream it saved, as the reference's kernel does, where the recorded non-fused block keeps the
    float64 sum: an fp32 roundoff apart, the fp32 bound."""
    K.check_block_recorded("cpu", torch.float64, tol=1e-11, tol_w=1e-11, flags=(0,))
    K.check_block_recorded("cpu", torch.float64, tol=K.TOL[torch.float32], flags=(1,))
    K.check_block_recorded("cpu", torch.float32)
