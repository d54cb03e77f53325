"""Drop-in path of the reference's `mamba_ssm.ops.triton.layernorm` (Triton kernels there; the MI355X library's fused
add + LayerNorm / RMSNorm kernels here).  `layer_norm_linear_fn` and the `*_ref` functions are not provided."""
from segmamba_amd.add_norm import LayerNormFn, RMSNorm, layer_norm_fn, rms_norm_fn  # noqa: F401
