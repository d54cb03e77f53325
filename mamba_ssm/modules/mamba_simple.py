"""Drop-in for reference mamba/mamba_ssm/modules/mamba_simple.py (classes `Mamba` and `Block`)."""
from segmamba_amd.mamba_simple import Block, Mamba  # noqa: F401
