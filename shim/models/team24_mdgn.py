"""`from models.team24_mdgn import MDGN` (test_demo.py) -> the HIP-engine MDGN."""
from ntire2022_esr_amd.mdgn import MDGN  # noqa: F401

__all__ = ["MDGN"]
