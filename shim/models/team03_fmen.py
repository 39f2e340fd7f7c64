"""`from models.team03_fmen import FMEN` (test_demo.py:47) -> the HIP-engine FMEN."""
from ntire2022_esr_amd.fmen import FMEN  # noqa: F401

__all__ = ["FMEN"]
