"""`from models.team43_resdn import ResDN` (test_demo.py) -> the HIP-engine ResDN."""
from ntire2022_esr_amd.resdn import ResDN  # noqa: F401

__all__ = ["ResDN"]
