"""`from models.team37_bmdn import BMDN` (test_demo.py) -> the HIP-engine BMDN."""
from ntire2022_esr_amd.bmdn import BMDN  # noqa: F401

__all__ = ["BMDN"]
