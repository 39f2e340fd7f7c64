"""`from models.team25_frfdn.FRFDN import FasterRFDN` (test_demo.py) -> the HIP-engine FasterRFDN."""
from ntire2022_esr_amd.frfdn import FasterRFDN  # noqa: F401

__all__ = ["FasterRFDN"]
