"""`from models.team14_arfdn.ARFDN import ARFDN` (test_demo.py) -> the HIP-engine ARFDN."""
from ntire2022_esr_amd.arfdn import ARFDN

__all__ = ["ARFDN"]
