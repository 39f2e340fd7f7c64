"""`from models.team35_rfdn.rfdn import RFDN` (test_demo.py) -> the HIP-engine DWRFDN."""
from ntire2022_esr_amd.dwrfdn import DWRFDN

RFDN = DWRFDN

__all__ = ["RFDN"]
