"""`from models.team05_efdn.plainsr import PLAINRFDN` (test_demo.py:61) -> the HIP-engine EFDN."""
from ntire2022_esr_amd.efdn import PLAINRFDN  # noqa: F401

__all__ = ["PLAINRFDN"]
