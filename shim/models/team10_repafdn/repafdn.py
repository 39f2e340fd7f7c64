"""`from models.team10_repafdn.repafdn import RePAFDN` (test_demo.py) -> the HIP-engine RePAFDN."""
from ntire2022_esr_amd.repafdn import RePAFDN

__all__ = ["RePAFDN"]
