"""`models.team10_repafdn` (test_demo.py: id 10) -> the HIP-engine RePAFDN (see repafdn.py)."""
