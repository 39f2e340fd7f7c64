"""`models.team35_rfdn` (test_demo.py: id 35) -> the HIP-engine DWRFDN (see rfdn.py)."""
