"""`models.team25_frfdn` (test_demo.py: id 25) -> the HIP-engine FasterRFDN (see FRFDN.py)."""
