"""`models.team14_arfdn` (test_demo.py: id 14) -> the HIP-engine ARFDN (see ARFDN.py)."""
