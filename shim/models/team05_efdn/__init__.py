"""`models.team05_efdn` (test_demo.py:61) -> the HIP-engine EFDN."""
