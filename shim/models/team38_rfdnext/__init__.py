"""`models.team38_rfdnext` (test_demo.py: id 38) -> the HIP-engine RFDNeXt (see RFDN.py)."""
