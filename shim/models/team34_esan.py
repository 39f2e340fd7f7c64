"""`from models.team34_esan import make_model` / `ESAN` (test_demo.py: id 34, make_model(1)) -> the HIP-engine ESAN."""
from ntire2022_esr_amd.esan import ESAN  # noqa: F401


def make_model(level):
    return ESAN(level=level)


__all__ = ["ESAN", "make_model"]
