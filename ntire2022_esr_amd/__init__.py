"""MI355X-native engine for the NTIRE2022_ESR test_demo.py forward path.

Package contents (only what the path needs):
  csrc/        HIP kernels + C ABI (include/esr_hip.h) -> libesr_hip.so
  _lib.py      ctypes binding (fails loudly, no fallback)
  engine.py    weight packing, workspace, op-list replay
  imdn.py ...  drop-in nn.Modules with the reference's ctor / state_dict surface
"""
from .arfdn import ARFDN  # noqa: F401
from .bmdn import BMDN  # noqa: F401
from .bsrn import BSRN  # noqa: F401
from .dwrfdn import DWRFDN  # noqa: F401
from .efdn import PLAINRFDN  # noqa: F401
from .esan import ESAN  # noqa: F401
from .fmen import FMEN  # noqa: F401
from .frfdn import FasterRFDN  # noqa: F401
from .imdn import IMDN  # noqa: F401
from .mdgn import MDGN  # noqa: F401
from .rfdn import RFDN  # noqa: F401
from .repafdn import RePAFDN  # noqa: F401
from .resdn import ResDN  # noqa: F401
from .rfdnext import RFDNeXt  # noqa: F401
from .rlfn import RLFN_cut  # noqa: F401

__all__ = ["ARFDN", "BMDN", "BSRN", "DWRFDN", "ESAN", "FMEN", "FasterRFDN", "IMDN", "MDGN", "PLAINRFDN", "RFDN", "RFDNeXt", "RLFN_cut", "RePAFDN", "ResDN"]
