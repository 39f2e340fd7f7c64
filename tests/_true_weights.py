"""The seven newer networks with their unrounded fp32 checkpoints (tools/gen_golden_true_weights.py): what tests/test_true_weight_fixtures.py
and tests/test_gpu_true_weights.py share.

Every network is described by how its OWN GPU test file builds and bounds it: the class and its constructor arguments, the flag that chooses
between the fused and the per-op form, the (compute, flag) pairs that file runs at 256 x 256, the kind and number of fused ops it asserts,
the bar of its fp32 e2e test, and the range its max |dy| / range divides by.  BUDGET and MAX_REL are read from that module, not repeated."""
import importlib
import os
from collections import namedtuple

import numpy as np

from conftest import GOLD

FILE_LIMIT = 1 << 20          # no committed file is larger

Net = namedtuple("Net", "stem module cls kwargs flag forms fused e2e_over_output rel_over_output")
_FORMS16 = [("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]
NETS = {n.stem: n for n in [
    # FMEN: bf16 only (fp16 storage is refused); test_gpu_fmen.py runs fuse_hfab on and off
    Net("team03_fmen", "test_gpu_fmen", "FMEN", {}, "fuse_hfab", [("bf16", True), ("bf16", False)], None, True, False),
    # EFDN: test_gpu_efdn.py builds every 16-bit plan with the fused stride-7 branch
    Net("team05_efdn", "test_gpu_efdn", "PLAINRFDN", {}, "fuse_esa_lowres", [("bf16", True), ("f16", True)], None, True, False),
    Net("team25_frfdn", "test_gpu_frfdn", "FasterRFDN", {}, "fuse_cascade", _FORMS16, ("cascade", 4), False, False),
    Net("team34_esan", "test_gpu_esan", "ESAN", {}, "fuse_head", _FORMS16, ("reshead", 16), True, True),
    Net("team35_rfdn", "test_gpu_dwrfdn", "DWRFDN", {}, "fuse_pair", _FORMS16, ("dwpw", 12), False, False),
    Net("team37_bmdn", "test_gpu_bmdn", "BMDN", {}, "fuse_step", _FORMS16, ("distill", 12), True, False),
    Net("team38_rfdnext", "test_gpu_rfdnext", "RFDNeXt", dict(block_type="RFDB", act_type="lrelu"), "fuse_cx", _FORMS16, ("cx", 4),
        False, False),
]}
# the flag of an fp32 plan, as each file's own fp32 tests set it (an fp32 plan has the per-op form only; FMEN and EFDN keep their default)
F32_FLAG = {"team03_fmen": True, "team05_efdn": True}

# test_gpu_dwrfdn.py and test_gpu_rfdnext.py bound max |dy| / range in fp32 only, so they have no 16-bit MAX_REL to import.  The other five
# files define theirs as TWICE the largest value measured with exact (bf16-representable) weights over both sizes and both forms; the same
# rule applied to the exact-weight figures DESIGN.md records for these two (sections 7h and 7g, "Accuracy against the reference's goldens"):
#   DWRFDN   bf16 6.99e-3 (256 x 256, both forms), f16 1.36e-3 (256 x 256)
#   RFDNeXt  bf16 4.60e-3 (256 x 256, fused),      f16 6.85e-4 (fused)
MAX_REL_16 = {"team35_rfdn": {"bf16": 1.40e-2, "f16": 2.72e-3},
              "team38_rfdnext": {"bf16": 9.20e-3, "f16": 1.37e-3}}


def module(net):
    return importlib.import_module(net.module)


def budget(net, compute):
    return module(net).BUDGET[compute]


def max_rel(net, compute):
    own = getattr(module(net), "MAX_REL", {})
    return own[compute] if compute in own else MAX_REL_16[net.stem][compute]


def true_paths(stem):
    """the fp32 checkpoint's file(s): one, or two where one would be beyond FILE_LIMIT"""
    ps = [os.path.join(GOLD, stem + "_f32.safetensors"), os.path.join(GOLD, stem + "_f32.part2.safetensors")]
    return [p for p in ps if os.path.exists(p)]


def load_true(stem):
    from safetensors.torch import load_file
    sd = {}
    for p in true_paths(stem):
        part = load_file(p)
        assert not set(part) & set(sd), p
        sd.update(part)
    return sd


def load_rounded(stem):
    from safetensors.torch import load_file
    return load_file(os.path.join(GOLD, stem + ".safetensors"))


def golden(stem):
    """true_<stem>.npz with the inputs it refers to: xb, xc of e2e_<stem>.npz and lr of big_<stem>_256x256.npz"""
    g = dict(np.load(os.path.join(GOLD, f"true_{stem}.npz")))
    e2e = np.load(os.path.join(GOLD, f"e2e_{stem}.npz"))
    g["xb"], g["xc"] = e2e["xb"], e2e["xc"]
    g["lr"] = np.load(os.path.join(GOLD, f"big_{stem}_256x256.npz"))["lr"]
    return g


def rel_range(net, g):
    dr = float(g["data_range"])
    return max(dr, float(np.abs(g["sr_sample"]).max())) if net.rel_over_output else dr
