"""tools/plan_digest.py says something: equal plans give equal digests, and a flag, a shape or a wrong blob name does not go unnoticed; its
whole output is the recorded one (tests/golden/plan_digests_14_networks.txt, which holds every network by now); and every op of every plan
reads exactly the blobs it declares (engine._Op.blobs), which the model has packed."""
import importlib.util
import os

import pytest
import torch

from conftest import REPO

spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(REPO, "tools", "plan_digest.py"))
pd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pd)

from ntire2022_esr_amd import MDGN, _lib as L
from ntire2022_esr_amd.engine import CX1, CX2, DWPW, Plan, _Fused

SHAPE = (2, 45, 70)
GOLDEN = os.path.join(REPO, "tests", "golden", "plan_digests_14_networks.txt")
# The cells whose flag keeps a one-launch form out of every plan.  The fixture was recorded when the networks packed that form's blobs
# whatever the flag said; now the ops name what they read, and these cells hold the default build's blobs minus (suffixes, how many) that no
# op reads.
DROPPED = {("RFDNeXt", "bf16", "fuse_cx"): ((CX1, CX2), 8), ("RFDNeXt", "f16", "fuse_cx"): ((CX1, CX2), 8),
           ("DWRFDN", "bf16", "fuse_pair"): ((DWPW,), 24), ("DWRFDN", "f16", "fuse_pair"): ((DWPW,), 24)}


def test_output_matches_the_fixture():
    """The tool's whole output -- every network in every storage, the defaults and every flag flipped: per cell the SHA-256 over the packed
    blobs and the one over the cost entries and complexity terms of its plans; per shape the op count, the arena sizes and the SHA-256 over
    the finalized descriptors and the buffer table -- is the fixture (`python tools/plan_digest.py`), line for line.  Only FMEN's fp16 cells
    refuse.
    The four DROPPED cells: their plan lines are the recorded ones once the blobs stand at the recorded addresses (ranks in the default
    build's names); in place of their `packed` line, the key set is the default build's minus exactly the dropped suffixes' names, and every
    blob equals the default build's."""
    want = open(GOLDEN).read().splitlines()
    got = []
    for cell in pd.cells():
        if cell not in DROPPED:
            got.append(pd.cell_lines(*cell)[1])
            continue
        (suffixes, count), base = DROPPED[cell], pd.build(*cell[:2])
        m, lines = pd.cell_lines(*cell, names=set(base._packed))
        gone = {n for n in base._packed if n.endswith(suffixes)}
        assert len(gone) == count and set(m._packed) == set(base._packed) - gone, cell
        assert all(torch.equal(m._packed[n], base._packed[n]) for n in m._packed), cell
        got.append(lines)
    got = pd.arrange(got)
    packed_of_dropped = tuple(f"{name} {store} {flip} packed " for name, store, flip in DROPPED)
    assert sum(line.startswith(packed_of_dropped) for line in want) == len(DROPPED)
    assert [line for line in got if not line.startswith(packed_of_dropped)] == [line for line in want if not line.startswith(packed_of_dropped)]
    refused = [line.split(" refused: ")[0] for line in got if " refused: " in line]
    assert refused == ["FMEN f16 defaults", "FMEN f16 tight_pitch", "FMEN f16 fuse_hfab"]


class Recorder(pd.Blobs):
    """the names an encode reads with weights[name] (a lookup with .get() or `in` is an optional one: the Winograd image)"""
    def __init__(self, names):
        super().__init__(names)
        self.read = set()

    def __getitem__(self, name):
        self.read.add(name)
        return self.at[name]


def test_every_op_reads_the_blobs_it_declares():
    """every cell of the tool, every shape: each op of the plan, encoded on its own, reads exactly the names its blobs() lists -- a fused op
    a subset: the rest is what the ops it replaces would read in a plan that keeps them -- and the model has packed every one of them"""
    checked = 0
    for cell in pd.cells():
        try:
            m = pd.build(*cell)
        except L.EsrError:
            assert cell[:2] == ("FMEN", "f16")
            continue
        for shape in pd.SHAPES:
            plan = Plan(*shape, m._store())
            m._build_plan(plan, m.in_nc)
            for o in plan.ops:
                rec = Recorder(m._packed)
                o.encode(L.Op(), plan, (0x10000000, plan.total), rec)
                declared = {name for name, kind, srcs in o.blobs(plan)}
                assert (rec.read <= declared) if isinstance(o, _Fused) else (rec.read == declared), (cell, shape, o.kind, rec.read ^ declared)
                assert declared <= set(m._packed), (cell, shape, o.kind, declared - set(m._packed))
                checked += 1
    assert checked > 10000


def test_a_blob_nobody_packs_is_refused_at_repack():
    """an op that names a blob which neither the engine's packers nor the network's _extra_pack build: an EsrError with the op and the blob,
    when the model packs -- not a KeyError at the first forward"""
    class Forgetful(MDGN):
        def _extra_pack(self, packed, device):
            pass
    m = Forgetful()
    m.compute = "bf16"
    with pytest.raises(L.EsrError, match=r"B\.0\.conv_fuse\.0.*mdsagate.*B\.0\.sa\.0#rep#s16"):
        m._repack("cpu")


def test_two_instances_agree():
    a, b = pd.build("RFDN", "bf16"), pd.build("RFDN", "bf16")
    assert a is not b and pd.plan_digest(a, SHAPE) == pd.plan_digest(b, SHAPE)
    assert pd.packed_digest(a) == pd.packed_digest(b)


def test_flag_and_shape_change_the_digest():
    base = pd.plan_digest(pd.build("RFDN", "bf16"), SHAPE)
    assert pd.plan_digest(pd.build("RFDN", "bf16", "fuse_esa_lowres"), SHAPE)[3] != base[3]
    assert pd.plan_digest(pd.build("RFDN", "bf16"), (2, 45, 71))[3] != base[3]


def test_missing_blob_name_raises():
    m = pd.build("RFDN", "bf16")
    names = sorted(m._packed)
    assert pd.plan_digest(m, SHAPE, names) == pd.plan_digest(m, SHAPE)
    with pytest.raises(KeyError):
        pd.plan_digest(m, SHAPE, [n for n in names if n != "B2.c5#s16"])
