"""copy.deepcopy and pickle (torch.save(model)) of a HipSRModel that has already run (no GPU).

A model that has run holds state no copy may share: packed blobs, per-stream contexts with plans whose esr_op arrays carry raw device pointers,
and esr_graph handles that _Entry.__del__ destroys.  Here that state is built by hand on the CPU -- a Plan finalized against an integer base
into an _Entry with a non-null graph handle, inside a _StreamCtx of m._ctxs, next to a _packed dict -- and both ways of copying must give a
model that carries parameters, specs, compute mode and flags and nothing else (engine.HipSRModel.__getstate__), and leave the source as it was."""
import contextlib
import copy
import ctypes
import gc
import io
import pickle

import pytest
import torch

import ntire2022_esr_amd as pkg
from ntire2022_esr_amd import _lib as L
from ntire2022_esr_amd import engine as E
from ntire2022_esr_amd.registry import _entries

CTORS = {f"id{k}": v[4] for k, v in _entries().items()}
CTORS.update(FMEN=pkg.FMEN, PLAINRFDN=pkg.PLAINRFDN, FasterRFDN=pkg.FasterRFDN, ESAN=pkg.ESAN, DWRFDN=pkg.DWRFDN, BMDN=pkg.BMDN,
             RFDNeXt=lambda: pkg.RFDNeXt(block_type="RFDB", act_type="lrelu"))
BASE = 0x10000000
KEY = (1, 3, 24, 31, torch.device("cuda", 0))
CTX_KEY = (torch.device("cuda", 0), 0x7F0000001230)
GRAPH = 0x5EED0


def _build(name):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):         # (BSRN prints its conv type, as the reference does)
        return CTORS[name]().eval()


class _Blobs(E._AnyBlob):
    """_AnyBlob for a whole plan: an fp32 conv also asks whether a Winograd blob exists, a low-resolution depthwise layer whether a padded one"""

    def get(self, name, default=None):
        return default

    def __contains__(self, name):
        return False


COPIES = {"deepcopy": copy.deepcopy, "pickle": lambda m: pickle.loads(pickle.dumps(m))}


@pytest.fixture
def destroyed(monkeypatch):
    """the handles passed to esr_graph_destroy while the test runs (none of them is a real graph), and the entries whose fake handle must be
    gone before the real function is back"""
    calls, entries = [], []
    monkeypatch.setattr(L.lib(), "esr_graph_destroy", lambda g: calls.append(g.value if isinstance(g, ctypes.c_void_p) else g))
    yield calls, entries
    for ent in entries:
        ent.graph = None


def _run_state(m, store, entries):
    """gives `m` the state of a model after forwards: one plan entry with a finalized op array and a graph handle, and packed blobs"""
    m.set_compute(store)
    plan = E.Plan(1, 24, 31, store)
    m._build_plan(plan, 3)
    ent = E._Entry(plan)
    ent.base = (BASE, plan.total_lo)
    ent.arr, ent.in_idx, ent.out_idx = plan.finalize(ent.base, _Blobs())
    ent.graph, ent.uses = ctypes.c_void_p(GRAPH), 3
    entries.append(ent)
    ctx = E._StreamCtx()
    ctx.plans[KEY], ctx.lo_cap, ctx.ws_owner = ent, plan.total_lo, KEY
    ctx.ws = torch.zeros(max(plan.total_lo + plan.total, 256), dtype=torch.uint8)
    m._ctxs[CTX_KEY] = ctx
    m._packed = {"__fake__": torch.zeros(4)}
    m._dirty = False
    assert len(ent.arr) == len(plan.ops) > 0 and ent.in_idx and ent.out_idx
    return ctx, ent


@pytest.mark.parametrize("how", list(COPIES))
@pytest.mark.parametrize("name,store,flag", [("id4", "bf16", "fuse_chain"), ("id-1", "f32", "winograd"), ("id18", "f16", "fuse_esa_lowres"),
                                             ("FMEN", "bf16", "fuse_hfab"), ("ESAN", "f32", "fuse_head")])
def test_copy_of_a_model_that_has_run(name, store, flag, how, destroyed):
    calls, entries = destroyed
    m = _build(name)
    setattr(m, flag, not getattr(m, flag))                  # a flag off its default travels with the copy
    ctx, ent = _run_state(m, store, entries)
    packed, lock, handle, arr = m._packed, m._lock, m.handle, ent.arr
    c = COPIES[how](m)
    # the copy: parameters, specs, compute mode and flags -- and nothing that points at the source's device state
    assert type(c) is type(m) and c is not m
    assert c._ctxs == {} and c._packed is None and c._packed_sig is None and c._dirty
    assert c.compute == store and getattr(c, flag) == getattr(m, flag) and c.use_graphs == m.use_graphs
    assert c._conv_specs == m._conv_specs and c._dense_specs == m._dense_specs and c._dw_specs == m._dw_specs
    sd, sc = m.state_dict(), c.state_dict()
    assert list(sd) == list(sc) and all(torch.equal(sd[k], sc[k]) for k in sd)
    assert not {p.data_ptr() for p in m.parameters()} & {p.data_ptr() for p in c.parameters()}
    assert isinstance(c._lock, E._ModelLock) and c._lock is not lock and c._lock._l is not lock._l
    with lock, c._lock:
        pass
    assert c.handle != handle and E._LIVE[c.handle] is c and E._LIVE[handle] is m
    # the source is as it was
    assert m._ctxs == {CTX_KEY: ctx} and ctx.plans[KEY] is ent and ent.arr is arr and ent.graph.value == GRAPH and ent.uses == 3
    assert m._packed is packed and not m._dirty and m._lock is lock and m.handle == handle and ctx.ws_owner == KEY
    # the copy re-packs on its next use, into blobs of its own
    c._ensure_packed(torch.device("cpu"))
    assert c._packed is not None and c._packed is not packed and not c._dirty and "__fake__" not in c._packed
    assert m._packed is packed
    # a load marks the model it is called on
    c.load_state_dict(sd)
    assert c._dirty and not m._dirty
    c._ensure_packed(torch.device("cpu"))
    m.load_state_dict(sc)
    assert m._dirty and not c._dirty
    # nobody but the source's own entry destroys the source's graph, and only once
    del c
    gc.collect()
    assert calls == []
    m._drop_plans()
    assert calls == [GRAPH] and ent.graph is None
    del m, ctx, ent
    gc.collect()
    assert calls == [GRAPH]


@pytest.mark.parametrize("how", list(COPIES))
def test_copy_of_a_copy_and_shallow_copy(how, destroyed):
    calls, entries = destroyed
    m = _build("id4")
    _run_state(m, "bf16", entries)
    c = COPIES[how](COPIES[how](m))
    s = copy.copy(m)
    for k in (c, s):
        assert k._ctxs == {} and k._packed is None and k._dirty and E._LIVE[k.handle] is k
    assert len({m.handle, c.handle, s.handle}) == 3
    del c, s
    gc.collect()
    assert calls == [] and entries[0].graph.value == GRAPH


@pytest.mark.parametrize("name", list(CTORS))
def test_every_network_pickles_before_its_first_forward(name):
    m = _build(name)
    m.set_compute("bf16")
    c = pickle.loads(pickle.dumps(m))
    d = copy.deepcopy(m)
    sd = m.state_dict()
    for k in (c, d):
        sk = k.state_dict()
        assert type(k) is type(m) and k.compute == "bf16" and list(sk) == list(sd) and all(torch.equal(sd[n], sk[n]) for n in sd)
        assert k.handle != m.handle and E._LIVE[k.handle] is k and k._dirty and k._packed is None
