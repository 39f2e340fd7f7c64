"""-m gpu: no plan's result depends on what its workspace held before (engine.HipSRModel.rezero_on_switch = False).

The engine keeps one grow-only workspace per stream and shares it between the plans of all shapes without re-zeroing: every pad slot is only
ever multiplied by a zero weight, added to an accumulator nobody stores, or copied into another pad slot, so stale FINITE values of the same
element type cannot reach a result.  Every form the engine plans is held to that here, bit for bit (torch.equal; nothing has a tolerance):

  1. the whole workspace overwritten with hostile finite patterns (tests/_poison.py) between two forwards of one shape -- below one tile,
     ragged tiles, a batch of several tiles; esr_run_ops and graph replay; a failure names the plan buffers that let the pattern through;
  2. thirty shapes through one workspace and back (the logic of test_gpu_big.py's _hundred_shapes) for FMEN, EFDN, BMDN and ESAN;
  3. forwards overlapped on four streams against serial ones for the same four networks;
  4. after a forward with a non-finite output: the harness's flag is raised, invalidate_workspaces() restores the earlier result."""
import os

import pytest
import torch

import _poison as P
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# network -> (how test_gpu_<network>.py builds it, data_range, the flag that selects its one-launch form, op kind and count of that form)
GOLD_NETS = {"fmen": ("FMEN", "team03_fmen", 255.0, "fuse_hfab", "chain", 4),
             "efdn": ("PLAINRFDN", "team05_efdn", 255.0, "fuse_esa_lowres", "lowres", 4),
             "bmdn": ("BMDN", "team37_bmdn", 1.0, "fuse_step", "distill", 12),
             "esan": ("ESAN", "team34_esan", 255.0, "fuse_head", "reshead", 16)}
REGISTRY = {"imdn_baseline": -1, "rfdn_baseline": 0, "team04_rlfn": 4, "team18_bsrn": 18,
            "team06_v1": 6, "team08_sfdn": 8, "team22_rep_rfdn": 22, "team26_imdn_nb7": 26, "team40_rfdn_pruned": 40}

# (network, compute, fused): fused is None for the networks whose plans have one form per storage type
FORMS = ([("imdn_baseline", "f32", None), ("imdn_baseline", "bf16", None), ("rfdn_baseline", "f32", None), ("rfdn_baseline", "bf16", None),
          ("team04_rlfn", "f32", None), ("team04_rlfn", "bf16", None), ("team18_bsrn", "f32", None), ("team18_bsrn", "f16", None),
          ("fmen", "f32", False), ("fmen", "bf16", True), ("fmen", "bf16", False)]
         + [("efdn", c, f) for c in ("f32", "bf16", "f16") for f in (True, False)]
         + [("bmdn", "f32", False)] + [("bmdn", c, f) for c in ("bf16", "f16") for f in (True, False)]
         + [("esan", "f32", False)] + [("esan", c, f) for c in ("bf16", "f16") for f in (False, True)]
         + [(n, c, None) for n in ("team06_v1", "team08_sfdn", "team22_rep_rfdn", "team26_imdn_nb7", "team40_rfdn_pruned") for c in ("f32", "bf16")])
# below one 16 x 16 tile; ragged tiles; a batch of several tiles
SHAPES = [(1, 3, 15, 15), (1, 3, 24, 31), (2, 3, 45, 70)]

_models = {}


def _model(name, compute, fused=None, lowres=True):
    """(model, data_range) in the asked form, graphs on; one instance per network.  lowres: ESA's low-resolution branch as one op (every
    network's default; EFDN's `fused` is this flag)"""
    if name not in _models:
        if name in GOLD_NETS:
            import ntire2022_esr_amd
            from safetensors.torch import load_file
            ctor, stem, dr = GOLD_NETS[name][:3]
            m = getattr(ntire2022_esr_amd, ctor)()
            m.load_state_dict(load_file(os.path.join(GOLD, stem + ".safetensors")), strict=True)
            _models[name] = (m.eval().to(DEV), dr)
        else:
            from ntire2022_esr_amd.registry import select_model
            m, _, dr, _ = select_model(REGISTRY[name], torch.device(DEV))
            _models[name] = (m, dr)
    m, dr = _models[name]
    m.set_compute(compute)
    if hasattr(m, "fuse_esa_lowres"):
        m.fuse_esa_lowres = lowres
    if fused is not None:
        setattr(m, GOLD_NETS[name][3], fused)
    m.use_graphs = True
    assert not m.rezero_on_switch
    return m, dr


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _assert_form(name, m, shape, fused):
    """the plan of `shape` holds the network's one-launch op exactly when the form asks for it"""
    if fused is None:
        return
    kind, count = GOLD_NETS[name][4:]
    ops = m._plans[_key(shape)].plan.ops
    n = sum(o.kind == kind and (name != "fmen" or o.gate) and (name != "efdn" or o.w is None) for o in ops)
    assert n == (count if fused else 0), (name, shape, fused, n)
    if name == "efdn":                                          # the per-op form pools with its own launch
        assert sum(o.kind == "pool7" for o in ops) == (0 if fused else 4)


def _input(shape, dr, seed):
    return (torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) * dr).to(DEV)


def _ctx0(m):
    dev = torch.device(DEV)
    return m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]


_pattern_cache = {}


def _pattern(name, nbytes, lo_cap, store, seed):
    """P.pattern on the device; the last one is kept (the esr_run_ops and the graph pass of a case ask for the same bytes)"""
    key = (name, nbytes, lo_cap, store, seed)
    if key not in _pattern_cache:
        if len(_pattern_cache) >= len(P.PATTERNS):
            _pattern_cache.clear()
        _pattern_cache[key] = P.pattern(name, nbytes, lo_cap, store, seed).to(DEV)
    return _pattern_cache[key]


def _leaking_buffers(m, x, y0, data, ent):
    """names of the plan buffers through which `data` reaches the result: each poisoned alone over a zeroed workspace"""
    ctx = _ctx0(m)
    bad = []
    for name, start, size in P.buffer_ranges(ent.plan, ctx.lo_cap):
        ctx.ws.zero_()
        m(x)                                                   # this plan's own leftovers, as in the failing run
        P.poison_range(ctx.ws, data, start, size)
        if not torch.equal(m(x), y0):
            bad.append(name)
    return bad


def _poisoned_forwards_equal_clean(name, compute, fused, shape, lowres=True):
    m, dr = _model(name, compute, fused, lowres)
    x = _input(shape, dr, 17 * shape[2] + shape[3])
    try:
        results = []
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()                                     # a fresh context: prepare() zero-fills the workspace
            ent = m.prepare(shape, DEV)
            ctx = _ctx0(m)
            assert ctx.ws_owner == _key(shape) and not bool(ctx.ws.any())
            _assert_form(name, m, shape, fused)
            y0 = m(x).clone()
            if graphs:
                m(x)                                            # the second forward of a shape captures the graph; replays from here on
                assert ent.graph is not None
            assert bool(torch.isfinite(y0).all())
            results.append(y0)
            ptr, graph = ctx.ws.data_ptr(), ent.graph
            for pat in P.PATTERNS:
                data = _pattern(pat, ctx.ws.numel(), ctx.lo_cap, compute, shape[2])
                ctx.ws.copy_(data)                              # ws_owner stays: the engine does not zero-fill
                y = m(x)
                # the forward really ran on the poisoned bytes: same workspace, same plan entry, same graph, no zero fill in between
                assert ctx.ws.data_ptr() == ptr and m._plans[_key(shape)] is ent and ent.graph is graph and ctx.ws_owner == _key(shape)
                if not torch.equal(y, y0):
                    diff = float((y - y0).abs().max())
                    leaks = _leaking_buffers(m, x, y0, data, ent)
                    pytest.fail(f"{name} {compute} fused={fused} {shape} graphs={graphs} pattern {pat}: max|y - y0| = {diff:.3e}, "
                                f"{int((y != y0).sum())} of {y.numel()} values differ; buffers that let it through: {leaks}")
        assert torch.equal(results[0], results[1])              # (graph replay and esr_run_ops agree, as the per-network tests say)
    finally:
        m.invalidate_workspaces()                               # the next forward of this model starts from zeros again


_ids = lambda s: "x".join(str(v) for v in s)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("name,compute,fused", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(name, compute, fused, shape):
    _poisoned_forwards_equal_clean(name, compute, fused, shape)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
@pytest.mark.parametrize("compute", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("name", ["rfdn_baseline", "team04_rlfn", "team18_bsrn", "bmdn", "esan"])
def test_per_op_esa_branch_does_not_depend_on_stale_workspace_bytes(name, compute, shape):
    """fuse_esa_lowres off (no network's default; EFDN's is in FORMS): the low-resolution maps come from one launch per layer.  These stored
    only their f < 16 channels, and the fp16 ESA apply kernel rounds all 16 slots of bilinear(c3) + conv_f(c1) to fp16 before conv4's zero
    weight rows: a stale fp32 value beyond 65504 in a pad slot of c3 became Inf, then NaN -- found by this module in EFDN's fp16 per-op form
    (pattern 0x77, buffer esa_c3) and in BSRN's (buffer esa_b, behind a depthwise launch), fixed by storing the whole dense map
    (engine._stored_width; engine.Dw.encode)"""
    fused = True if name in GOLD_NETS and compute != "f32" else (False if name in GOLD_NETS else None)
    _poisoned_forwards_equal_clean(name, compute, fused, shape, lowres=False)
    ops = _models[name][0]._plans[_key(shape)].plan.ops
    assert not any(o.kind == "lowres" for o in ops) and any(o.kind in ("pool", "pool7") for o in ops)


# ---- 2. thirty shapes through one workspace ------------------------------------------------------------------------------------------
# one 16-bit one-launch form, one 16-bit per-op form and fp32 per network
SWITCH_FORMS = [("fmen", "bf16", True), ("fmen", "bf16", False), ("fmen", "f32", False),
                ("efdn", "bf16", True), ("efdn", "f16", False), ("efdn", "f32", True),
                ("bmdn", "bf16", True), ("bmdn", "f16", False), ("bmdn", "f32", False),
                ("esan", "f16", True), ("esan", "bf16", False), ("esan", "f32", False)]


def _many_shapes(m, dr, nshapes=30):
    """test_gpu_big.py's _hundred_shapes for any model: the first result is reproduced bit for bit after `nshapes` other shapes ran in
    the same workspace; the second pass re-plans and re-allocates nothing"""
    g = torch.Generator().manual_seed(0)
    x0 = (torch.rand(1, 3, 40, 56, generator=g) * dr).to(DEV)
    y0 = m(x0).clone()
    shapes = [(24 + (i * 7) % 41, 20 + (i * 11) % 53) for i in range(nshapes)]
    big = max(m.workspace_bytes(1, h, w) for h, w in shapes)
    for h, w in shapes:
        m.prepare((1, 3, h, w), DEV)
        m((torch.rand(1, 3, h, w, generator=g) * dr).to(DEV))
    torch.cuda.synchronize()
    assert len(m._plans) <= m.MAX_PLANS and m._ws.numel() >= big
    base = m._ws.data_ptr()
    for h, w in shapes[:20]:
        ent = m._plans[_key((1, 3, h, w))]
        m((torch.rand(1, 3, h, w, generator=g) * dr).to(DEV))
        assert m._plans[_key((1, 3, h, w))] is ent and m._ws.data_ptr() == base
    assert torch.equal(m(x0), y0)


@pytest.mark.parametrize("name,compute,fused", SWITCH_FORMS)
def test_thirty_shapes_one_workspace(name, compute, fused):
    m, dr = _model(name, compute, fused)
    _many_shapes(m, dr)
    _assert_form(name, m, (1, 3, 40, 56), fused)


# ---- 3. overlapped streams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,compute", [("fmen", "bf16"), ("efdn", "f16"), ("bmdn", "bf16"), ("esan", "f16")])
def test_forwards_on_several_streams_equal_serial(name, compute):
    """the body of test_gpu_big.py's test of the same name for the one-launch forms: ten shapes round-robin on four streams, one workspace per
    stream context, every overlapped result bit-identical to its serial one.  10 rounds = 100 overlapped forwards per network (the 40 rounds
    of the original were sized to one known defect's rate)"""
    m, dr = _model(name, compute, True)
    g = torch.Generator().manual_seed(3)
    shapes = [(85, 128), (96, 128), (128, 85), (74, 128), (85, 128), (87, 128), (128, 96), (85, 128), (85, 128), (64, 64)]
    xs = [(torch.rand(1, 3, h, w, generator=g) * dr).to(DEV) for h, w in shapes]
    want = [m(x).clone() for x in xs]
    _assert_form(name, m, (1, 3, 85, 128), True)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(DEV) for _ in range(4)]
    for rnd in range(10):
        got = []
        for i, x in enumerate(xs):
            with torch.cuda.stream(streams[(i + rnd) % 4]):
                got.append(m(x))
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (rnd, i)
    dev = torch.device(DEV)
    used = {(dev, torch.cuda.default_stream(dev).cuda_stream)} | {(dev, s.cuda_stream) for s in streams}
    assert len(used) == 5 and used <= set(m._ctxs)          # default stream + 4, one workspace each
    assert len({m._ctxs[k].ws.data_ptr() for k in used}) == 5


# ---- 4. recovery after a non-finite forward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,compute,fused", [("imdn_baseline", "bf16", None), ("rfdn_baseline", "bf16", None), ("team04_rlfn", "bf16", None),
                                                ("team18_bsrn", "f16", None), ("fmen", "bf16", True), ("efdn", "f16", True),
                                                ("bmdn", "bf16", True), ("esan", "f16", True)])
def test_invalidate_workspaces_recovers_from_a_nonfinite_forward(name, compute, fused):
    """what harness.run does when an image overflows: the flag of ops.tensor2uint_device is raised (the long skip carries the input's Inf to
    the output), invalidate_workspaces() makes the next forward zero-fill, and a shape whose pad slots lay under the Inf / NaN values computes
    what it computed before"""
    from ntire2022_esr_amd import ops
    m, dr = _model(name, compute, fused)
    x = _input((1, 3, 24, 31), dr, 41)
    xb = _input((1, 3, 31, 24), dr, 43)
    xb[0, 1, 15, 12] = float("inf")
    try:
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()
            y0 = m(x).clone()
            if graphs:
                assert torch.equal(m(x), y0) and m._plans[_key(x.shape)].graph is not None
            assert bool(torch.isfinite(y0).all())
            yb = m(xb)
            flag = torch.zeros(1, dtype=torch.int32, device=DEV)
            ops.tensor2uint_device(yb, dr, nonfinite=flag)
            assert int(flag.item()) == 1, (name, compute, graphs)
            m.invalidate_workspaces()
            y = m(x)
            assert torch.equal(y, y0), (name, compute, graphs, float((y - y0).abs().max()))
            if graphs:
                assert m._plans[_key(x.shape)].graph is not None
    finally:
        m.invalidate_workspaces()
