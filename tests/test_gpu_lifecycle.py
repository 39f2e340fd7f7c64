"""-m gpu: a model's results across its lifetime, held to a FRESH instance (engine.HipSRModel: what sits between a parameter and a launch).

Packed blobs (the engine's and every network's _extra_pack), per-stream workspaces, LRU caches of plans, esr_op arrays with raw device pointers
and captured HIP graphs are all derived state; load_state_dict, .to(), set_compute and the plan-shaping flags invalidate it, MAX_PLANS /
MAX_STREAMS, copy.deepcopy and garbage collection evict from it.  A stale piece does not crash: it returns the previous checkpoint's image.

The reference of every case is a fresh instance -- same class, same constructor arguments, brought into the target state (weights, compute mode,
flags) BEFORE its first forward, use_graphs = False -- and every comparison is torch.equal: the forwards are deterministic (test_gpu_graph.py).
Weights B are the checkpoint times (1 + 0.02 u), u uniform in [-1, 1], seeded per key; every case that uses them asserts that they change the
result.  Each shape runs three times in a row: with graphs on, the second and third forwards are graph replays."""
import contextlib
import copy
import gc
import importlib.util
import io
import os
import pickle
import zlib

import pytest
import torch

import ntire2022_esr_amd as pkg
from conftest import GOLD, REPO
from ntire2022_esr_amd.registry import _entries, load_checkpoint
from test_gpu_stale_workspace import REGISTRY

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

spec = importlib.util.spec_from_file_location("plan_digest", os.path.join(REPO, "tools", "plan_digest.py"))
pd = importlib.util.module_from_spec(spec)
spec.loader.exec_module(pd)

# the seven networks whose checkpoints are goldens: (constructor as test_gpu_<net>.py calls it, checkpoint stem, data_range)
GOLDEN = {"fmen": (pkg.FMEN, "team03_fmen", 255.0), "efdn": (pkg.PLAINRFDN, "team05_efdn", 255.0), "frfdn": (pkg.FasterRFDN, "team25_frfdn", 1.0),
          "esan": (pkg.ESAN, "team34_esan", 255.0), "dwrfdn": (pkg.DWRFDN, "team35_rfdn", 255.0), "bmdn": (pkg.BMDN, "team37_bmdn", 1.0),
          "rfdnext": (lambda: pkg.RFDNeXt(block_type="RFDB", act_type="lrelu"), "team38_rfdnext", 1.0)}
NETS = list(REGISTRY) + list(GOLDEN)
MODES = {n: ("f32", "bf16") if n == "fmen" else ("f32", "bf16", "f16") for n in NETS}        # (FMEN refuses fp16 storage)
NET_MODES = [(n, c) for n in NETS for c in MODES[n]]
# the ESA minimum, below one tile; ragged tiles; a batch
SHAPES = [(1, 3, 15, 15), (1, 3, 24, 31), (2, 3, 17, 40)]
FOURTH = (1, 3, 33, 20)
# one network per storage type for the cases that are about the engine's caches, not about a network's blobs
THREE = [("team04_rlfn", "bf16"), ("imdn_baseline", "f32"), ("team18_bsrn", "f16")]
FLAGS = ("winograd", "hilo_skip", "tight_pitch")         # + every fuse_* property of the class

_cache = {}


def _spec(net):
    """(constructor, checkpoint A on the CPU, data_range)"""
    if ("spec", net) not in _cache:
        if net in GOLDEN:
            from safetensors.torch import load_file
            ctor, stem, dr = GOLDEN[net]
            sd = load_file(os.path.join(GOLD, stem + ".safetensors"))
        else:
            _, stem, dr, _, ctor = _entries()[REGISTRY[net]]
            sd = load_checkpoint(stem)
        _cache["spec", net] = (ctor, sd, dr)
    return _cache["spec", net]


def _weights(net, which):
    sd = _spec(net)[1]
    if which == "A":
        return sd
    if ("B", net) not in _cache:
        u = lambda k, v: torch.rand(v.shape, generator=torch.Generator().manual_seed(zlib.crc32(k.encode()))) * 2 - 1
        _cache["B", net] = {k: v * (1 + 0.02 * u(k, v)) for k, v in sd.items()}
    return _cache["B", net]


def _fresh(net, mode, which="A", flags=(), graphs=True):
    """a new instance in the target state before its first forward"""
    with contextlib.redirect_stdout(io.StringIO()):         # (BSRN prints its conv type, as the reference does)
        m = _spec(net)[0]()
    m.load_state_dict(_weights(net, which), strict=True)
    m.eval().set_compute(mode)
    for name, value in flags:
        setattr(m, name, value)
    m = m.to(DEV)
    m.use_graphs = graphs
    return m


def _inputs(net, shapes=tuple(SHAPES)):
    dr = _spec(net)[2]
    key = ("x", dr, shapes)
    if key not in _cache:
        _cache[key] = [(torch.rand(*s, generator=torch.Generator().manual_seed(100 * s[2] + s[3])) * dr).to(DEV) for s in shapes]
        torch.cuda.synchronize()
    return _cache[key]


def _ref(net, mode, which="A", flags=(), shapes=tuple(SHAPES)):
    """the fresh instance's results for `shapes`, computed once and left alone"""
    key = ("ref", net, mode, which, tuple(flags), shapes)
    if key not in _cache:
        m = _fresh(net, mode, which, flags, graphs=False)
        _cache[key] = [m(x).clone() for x in _inputs(net, shapes)]
        torch.cuda.synchronize()
    return _cache[key]


def _differ(a, b):
    """the condition on weights B (or a flag): no shape's result is left as it was"""
    return all(not torch.equal(x, y) for x, y in zip(a, b))


def _key(x):
    return tuple(x.shape) + (torch.device(DEV),)


def _check(m, xs, want, tag, graphs=True):
    """three forwards per shape, each equal to the reference; with graphs on the shape ends with a captured graph"""
    for x, r in zip(xs, want):
        ys = [m(x) for _ in range(3)]
        for i, y in enumerate(ys):
            assert torch.equal(y, r), (tag, tuple(x.shape), i, float((y - r).abs().max()))
        if graphs:
            assert m._plans[_key(x)].graph is not None, (tag, tuple(x.shape))


# ---- reload ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,mode", NET_MODES)
def test_reload_equals_a_fresh_instance(net, mode):
    """A-forwards with graphs -> load_state_dict(B) -> B's results, not A's -> load A -> the first results.  Every derived blob of the mode
    (`#s16`, `#post`, `#head#s16`, `#dense`, `#apost`, Winograd, hi + lo, each _extra_pack) must follow the parameters"""
    xs, ya, yb = _inputs(net), _ref(net, mode, "A"), _ref(net, mode, "B")
    assert _differ(ya, yb)
    m = _fresh(net, mode)
    _check(m, xs, ya, "A")
    m.load_state_dict(_weights(net, "B"), strict=True)
    _check(m, xs, yb, "B after A")
    m.load_state_dict(_weights(net, "A"), strict=True)
    _check(m, xs, ya, "A again")


@pytest.mark.parametrize("net,mode", [(n, "bf16") for n in NETS] + [("imdn_baseline", "f32"), ("team18_bsrn", "f16")])
def test_repack_after_untracked_edits(net, mode):
    """the documented contract (HipSRModel._ensure_packed): a sub-module's load_state_dict and p.copy_() do not mark the model; after
    repack(device) the results are the new weights'"""
    xs, ya, yb = _inputs(net), _ref(net, mode, "A"), _ref(net, mode, "B")
    assert _differ(ya, yb)
    m = _fresh(net, mode)
    _check(m, xs, ya, "A")
    b = _weights(net, "B")
    first, child = next(iter(m.named_children()))
    child.load_state_dict({k[len(first) + 1:]: v for k, v in b.items() if k.startswith(first + ".")}, strict=True)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if not k.startswith(first + "."):
                p.copy_(b[k])
    assert not m._dirty
    m.repack(torch.device(DEV))
    _check(m, xs, yb, "B after repack")


# ---- compute modes and flags ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", NETS)
def test_compute_switches_equal_fresh_instances(net):
    """f32 -> bf16 -> (f16) -> f32 on one instance, graphs captured in each mode; the last stage is the first, bit for bit (one reference)"""
    xs = _inputs(net)
    m = _fresh(net, "f32")
    for mode in MODES[net] + ("f32",):
        m.set_compute(mode)
        _check(m, xs, _ref(net, mode), mode)
    assert _differ(_ref(net, "f32"), _ref(net, "bf16"))


def _digest(net, mode, flip=None, shapes=tuple(SHAPES)):
    """what the network launches for SHAPES in `mode` with the flag `flip` inverted (CPU; tools/plan_digest.py) and the blobs it reads"""
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = _spec(net)[0]()
    m.compute = mode
    if flip:
        setattr(m, flip, not getattr(m, flip))
    m._repack("cpu")
    return [pd.plan_digest(m, (s[0], s[2], s[3])) for s in shapes], pd.packed_digest(m), getattr(m, flip) if flip else None


def _reactive_flags(net, mode):
    """[(flag, inverted value)] of the plan-shaping properties that this network's launches or blobs react to in `mode`"""
    cls = type(_fresh_cpu(net))
    names = [n for n in dir(cls) if isinstance(getattr(cls, n), property) and (n in FLAGS or n.startswith("fuse_"))]
    base = _digest(net, mode)[:2]
    out = []
    for n in names:
        plans, blobs, value = _digest(net, mode, n)
        if (plans, blobs) != base:
            out.append((n, value))
    return out


def _fresh_cpu(net):
    with contextlib.redirect_stdout(io.StringIO()):
        return _spec(net)[0]()


def test_flag_discovery_finds_the_known_flags():
    """the discovery of test_flag_switches is not blind: each network's own one-launch form, the shared switches"""
    got = lambda net, mode: {n for n, _ in _reactive_flags(net, mode)}
    assert got("imdn_baseline", "f32") == {"winograd"}
    assert got("rfdn_baseline", "bf16") >= {"hilo_skip", "tight_pitch", "fuse_esa_lowres"}
    assert "fuse_chain" in got("team04_rlfn", "bf16") and "fuse_hfab" in got("fmen", "bf16") and "fuse_step" in got("bmdn", "f16")
    assert "fuse_head" in got("esan", "bf16") and "fuse_cascade" in got("frfdn", "bf16") and "fuse_cx" in got("rfdnext", "bf16")
    assert "fuse_pair" in got("dwrfdn", "bf16") and "fuse_esa_lowres" in got("efdn", "f32")


@pytest.mark.parametrize("net,mode", NET_MODES)
def test_flag_switches_equal_fresh_instances(net, mode):
    """every plan-shaping flag the network reacts to in this mode, toggled after graphs exist: the result is a fresh instance's that had the
    flag before its first forward; toggled back, the first result.  use_graphs likewise"""
    xs, y0 = _inputs(net), _ref(net, mode)
    m = _fresh(net, mode)
    _check(m, xs, y0, "defaults")
    for flag, value in _reactive_flags(net, mode):
        setattr(m, flag, value)
        _check(m, xs, _ref(net, mode, "A", ((flag, value),)), f"{flag}={value}")
        setattr(m, flag, not value)
        _check(m, xs, y0, f"{flag} back")
    m.use_graphs = False
    _check(m, xs, y0, "graphs off", graphs=False)
    m.use_graphs = True
    _check(m, xs, y0, "graphs on again")


@pytest.mark.parametrize("net,mode", [("rfdn_baseline", "bf16"), ("team18_bsrn", "f16")])
def test_fuse_tail_switch_at_a_shape_that_reaches_it(net, mode):
    """fuse_tail shapes a plan from 256 tiles on (no shape of SHAPES): toggled on a live instance at 256 x 256"""
    big = ((1, 3, 256, 256),)
    base = _digest(net, mode, shapes=big)[:2]
    assert _digest(net, mode, "fuse_tail", shapes=big)[:2] != base
    xs, y0 = _inputs(net, big), _ref(net, mode, shapes=big)
    m = _fresh(net, mode)
    _check(m, xs, y0, "defaults")
    m.fuse_tail = False
    _check(m, xs, _ref(net, mode, "A", (("fuse_tail", False),), big), "fuse_tail off")
    m.fuse_tail = True
    _check(m, xs, y0, "fuse_tail back")


# ---- .to() / .float() ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net,mode", THREE)
def test_to_and_float_on_the_same_device(net, mode):
    xs, y0 = _inputs(net), _ref(net, mode)
    m = _fresh(net, mode)
    _check(m, xs, y0, "before")
    assert m.to(DEV) is m
    _check(m, xs, y0, ".to(same)")
    m.float()
    _check(m, xs, y0, ".float()")


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs")
@pytest.mark.parametrize("net,mode", THREE)
def test_to_another_device_and_back(net, mode):
    xs, y0 = _inputs(net), _ref(net, mode)
    m = _fresh(net, mode)
    _check(m, xs, y0, "cuda:0")
    m.to("cuda:1")
    for x, r in zip(xs, y0):
        for _ in range(3):
            assert torch.equal(m(x.to("cuda:1")).to(DEV), r)
    fresh = _fresh(net, mode, graphs=False).to("cuda:1")
    assert torch.equal(fresh(xs[1].to("cuda:1")).to(DEV), y0[1])
    m.to(DEV)
    _check(m, xs, y0, "back on cuda:0")


# ---- eviction, growth, deletion ------------------------------------------------------------------------------------------------------
FOUR = tuple(SHAPES) + (FOURTH,)


@pytest.mark.parametrize("net,mode", THREE)
def test_plan_eviction_with_launches_queued(net, mode):
    """MAX_PLANS = 2, four shapes round robin three times, three forwards a visit (the graph is captured and replayed), nothing synchronises:
    every evicted entry's graph is destroyed while its launches may still be queued (esr_graph_destroy waits for them)"""
    xs, want = _inputs(net, FOUR), _ref(net, mode, shapes=FOUR)
    m = _fresh(net, mode)
    m.MAX_PLANS = 2
    got = []
    for rnd in range(3):
        for x in xs:
            got.append([m(x) for _ in range(3)])
            assert m._plans[_key(x)].graph is not None and len(m._plans) <= 2
    torch.cuda.synchronize()
    for i, ys in enumerate(got):
        for y in ys:
            assert torch.equal(y, want[i % 4]), (i // 4, tuple(xs[i % 4].shape))


@pytest.mark.parametrize("net,mode", THREE)
def test_stream_context_eviction_with_launches_queued(net, mode):
    """MAX_STREAMS = 2, four streams in rotation, twice round, no synchronisation until the end: a context's workspace and graphs go while
    its stream may still be running them"""
    xs, want = _inputs(net, FOUR), _ref(net, mode, shapes=FOUR)
    m = _fresh(net, mode)
    m.MAX_STREAMS = 2
    streams = [torch.cuda.Stream(DEV) for _ in range(4)]
    got = []
    for rnd in range(2):
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                got.append([m(xs[(i + rnd) % 4]) for _ in range(3)])
            assert len(m._ctxs) <= 2
    torch.cuda.synchronize()
    for j, ys in enumerate(got):
        for y in ys:
            assert torch.equal(y, want[(j % 4 + j // 4) % 4]), j


@pytest.mark.parametrize("net,mode", THREE)
def test_workspace_growth_drops_the_graph_of_the_old_addresses(net, mode):
    """a larger shape moves the workspace: the small shape's entry is finalized again and its graph, which holds the old addresses, is gone
    before the next forward -- nothing writes into the freed workspace (a tensor of its size, most likely in its place, keeps its bytes)"""
    xs, want = _inputs(net), _ref(net, mode)
    m = _fresh(net, mode)
    _check(m, xs[:1], want[:1], "small")
    ent, old = m._plans[_key(xs[0])], m._ws
    ptr, size = old.data_ptr(), old.numel()
    del old
    _check(m, xs[2:], want[2:], "large")
    assert m._ws.numel() > size and m._ws.data_ptr() != ptr and m._plans[_key(xs[0])] is ent
    canary = torch.full((size,), 0xA5, dtype=torch.uint8, device=DEV)
    y = m(xs[0])
    assert ent.graph is None and ent.uses == 1 and ent.base[0] == m._ws.data_ptr()
    assert torch.equal(y, want[0])
    _check(m, xs[:1], want[:1], "small again")
    assert bool((canary == 0xA5).all())


@pytest.mark.parametrize("net,mode", THREE)
def test_results_survive_their_model(net, mode):
    """del m; gc.collect() with the forwards still queued; the freed blobs' and workspace's sizes are then allocated and filled on the stream"""
    xs, want = _inputs(net), _ref(net, mode)
    m = _fresh(net, mode)
    ys = [[m(x) for _ in range(3)] for x in xs]
    sizes = sorted({t.numel() for t in m._packed.values()})[-6:]
    ws = m._ws.numel()
    del m
    gc.collect()
    junk = [torch.full((n,), float("nan"), device=DEV) for n in sizes] + [torch.full((ws,), 0xFF, dtype=torch.uint8, device=DEV)]
    torch.cuda.synchronize()
    for y3, r in zip(ys, want):
        for y in y3:
            assert torch.equal(y, r)
    assert len(junk) == len(sizes) + 1


# ---- copies --------------------------------------------------------------------------------------------------------------------------
def _state(m):
    """addresses of everything of `m` that lives on the device or names device state"""
    ctxs = list(m._ctxs.values())
    ents = [e for c in ctxs for e in c.plans.values()]
    return dict(ws={c.ws.data_ptr() for c in ctxs}, entries={id(e) for e in ents}, graphs={e.graph.value for e in ents if e.graph is not None},
                blobs={t.data_ptr() for t in m._packed.values()}, params={p.data_ptr() for p in m.parameters()}, handle={m.handle})


@pytest.mark.parametrize("how", ["deepcopy", "pickle"])
@pytest.mark.parametrize("net,mode", [("team04_rlfn", "bf16"), ("imdn_baseline", "f32")])
def test_copy_of_a_model_that_has_run(net, mode, how):
    from torch.utils._python_dispatch import TorchDispatchMode
    xs, ya, yb = _inputs(net), _ref(net, mode, "A"), _ref(net, mode, "B")
    assert _differ(ya, yb)
    m = _fresh(net, mode)
    _check(m, xs, ya, "source")
    before = _state(m)
    m2 = copy.deepcopy(m) if how == "deepcopy" else pickle.loads(pickle.dumps(m))
    assert m2._ctxs == {} and m2._packed is None and _state(m) == before and all(p.is_cuda for p in m2.parameters())
    _check(m2, xs, ya, "copy")
    _check(m, xs, ya, "source after the copy ran")

    seen = []

    class Log(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if "sr_forward" in str(func):
                seen.append(args[1])
            return func(*args, **(kwargs or {}))

    with Log():
        y1, y2 = m(xs[1]), m2(xs[1])
    assert seen == [m.handle, m2.handle] and m.handle != m2.handle and torch.equal(y1, ya[1]) and torch.equal(y2, ya[1])
    s1, s2 = _state(m), _state(m2)
    for what in s1:
        assert s1[what] and s2[what] and not s1[what] & s2[what], what
    m2.load_state_dict(_weights(net, "B"), strict=True)
    _check(m2, xs, yb, "copy with B")
    _check(m, xs, ya, "source still A")
    m.load_state_dict(_weights(net, "B"), strict=True)
    m2.load_state_dict(_weights(net, "A"), strict=True)
    _check(m, xs, yb, "source with B")
    _check(m2, xs, ya, "copy back on A")
    del m
    gc.collect()
    _check(m2, xs, ya, "copy after its source is gone")
