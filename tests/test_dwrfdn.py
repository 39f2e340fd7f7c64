"""CPU: team 35's RFDN (NTIRE 2022 ESR, models.team35_rfdn.rfdn.RFDN) on the engine -- checkpoint surface and refusals, complexity counters
in both forms of the refinement path and every storage, plan shape, the `Dw` residual fields (additive: a BSRN plan's depthwise ops encode
as before), the packers (`con_`, the fused path's 1x1s), the shim import path, and the C ABI's validation of esr_dwpw_pair_s16 /
esr_esa_unshuffle_f32 without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team35_rfdn.safetensors")
WANT = {"activations": 229071536.0, "num_conv": 88, "flops": 13981927536.0, "num_parameters": 222704}
STORES = ["f32", "bf16", "f16"]


def _dwrfdn(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import DWRFDN
    m = DWRFDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_pair = fuse
    return m


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


# ---- loading and refusals -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _dwrfdn()
    assert len(sd) == 184 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 222704
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert tuple(sd["B2.c1_r.0.0.fn.weight"].shape) == (50, 1, 3, 3) and tuple(sd["B2.c3_r.2.1.weight"].shape) == (50, 50, 1, 1)
    assert tuple(sd["B2.esa.con_.weight"].shape) == (12, 48, 1, 1) and tuple(sd["B2.esa.conv_max.weight"].shape) == (12, 12, 3, 3)
    assert tuple(sd["B2.c4.weight"].shape) == (25, 50, 3, 3) and tuple(sd["c.0.weight"].shape) == (50, 200, 1, 1)
    assert m._leaf("B1.esa.con_").padding == (1, 1) and hasattr(m, "set_scale")
    # conv_max is loaded and counted, never launched
    m._repack("cpu")
    assert not any("conv_max" in str(getattr(o, "w", "")) for o in _plan(m, 1, 32, 32).ops)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import DWRFDN
    for kw in (dict(nf=48), dict(nf=64), dict(upscale=2), dict(num_modules=6), dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            DWRFDN(**kw)
    DWRFDN(in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4)


@pytest.mark.parametrize("store", STORES)
def test_inputs_below_14_pixels_are_refused_with_the_reason(store):
    from ntire2022_esr_amd import _lib as L
    m = _dwrfdn(store, True)
    for h, w in ((13, 40), (40, 13)):
        with pytest.raises(L.EsrError, match="H, W >= 14"):
            _plan(m, 1, h, w)
    _plan(m, 1, 14, 14)
    with pytest.raises(L.EsrError, match="3 input channels"):
        from ntire2022_esr_amd.engine import Plan
        m._build_plan(Plan(1, 20, 20, store), 4)


# ---- complexity and plans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    assert json.load(open(os.path.join(GOLD, "summary_team35_rfdn.json"))) == WANT
    m = _dwrfdn(store, fuse)
    assert model_complexity(m, (3, 256, 256)) == WANT
    # ... and from the plan of that storage and form itself (model_complexity builds an fp32-storage plan)
    plan = _plan(m, 1, 256, 256)
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    assert [float(sum(t[i] for t in terms)) for i in range(3)] == [WANT["flops"], WANT["activations"], float(WANT["num_conv"])]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("nhw", [(1, 14, 17), (2, 45, 70)])
def test_plans_build_and_finalize_in_every_storage_and_both_forms(store, fuse, nhw):
    from ntire2022_esr_amd import _lib as L
    m = _dwrfdn(store, fuse)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    arr, in_idx, out_idx = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [o for o in plan.ops if o.kind == "dwpw"]
    assert len(fused) == (12 if fuse and store != "f32" else 0)            # an fp32 plan has no fused op
    dws = [i for i, o in enumerate(plan.ops) if o.kind == "dw"]
    assert len(dws) == 24 - 2 * len(fused)
    for i in dws:                                                           # every depthwise launch adds its own input before it stores
        d, o = arr[i].conv, plan.ops[i]
        assert arr[i].kind == L.OP_DWCONV and d.res_mode == L.RES_PRE_ACT and (d.res.ptr, d.res.pitch, d.res.coff) == (d.inp.ptr, d.inp.pitch, d.inp.coff)
        assert d.out0.ptr != d.inp.ptr and d.act == L.ACT_NONE and o.res is o.src
    un = [i for i, o in enumerate(plan.ops) if o.kind == "unshuffle"]
    assert len(un) == 4
    n, h, w = nhw
    for i in un:
        e = arr[i].esa
        assert arr[i].kind == L.OP_ESA_UNSHUFFLE == 16 and (e.n, e.h, e.w, e.f) == (n, h, w, 12)
        assert (e.h_lo, e.w_lo) == ((h // 2 - 7) // 3 + 3, (w // 2 - 7) // 3 + 3) and e.storage == L.STORE[store] and e.x.pitch == 16 and e.y.pitch == 16
    ap = [arr[i].esa for i, o in enumerate(plan.ops) if o.kind == "apply"]
    assert len(ap) == 4 and all((e.h_lo, e.w_lo) == (arr[un[0]].esa.h_lo, arr[un[0]].esa.w_lo) and e.c3 == arr[un[0]].esa.y.ptr for e in ap)
    assert len(in_idx) == 1 and len(out_idx) == 1


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_fuse_pair_replaces_exactly_four_ops_twelve_times(store):
    """a 16-bit plan at 2 x 45 x 70: 12 dwpw ops whose descriptors satisfy esr_dwpw_pair_supported; each stands for [dw + x, 1x1 + relu,
    dw + h, 1x1 + x + lrelu] of its path, and the rest of the plan is the per-op plan without those launches"""
    from ntire2022_esr_amd import _lib as L
    m = _dwrfdn(store, True)
    m._repack("cpu")
    plan = _plan(m, 2, 45, 70)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "dwpw"]
    assert len(fused) == 12
    tf = "true" if store == "bf16" else "false"
    costs = m.op_costs(plan, arr)
    paths = [f"B{k}.c{j}_r" for k in range(1, 5) for j in (1, 2, 3)]
    for p, (i, o) in zip(paths, fused):
        assert [(c.kind, c.w) for c in o.replaces] == [("dw", p + ".0.0.fn"), ("conv", p + ".0.1"), ("dw", p + ".2.0.fn"), ("conv", p + ".2.1")]
        d = arr[i].chain
        assert arr[i].kind == L.OP_DWPW_PAIR == 15
        assert L.lib().esr_dwpw_pair_supported(ctypes.byref(d)) == 1
        assert (d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout) == (2, 45, 70, 4, 50, 50, 50)
        assert d.act == L.ACT_LRELU and abs(d.slope - 0.05) < 1e-9 and d.res_mode == L.RES_PRE_ACT
        assert (d.inp.pitch, d.inp.coff) == (56, 0) and (d.post_out.pitch, d.post_out.coff, d.post_cout) == (56, 0, 56)
        assert d.post_out.ptr != d.inp.ptr and all(d.wpacked[l] for l in range(4))
        assert d.wpacked[1] == m._packed[p + ".0.1#dwpw"].data_ptr() and d.wpacked[2] == m._packed[p + ".2.0.fn"].data_ptr()
        assert not d.post_wpacked and not d.post2_wpacked
        assert costs[i]["kernel"] == f"dwpw_pair_kernel<{tf}>" and costs[i]["stored_bytes"] - 4.0 * 2 * (10 * 50 + 2500 + 50) == 2 * 45 * 70 * 224
    per_op = _plan(_dwrfdn(store, False), 2, 45, 70)
    is_path = lambda o: "_r." in str(getattr(o, "w", ""))
    assert [o.w for o in per_op.ops if is_path(o)][:4] == ["B1.c1_r.0.0.fn", "B1.c1_r.0.1", "B1.c1_r.2.0.fn", "B1.c1_r.2.1"]
    assert sum(is_path(o) for o in per_op.ops) == 48 and not any(o.kind == "dwpw" for o in per_op.ops)
    assert [(o.kind, getattr(o, "w", None)) for o in per_op.ops if not is_path(o)] == [(o.kind, getattr(o, "w", None)) for o in plan.ops if o.kind != "dwpw"]
    # ... and only the per-op plan keeps the buffers between those launches
    assert {"t1", "t2"} <= {b.name for b in per_op.buffers} and not {"t1", "t2"} & {b.name for b in plan.buffers}
    assert plan.total < per_op.total


def _views(st):
    """every esr_view inside a ctypes structure, nested structures and arrays included"""
    from ntire2022_esr_amd import _lib as L
    for name, tp in st._fields_:
        v = getattr(st, name)
        if isinstance(v, L.View):
            yield name, v
        elif isinstance(v, ctypes.Structure):
            yield from _views(v)
        elif isinstance(v, ctypes.Array) and len(v) and isinstance(v[0], ctypes.Structure):
            for e in v:
                yield from _views(e)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("nhw", [(1, 14, 17), (2, 45, 70), (32, 256, 256)])
def test_every_view_of_every_op_lies_inside_the_workspace(store, fuse, nhw):
    """the finalized descriptors, not the plan's bookkeeping: every tensor a launch addresses lies inside the bytes the engine allocates --
    full-resolution views inside the plan.total bytes behind the low-resolution arena, c3 (the one low-resolution map) inside that arena --
    also where a fully fused plan has given buffers back"""
    m = _dwrfdn(store, fuse)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    n, h, w = nhw
    base = 1 << 44                                  # (far from every host address a weight blob may have)
    arr, _, _ = plan.finalize((base, plan.total_lo), m._packed)
    h_lo, w_lo = (h // 2 - 7) // 3 + 3, (w // 2 - 7) // 3 + 3
    assert plan.total_lo >= n * h_lo * w_lo * 16 * 4
    es = plan.esize
    seen = 0
    for i, o in enumerate(plan.ops):
        for name, v in _views(arr[i]):
            if not v.ptr:
                continue
            seen += 1
            if o.kind == "unshuffle" and name == "y":
                lo, hi = v.ptr - base, v.ptr - base + n * h_lo * w_lo * v.pitch * 4
                assert 0 <= lo and hi <= plan.total_lo, (i, name, lo, hi)
                continue
            lo, hi = v.ptr - base - plan.total_lo, v.ptr - base - plan.total_lo + n * h * w * v.pitch * es
            assert 0 <= lo and hi <= plan.total, (i, o.kind, getattr(o, "w", None), name, lo, hi, plan.total)
        if o.kind == "apply":                       # c1 and c3 travel as plain pointers
            e = arr[i].esa
            assert 0 <= e.c3 - base and e.c3 - base + n * h_lo * w_lo * 16 * 4 <= plan.total_lo
            assert 0 <= e.c1 - base - plan.total_lo and e.c1 - base - plan.total_lo + n * h * w * 16 * es <= plan.total
    assert seen > 2 * len(plan.ops) - 4
    assert max(b.offset + plan.n * b.h * b.w * b.pitch * b.esize for b in plan.buffers if b.arena == 0) <= plan.total


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_op_kinds_do_not_depend_on_the_batch(store, fuse):
    m = _dwrfdn(store, fuse)
    kinds = [[(o.kind, getattr(o, "w", None)) for o in _plan(m, n, 45, 45).ops] for n in (1, 8)]
    assert kinds[0] == kinds[1]


# ---- unchanged and additive pieces --------------------------------------------------------------------------------------------------------
def test_a_dw_without_res_encodes_byte_for_byte_as_before():
    """`Dw` gained `res` / `res_mode`; with the defaults nothing that exists encodes differently: the esr_op bytes of every depthwise op of
    a BSRN fp32 plan against a descriptor filled the way Dw.encode filled it before the fields existed"""
    from ntire2022_esr_amd import BSRN, _lib as L
    from ntire2022_esr_amd.engine import DWPAD, Buffer, Plan, _view
    m = BSRN(num_in_ch=3, num_feat=48, num_block=5, num_out_ch=3, upscale=4)
    m.fuse_esa_lowres = False                       # the low-resolution depthwise layers as ops of their own too (the `#pad16` blobs)
    m._repack("cpu")
    plan = Plan(1, 32, 40, "f32")
    m._build_plan(plan, 3)
    base = (0x10000000, plan.total_lo)
    arr, _, _ = plan.finalize(base, m._packed)
    dws = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "dw"]
    assert len(dws) == 16 and any(o.hw is not None for _, o in dws) and all(o.res is None and o.res_mode == L.RES_NONE for _, o in dws)
    for i, o in dws:
        old = L.Op()
        old.kind = L.OP_DWCONV
        d = old.conv
        d.n, d.h, d.w = (plan.n,) + ((plan.h, plan.w) if o.hw is None else tuple(o.hw))
        d.cin = d.cout = o.c
        d.ksize = 3
        d.act, d.slope = o.act, o.slope
        d.in_layout = d.out_layout = L.NHWC
        d.inp, d.out0 = _view(o.src, base), _view(o.dst, base)
        d.storage = 0
        w = o.w
        if (o.hw is not None and o.c < 16 and isinstance(o.src, Buffer) and isinstance(o.dst, Buffer) and min(o.src.pitch, o.dst.pitch) >= 16
                and w + DWPAD in m._packed):
            d.cin = d.cout = 16
            w += DWPAD
        d.wpacked = m._packed[w].data_ptr()
        assert bytes(arr[i]) == bytes(old), (i, o.w)
    # the new fields reach the descriptor, and the cost counts a residual that is another tensor than the input
    from ntire2022_esr_amd.engine import Dw
    a, b, c = plan.buffer("a", 56), plan.buffer("b", 56), plan.buffer("c", 56)
    op = L.Op()
    Dw("fea_conv.dw", a, b, 50, res=c, res_mode=L.RES_POST_ACT).encode(op, plan, base, m._packed)
    assert op.conv.res_mode == L.RES_POST_ACT and op.conv.res.ptr == _view(c, base).ptr and op.conv.res.pitch == 56
    rd = lambda **kw: Dw("fea_conv.dw", a, b, 50, **kw).cost(plan, None)["read_bytes"]
    assert rd(res=c, res_mode=L.RES_PRE_ACT) == 2 * rd() and rd(res=a, res_mode=L.RES_PRE_ACT) == rd()


def test_shim_resolves_team35_rfdn():
    code = ("import json; from safetensors.torch import load_file; from models.team35_rfdn.rfdn import RFDN; "
            "m = RFDN(in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; m.set_scale(0); "
            "print(json.dumps([type(m).__module__, RFDN is e.DWRFDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.dwrfdn", True, 222704]


# ---- packers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [12, 16, 1])
def test_con_pack_round_trip(f):
    from ntire2022_esr_amd.engine import pack_unshuffle, unpack_unshuffle
    g = torch.Generator().manual_seed(f)
    w, b = torch.randn(f, 4 * f, 1, 1, generator=g), torch.randn(f, generator=g)
    blob = pack_unshuffle(w, b)
    assert blob.numel() == 4 * f * 16 + 16
    w2, b2 = unpack_unshuffle(blob, f)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    img = blob.reshape(4 * f + 1, 16)
    assert not bool(img[:, f:].any())                                   # pad outputs: zero columns, zero bias
    assert float(img[4 * f - 3, f - 1]) == float(w[f - 1, 4 * f - 3, 0, 0])      # [input channel][output]
    # the model packs exactly this
    m = _dwrfdn()
    m._repack("cpu")
    leaf = m._leaf("B3.esa.con_")
    assert torch.equal(m._packed["B3.esa.con_"], pack_unshuffle(leaf.weight, leaf.bias))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("c", [33, 50, 64])
def test_pointwise_blob_holds_the_weights_rounded_once(store, c):
    """the fused path's 1x1 blobs: MFMA A fragments in natural K order, the weights rounded once to the storage type, the bias fp32, zero
    rows and columns beyond C"""
    from ntire2022_esr_amd.engine import dwpw_pw_effective, pack_dwpw_pw
    dt = torch.bfloat16 if store == "bf16" else torch.float16
    g = torch.Generator().manual_seed(c)
    w, b = torch.randn(c, c, 1, 1, generator=g) * 0.1, torch.randn(c, generator=g)
    blob = pack_dwpw_pw(w, b, store)
    assert blob.numel() * 4 == 8192 + 256
    we, be = dwpw_pw_effective(blob, c, store)
    assert torch.equal(we, w.reshape(c, c).to(dt).double()) and torch.equal(be, b.double())
    full, _ = dwpw_pw_effective(blob, 64, store)
    assert not bool(full[c:].any()) and not bool(full[:, c:].any())
    # fragment (mt, ks), lane l, element j = W[mt * 16 + (l & 15)][ks * 32 + (l >> 4) * 8 + j]
    img = blob.view(torch.uint8)[:8192].view(dt).reshape(4, 2, 64, 8)
    assert float(img[1, 0, 16 * 2 + 3, 5]) == float(w[16 + 3, 0 * 32 + 2 * 8 + 5, 0, 0].to(dt))
    with pytest.raises(Exception):
        pack_dwpw_pw(torch.zeros(65, 65), None, store)


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def _pair_desc(L, a, **kw):
    """the model's own descriptor at 1 x 32 x 40: x and the result in two pitch-56 tensors"""
    d = L.ChainDesc()
    d.n, d.h, d.w, d.n_layers = 1, 32, 40, 4
    d.cin = d.cmid = d.cout = 50
    d.act, d.slope, d.res_mode = L.ACT_LRELU, 0.05, L.RES_PRE_ACT
    d.storage = d.compute = L.STORE["bf16"]
    d.inp = L.View(a, 56, 0)
    for l in range(4):
        d.wpacked[l] = a
    d.post_out, d.post_cout = L.View(a + 4096, 56, 0), 56
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_dwpw_pair_descriptor_validation_without_gpu():
    """esr_dwpw_pair_supported / esr_dwpw_pair_s16 validate before anything is launched: fp32 storage and every shape outside the range are
    ESR_ERR_UNSUPPORTED, null pointers, broken views and a result in x's tensor ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    b = a + 4096
    sup = lambda **kw: lib.esr_dwpw_pair_supported(ctypes.byref(_pair_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_dwpw_pair_s16(ctypes.byref(_pair_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(storage=L.STORE["f16"], compute=L.COMPUTE["f16"]) == 1
    assert sup(cin=33, cmid=33, cout=33, post_cout=40) == 1
    assert sup(cin=64, cmid=64, cout=64, post_cout=64, inp=L.View(a, 64, 0), post_out=L.View(b, 64, 0)) == 1
    assert sup(post_cout=64, post_out=L.View(b, 64, 0)) == 1
    refused = [dict(cin=32, cmid=32, cout=32), dict(cin=65, cmid=65, cout=65), dict(cout=49), dict(cmid=49), dict(cmid=200), dict(act=L.ACT_RELU),
               dict(act=L.ACT_NONE), dict(res_mode=L.RES_NONE), dict(res_mode=L.RES_POST_ACT), dict(res_mode=L.RES_GATE), dict(storage=0, compute=0),
               dict(storage=7, compute=7), dict(compute=L.COMPUTE["f16"]), dict(n_layers=3), dict(n_layers=2), dict(post_wpacked=a), dict(post2_wpacked=a),
               dict(post_cout=48), dict(post_cout=50), dict(post_cout=72), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_dwpw_pair_supported(None) == 0 and lib.esr_dwpw_pair_s16(None, None) == -1
    for kw in (dict(inp=L.View(None, 56, 0)), dict(post_out=L.View(None, 56, 0))):
        assert run(**kw) == -1, kw
    for l in range(4):
        d = _pair_desc(L, a)
        d.wpacked[l] = None
        assert lib.esr_dwpw_pair_s16(ctypes.byref(d), None) == -1, l
    for kw in (dict(inp=L.View(a, 56, 8)), dict(inp=L.View(a, 60, 0)), dict(inp=L.View(a, 48, 0)), dict(inp=L.View(a, 64, 12)),
               dict(post_out=L.View(b, 48, 0)), dict(post_out=L.View(b, 64, 16)), dict(post_out=L.View(b, 60, 0)), dict(post_out=L.View(b, 64, 4)),
               dict(post_out=L.View(a, 112, 56)), dict(inp=L.View(a, 112, 0), post_out=L.View(a, 112, 56))):     # a result in x's tensor: the halo is still being read
        assert run(**kw) == -1, kw
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the LDS opt-in / the launch
        assert run() == -3
        op = L.Op()
        op.kind, op.chain = L.OP_DWPW_PAIR, _pair_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.chain = _pair_desc(L, a, cmid=49)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2


def _un_desc(L, a, **kw):
    d = L.EsaDesc()
    d.n, d.h, d.w, d.f = 1, 32, 40, 12
    d.h_lo, d.w_lo = (32 // 2 - 7) // 3 + 3, (40 // 2 - 7) // 3 + 3
    d.storage = L.STORE["bf16"]
    d.x, d.y = L.View(a, 16, 0), L.View(a + 8192, 16, 0)
    d.w0 = a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_esa_unshuffle_descriptor_validation_without_gpu():
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    run = lambda **kw: lib.esr_esa_unshuffle_f32(ctypes.byref(_un_desc(L, a, **kw)), None)
    assert lib.esr_esa_unshuffle_f32(None, None) == -1
    for kw in (dict(x=L.View(None, 16, 0)), dict(y=L.View(None, 16, 0)), dict(w0=None), dict(f=0), dict(f=17), dict(storage=3), dict(storage=-1),
               dict(n=0), dict(h=0), dict(x=L.View(a, 8, 0)), dict(x=L.View(a, 16, 8)), dict(y=L.View(a + 8192, 12, 0)), dict(y=L.View(a + 8192, 16, 4)),
               dict(y=L.View(a + 8192, 18, 0)), dict(h_lo=5), dict(h_lo=7), dict(w_lo=6), dict(w_lo=8)):
        assert run(**kw) == -1, kw                                                               # ESR_ERR_BAD_ARG
    for kw in (dict(h=13, h_lo=3), dict(w=13, w_lo=3)):
        assert run(**kw) == -4, kw                                                               # ESR_ERR_TOO_SMALL
    if torch.cuda.device_count() == 0:
        # VALID descriptors on a host without a GPU pass every check and fail in the launch: every storage, the minimum size, odd sizes
        assert run() == -3 and run(storage=0) == -3 and run(storage=L.STORE["f16"]) == -3
        assert run(h=14, w=15, h_lo=3, w_lo=3) == -3 and run(h=45, w=70, h_lo=8, w_lo=12) == -3
        op = L.Op()
        op.kind, op.esa = L.OP_ESA_UNSHUFFLE, _un_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
