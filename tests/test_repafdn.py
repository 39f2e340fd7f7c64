"""CPU: RePAFDN (NTIRE 2022 ESR team 10, models.team10_repafdn.repafdn.RePAFDN) on the engine -- checkpoint surface and refusals, complexity
counters in every storage, plan shape (which op kinds, which rides, the gate behind the LR convolution and what it reads and writes), the
gate's weight blob read back, esr_pa_gate's validation without a GPU, and the shim import path."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team10_repafdn.safetensors")
WANT = {"activations": 93815232.0, "num_conv": 59, "flops": 20061696864.0, "num_parameters": 326040}
STORES = ["f32", "bf16", "f16"]


def _repafdn(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import RePAFDN
    m = RePAFDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_pa_tail = fuse
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
    m = _repafdn()
    assert len(sd) == 118 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 326040
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert tuple(sd["B1.c5.weight"].shape) == (48, 72, 1, 1) and tuple(sd["B4.c5.weight"].shape) == (48, 48, 1, 1)
    assert tuple(sd["B2.c4.weight"].shape) == (24, 48, 3, 3) and tuple(sd["B4.c3_d.weight"].shape) == (12, 48, 1, 1)
    assert tuple(sd["pa.conv.weight"].shape) == (48, 48, 1, 1) and tuple(sd["B3.esa.conv_max.weight"].shape) == (12, 12, 3, 3)
    assert "B1.c3_d.weight" not in sd and tuple(sd["c.0.weight"].shape) == (48, 192, 1, 1) and hasattr(m, "set_scale")
    # the unrounded checkpoint: the same keys across its two files, and the fixture is its RNE rounding to bf16
    true = {}
    for part in ("_f32.safetensors", "_f32.part2.safetensors"):
        p = os.path.join(GOLD, "team10_repafdn" + part)
        assert os.path.getsize(p) <= 1 << 20
        true.update(load_file(p))
    assert set(true) == set(sd) and all(v.dtype == torch.float32 for v in true.values())
    assert all(torch.equal(true[k].to(torch.bfloat16).view(torch.int16), sd[k].view(torch.int16)) for k in sd)
    m.load_state_dict(true, strict=True)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import RePAFDN
    for kw in (dict(nf=50), dict(nf=64), dict(upscale=2), dict(act_type="silu"), dict(act_type="relu"), dict(ds_rate=0.5), dict(dc=32), dict(dc=12),
               dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            RePAFDN(**kw)
    RePAFDN(in_nc=3, nf=48, out_nc=3, upscale=4, act_type="lrelu", ds_rate=0.25, rgb_range=1.0, dc=24)


@pytest.mark.parametrize("store", STORES)
def test_inputs_below_15_pixels_are_refused_with_the_reason(store):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    m = _repafdn(store)
    for h, w in ((14, 40), (40, 14)):
        with pytest.raises(L.EsrError, match="H, W >= 15"):
            _plan(m, 1, h, w)
    _plan(m, 1, 15, 15)
    with pytest.raises(L.EsrError, match="3 input channels"):
        m._build_plan(Plan(1, 20, 20, store), 4)


# ---- complexity and plans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    assert json.load(open(os.path.join(GOLD, "summary_team10_repafdn.json"))) == WANT
    m = _repafdn(store, fuse)
    assert model_complexity(m, (3, 256, 256)) == WANT
    # ... and from the plan of that storage itself (model_complexity builds an fp32-storage plan)
    plan = _plan(m, 1, 256, 256)
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    assert [float(sum(t[i] for t in terms)) for i in range(3)] == [WANT["flops"], WANT["activations"], float(WANT["num_conv"])]


def _names(plan):
    """every weight a plan launches, riding 1x1s included"""
    out = []
    for o in plan.ops:
        for c in (o.replaces if hasattr(o, "replaces") else [o]):
            if c.kind in ("conv", "pagate"):
                out.append(c.w.replace("#head", ""))
                p = getattr(c, "post", None)
                if p is not None:
                    out.append(p.w)
            elif c.kind == "apply":
                out += [c.wf, c.w4] + [p.w for p in c.post or ()]
            elif c.kind == "s2":
                out.append(c.w)
    return out


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("nhw", [(1, 15, 15), (2, 45, 70), (32, 256, 256)], ids=lambda s: "x".join(str(v) for v in s))
def test_plan_shape(store, nhw):
    """every convolution of the reference graph exactly once, in every storage; the 16-bit plans take rfdn.py's rides where dc = 24 and none of
    the distillation rides in B4 (dc = 12); the gate stands between the LR convolution and the upsampler and never writes what it reads"""
    from ntire2022_esr_amd import _lib as L
    m = _repafdn(store)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    arr, in_idx, out_idx = plan.finalize((0x10000000, plan.total_lo), m._packed)
    want = ["fea_conv"] + [f"B{k}.{n}" for k in range(1, 5) for n in
                           ([f"c{j}_{t}" for j in range(1, 3 if k < 4 else 4) for t in "dr"] + ["c4", "c5"] +
                            ["esa." + e for e in ("conv1", "conv_f", "conv_max", "conv2", "conv3", "conv3_", "conv4")])] + \
        ["c.0", "LR_conv", "pa.conv", "upsampler.0"]
    assert sorted(_names(plan)) == sorted(want) and len(want) == 59
    kinds = [o.kind for o in plan.ops]
    assert kinds.count("pagate") == 1 and kinds.count("apply") == 4 and kinds.count("lowres") == 4
    assert kinds[-3:] == ["conv", "pagate", "conv"] and [plan.ops[i].w for i in (-3, -2, -1)] == ["LR_conv", "pa.conv", "upsampler.0"]
    assert len(plan.ops) == (43 if store == "f32" else 34) and kinds.count("pack") == (0 if store == "f32" else 1)
    riders = {p.w for o in plan.ops if o.kind == "conv" and o.post is not None for p in [o.post]} | \
             {p.w for o in plan.ops if o.kind == "apply" for p in o.post or ()}
    if store == "f32":
        assert not riders
    else:
        assert riders == {"B1.c1_d", "B2.c1_d", "B3.c1_d"} | {f"B{k}.c2_d" for k in (1, 2, 3)} | {f"B{k}.esa.conv1" for k in (1, 2, 3, 4)}
    # the gate's descriptor
    i = len(plan.ops) - 2
    d, o = arr[i].conv, plan.ops[i]
    lr, up = arr[i - 1].conv, arr[i + 1].conv
    assert arr[i].kind == L.OP_PA_GATE == 17 and L.lib().esr_pa_gate_supported(ctypes.byref(d)) == 1
    assert (d.n, d.h, d.w, d.cin, d.cout, d.ksize) == nhw + (48, 48, 1) and d.storage == d.compute == L.STORE[store]
    assert d.res_mode == L.RES_POST_ACT and d.act == L.ACT_NONE and (d.inp.pitch, d.out0.pitch, d.res.pitch) == (48, 48, 48)
    assert d.inp.ptr == lr.out0.ptr and d.out0.ptr == up.inp.ptr and d.res.ptr == arr[in_idx[0] if store == "f32" else 1].conv.out0.ptr
    assert d.wpacked == m._packed["pa.conv#pag"].data_ptr()
    ptrs = {d.inp.ptr, d.res.ptr, d.out0.ptr}
    if store == "bf16":                     # the long skip as hi + lo pairs: fea is read as one, out_lr written as one, the upsampler reads it
        assert d.hilo == (L.HILO_RES | L.HILO_OUT) and d.hilo_stride == (nhw[0] * nhw[1] * nhw[2] * 48 * 2 + 255) // 256 * 256 and up.hilo == L.HILO_IN and lr.hilo == 0
        ptrs |= {d.res.ptr + d.hilo_stride, d.out0.ptr + d.hilo_stride}
        assert len(ptrs) == 5
        m.hilo_skip = False
        assert not any(getattr(q, "hilo", 0) for q in _plan(m, *nhw).ops)
    else:
        assert d.hilo == 0 and len(ptrs) == 3
    cost = m.op_costs(plan, arr)[i]
    npix = nhw[0] * nhw[1] * nhw[2]
    pairs = 2 if store == "bf16" else 1
    assert cost["kernel"] == f"pa_gate_kernel<{L.STORE[store]}>" and cost["flops"] == 2.0 * npix * 48 * 48
    assert cost["read_bytes"] == npix * plan.esize * 48 * (1 + pairs) + 4.0 * (48 * 48 + 48) and cost["write_bytes"] == npix * plan.esize * 48 * pairs


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_fuse_pa_tail_replaces_exactly_the_lr_conv_and_the_gate(store):
    """a 16-bit plan at 2 x 45 x 70 with the flag on: ONE patail op whose descriptor satisfies esr_pa_tail_supported; it stands for [LR_conv,
    pa.conv], reads what LR_conv read and writes what the gate wrote, and the rest of the plan is the per-op plan without those two; an
    fp32 plan has no fused op whatever the flag says; the flag is off by default"""
    from ntire2022_esr_amd import RePAFDN, _lib as L
    assert RePAFDN().fuse_pa_tail is False
    m = _repafdn(store, True)
    m._repack("cpu")
    plan = _plan(m, 2, 45, 70)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    per_op = _plan(_repafdn(store, False), 2, 45, 70)
    ref, _, _ = per_op.finalize((0x10000000, per_op.total_lo), m._packed)
    fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "patail"]
    assert len(fused) == 1 and len(plan.ops) == len(per_op.ops) - 1 and plan.total == per_op.total
    i, o = fused[0]
    assert [(c.kind, c.w) for c in o.replaces] == [("conv", "LR_conv"), ("pagate", "pa.conv")]
    key = lambda q: (q.kind, getattr(q, "w", None))
    assert [key(q) for q in plan.ops if q.kind != "patail"] == [key(q) for q in per_op.ops if key(q) not in (("conv", "LR_conv"), ("pagate", "pa.conv"))]
    assert [key(q) for q in per_op.ops][i:i + 2] == [("conv", "LR_conv"), ("pagate", "pa.conv")]
    d, lr, g = arr[i].conv, ref[i].conv, ref[i + 1].conv
    assert arr[i].kind == L.OP_PA_TAIL == 18 and L.lib().esr_pa_tail_supported(ctypes.byref(d)) == 1
    assert (d.n, d.h, d.w, d.cin, d.cout, d.ksize) == (2, 45, 70, 48, 48, 3) and d.storage == d.compute == L.STORE[store]
    assert (d.inp.ptr, d.inp.pitch, d.inp.coff) == (lr.inp.ptr, 48, 0) and d.wpacked == lr.wpacked == m._packed["LR_conv#s16"].data_ptr()
    assert d.tail_wpacked == g.wpacked == m._packed["pa.conv#pag"].data_ptr() and not d.tail_cat.ptr and d.tail_cat_c == 0
    assert (d.out0.ptr, d.res.ptr, d.res_mode, d.hilo, d.hilo_stride) == (g.out0.ptr, g.res.ptr, L.RES_POST_ACT, g.hilo, g.hilo_stride)
    assert d.out0.ptr != d.inp.ptr and d.res.ptr != d.out0.ptr and d.hilo == ((L.HILO_RES | L.HILO_OUT) if store == "bf16" else 0)
    cost = m.op_costs(plan, arr)[i]
    npix, pairs = 2 * 45 * 70, 2 if store == "bf16" else 1
    assert cost["kernel"] == f"pa_tail_kernel<{'true' if store == 'bf16' else 'false'}, 3>" and cost["flops"] == 2.0 * npix * 48 * 48 * 10
    assert cost["read_bytes"] == npix * 2 * 48 * (1 + pairs) + 4.0 * (48 * 48 + 48) + 4.0 * (9 * 48 * 48 + 48) and cost["write_bytes"] == npix * 2 * 48 * pairs
    f32 = _repafdn("f32", True)
    assert not any(q.kind == "patail" for q in _plan(f32, 2, 45, 70).ops)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_op_kinds_do_not_depend_on_the_batch(store, fuse):
    m = _repafdn(store, fuse)
    kinds = [[(o.kind, getattr(o, "w", None), getattr(getattr(o, "post", None), "w", None) if o.kind == "conv" else None) for o in _plan(m, n, 45, 45).ops]
             for n in (1, 8)]
    assert kinds[0] == kinds[1]


def _views(st):
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
@pytest.mark.parametrize("nhw", [(1, 15, 15), (2, 45, 70)], ids=lambda s: "x".join(str(v) for v in s))
def test_every_full_resolution_view_lies_inside_the_workspace(store, nhw):
    """the finalized descriptors: every full-resolution tensor a launch addresses -- the low parts of the gate's pairs included -- lies
    inside the plan.total bytes behind the low-resolution arena"""
    from ntire2022_esr_amd import _lib as L
    m = _repafdn(store)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    n, h, w = nhw
    base = 1 << 44
    arr, _, _ = plan.finalize((base, plan.total_lo), m._packed)
    seen = 0
    for i, o in enumerate(plan.ops):
        if o.kind == "lowres" or getattr(o, "hw", None) is not None:
            continue
        for name, v in _views(arr[i].conv if o.kind in ("conv", "pagate", "pack") else arr[i].esa):
            if not v.ptr or v.ptr < base:           # (the network input / output are not workspace views)
                continue
            seen += 1
            bit = {"inp": L.HILO_IN, "res": L.HILO_RES, "out0": L.HILO_OUT}.get(name, 0) if o.kind in ("conv", "pagate") else 0
            hl = arr[i].conv.hilo_stride if (bit and arr[i].conv.hilo & bit) else 0          # a hi + lo pair: the low parts behind the view
            lo, hi = v.ptr - base - plan.total_lo, v.ptr - base - plan.total_lo + n * h * w * v.pitch * plan.esize
            assert 0 <= lo and hi + hl <= plan.total, (i, o.kind, getattr(o, "w", None), name, lo, hi, hl, plan.total)
    assert seen > len(plan.ops)


# ---- the gate's blob ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("c", [33, 48, 64])
def test_gate_blob_round_trip(store, c):
    """pack, then read the effective weights back: fp32 -- the weights themselves; 16-bit -- hi + lo, hi the weight rounded to the storage
    type and lo the rounded remainder; the bias fp32; zero rows and columns beyond C; and the documented fragment order"""
    from ntire2022_esr_amd.engine import pa_gate_effective, pack_pa_gate
    g = torch.Generator().manual_seed(c)
    w, b = torch.randn(c, c, 1, 1, generator=g) * 0.3, torch.randn(c, generator=g)
    blob = pack_pa_gate(w, b, store)
    assert blob.numel() * 4 == 16384 + 256
    we, be = pa_gate_effective(blob, c, store)
    w2 = w.reshape(c, c)
    if store == "f32":
        assert torch.equal(we, w2.double())
        img = blob[:4096].reshape(4, 16, 64)          # (mt, step 4 j + i, lane 16 kq + row) = W[16 mt + row][16 j + 4 kq + i]
        assert float(img[1, 4 * 0 + 2, 16 * 3 + 5]) == float(w2[16 + 5, 0 + 12 + 2])
    else:
        dt = torch.bfloat16 if store == "bf16" else torch.float16
        hi = w2.to(dt).float()
        lo = (w2 - hi).to(dt).float()
        assert torch.equal(we, hi.double() + lo.double())
        assert float((we - w2.double()).abs().max()) <= float(w2.abs().max()) * (2.0 ** -16 if store == "bf16" else 2.0 ** -21)
        img = blob.view(torch.uint8)[:16384].view(dt).reshape(2, 4, 2, 64, 8)     # (hi | lo, mt, ks, lane, e) = W[16 mt + row][16 (2 ks + e / 4) + 4 kq + e % 4]
        assert float(img[0, 1, 1, 16 * 2 + 3, 5]) == float(hi[16 + 3, 16 * 3 + 8 + 1]) if c > 57 else True
        assert float(img[0, 2, 0, 16 * 1 + 0, 6]) == float(hi[32 + 0, 16 * 1 + 4 + 2]) and float(img[1, 2, 0, 16 * 1 + 0, 6]) == float(lo[32, 22])
    assert torch.equal(be, b.double())
    full, bfull = pa_gate_effective(blob, 64, store)
    assert not bool(full[c:].any()) and not bool(full[:, c:].any()) and not bool(bfull[c:].any())
    for bad in (torch.zeros(65, 65), torch.zeros(48, 40)):
        with pytest.raises(Exception):
            pack_pa_gate(bad, None, store)
    # the model packs exactly this
    if c == 48:
        m = _repafdn(store)
        m._repack("cpu")
        leaf = m._leaf("pa.conv")
        assert torch.equal(m._packed["pa.conv#pag"], pack_pa_gate(leaf.weight, leaf.bias, store))


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
S = 1 << 20     # bytes between the stand-in tensors of the descriptors below: more than one of them holds (1 x 32 x 40 x 96 x 4 at most)


def _gate_desc(L, a, store="bf16", **kw):
    """the model's own descriptor at 1 x 32 x 40: t, s and y in three pitch-48 tensors S bytes apart (addresses only: nothing below reads
    or writes them -- every descriptor here is refused before a launch, or run where no GPU exists)"""
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 32, 40, 48, 48, 1
    d.in_layout = d.out_layout = L.NHWC
    d.res_mode = L.RES_POST_ACT
    d.storage = d.compute = L.STORE[store]
    d.inp, d.res, d.out0 = L.View(a, 48, 0), L.View(a + S, 48, 0), L.View(a + 2 * S, 48, 0)
    d.wpacked = a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pa_gate_descriptor_validation_without_gpu():
    """esr_pa_gate_supported / esr_pa_gate validate before anything is launched: every shape and feature outside the range is
    ESR_ERR_UNSUPPORTED; null pointers, broken views and a result in t's or s's tensor are ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 8192)()
    a = ctypes.addressof(buf)
    sup = lambda **kw: lib.esr_pa_gate_supported(ctypes.byref(_gate_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_pa_gate(ctypes.byref(_gate_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(store="f16") == 1 and sup(store="f32") == 1 and sup(res_mode=L.RES_NONE) == 1
    assert sup(cin=33, cout=40) == 1 and sup(store="f32", cin=33, cout=36) == 1 and sup(cin=64, cout=64) == 1 and sup(cin=50, cout=64) == 1
    assert sup(hilo=L.HILO_RES, hilo_stride=4096) == 1 and sup(hilo=L.HILO_OUT | L.HILO_RES, hilo_stride=4096, store="f16") == 1
    refused = [dict(cin=32, cout=32), dict(cin=65, cout=72), dict(cout=40), dict(cout=52), dict(cout=72), dict(store="f32", cout=50), dict(ksize=3),
               dict(act=L.ACT_LRELU), dict(act=L.ACT_RELU), dict(res_mode=L.RES_PRE_ACT), dict(res_mode=L.RES_GATE), dict(storage=7, compute=7),
               dict(compute=L.COMPUTE["f16"]), dict(compute=0), dict(in_layout=L.NCHW_IN), dict(out_layout=L.NCHW_SHUFFLE4), dict(split=16),
               dict(tail_wpacked=a), dict(tail_cat=L.View(a, 32, 0)), dict(tail_cat_c=32), dict(post_wpacked=a), dict(post2_wpacked=a), dict(border_bias=a), dict(blocked8=1), dict(in_seg_stride=64),
               dict(wino_wpacked=a), dict(hilo=L.HILO_IN, hilo_stride=4096), dict(hilo=L.HILO_OUT), dict(hilo=L.HILO_OUT, hilo_stride=24),
               dict(hilo=L.HILO_OUT, hilo_stride=-16), dict(store="f32", hilo=L.HILO_OUT, hilo_stride=4096),
               dict(hilo=L.HILO_RES, hilo_stride=4096, res_mode=L.RES_NONE), dict(n=0), dict(h=0), dict(w=-1), dict(h=65536, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_pa_gate_supported(None) == 0 and lib.esr_pa_gate(None, None) == -1
    bad = [dict(inp=L.View(None, 48, 0)), dict(out0=L.View(None, 48, 0)), dict(res=L.View(None, 48, 0)), dict(wpacked=None),
           dict(inp=L.View(a, 48, 8)), dict(inp=L.View(a, 44, 0)), dict(inp=L.View(a, 64, 12)), dict(res=L.View(a + S, 40, 0)),
           dict(res=L.View(a + S, 64, 24)), dict(out0=L.View(a + 2 * S, 40, 0)), dict(out0=L.View(a + 2 * S, 64, 20)), dict(out0=L.View(a + 2 * S, 64, 24)),
           dict(store="f32", inp=L.View(a, 48, 2)), dict(store="f32", out0=L.View(a + 2 * S, 50, 0)),
           dict(out0=L.View(a, 96, 48)), dict(out0=L.View(a + S, 96, 48)),                       # a result in t's / s's tensor
           dict(hilo=L.HILO_OUT, hilo_stride=S, out0=L.View(a + 2 * S, 48, 0), inp=L.View(a + 3 * S, 48, 0)),   # y's low parts where t is
           dict(hilo=L.HILO_RES, hilo_stride=S),                                                # s's low parts where y is
           dict(out0=L.View(a + 16, 48, 0)), dict(out0=L.View(a + S - 4096, 48, 0)), dict(out0=L.View(a + S + 122880 - 16, 48, 0)),   # y's bytes meet t's / s's
           dict(inp=L.View(a + 2 * S + 64, 64, 0))]
    for kw in bad:
        assert run(**kw) == -1, kw                                                               # ESR_ERR_BAD_ARG
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the launch
        assert run() == -3 and run(store="f32") == -3 and run(res_mode=L.RES_NONE) == -3
        op = L.Op()
        op.kind, op.conv = L.OP_PA_GATE, _gate_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.conv = _gate_desc(L, a, cin=32, cout=32)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2


def test_pa_tail_descriptor_validation_without_gpu():
    """esr_pa_tail_supported / esr_pa_tail: the gate's descriptor with ksize 3, 16-bit storage only, two blobs"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 8192)()
    a = ctypes.addressof(buf)
    tail = lambda **kw: _gate_desc(L, a, **{**dict(ksize=3, tail_wpacked=a), **kw})
    sup = lambda **kw: lib.esr_pa_tail_supported(ctypes.byref(tail(**kw)))
    run = lambda **kw: lib.esr_pa_tail(ctypes.byref(tail(**kw)), None)
    assert sup() == 1 and sup(store="f16") == 1 and sup(res_mode=L.RES_NONE) == 1 and sup(cin=33, cout=40) == 1 and sup(cin=64, cout=64) == 1
    assert sup(hilo=L.HILO_RES, hilo_stride=4096) == 1 and sup(hilo=L.HILO_OUT | L.HILO_RES, hilo_stride=4096, store="f16") == 1
    refused = [dict(store="f32"), dict(ksize=1), dict(cin=32, cout=32), dict(cin=65, cout=72), dict(cout=40), dict(cout=52), dict(cout=64),
               dict(act=L.ACT_LRELU), dict(res_mode=L.RES_PRE_ACT), dict(res_mode=L.RES_GATE), dict(compute=L.COMPUTE["f16"]), dict(compute=0),
               dict(in_layout=L.NCHW_IN), dict(out_layout=L.NCHW_SHUFFLE4), dict(split=16), dict(tail_cat=L.View(a, 32, 0)), dict(tail_cat_c=32),
               dict(post_wpacked=a), dict(post2_wpacked=a), dict(border_bias=a), dict(blocked8=1), dict(in_seg_stride=64), dict(wino_wpacked=a),
               dict(hilo=L.HILO_IN, hilo_stride=4096), dict(hilo=L.HILO_OUT), dict(hilo=L.HILO_OUT, hilo_stride=24),
               dict(hilo=L.HILO_RES, hilo_stride=4096, res_mode=L.RES_NONE), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_pa_tail_supported(None) == 0 and lib.esr_pa_tail(None, None) == -1
    bad = [dict(inp=L.View(None, 48, 0)), dict(out0=L.View(None, 48, 0)), dict(res=L.View(None, 48, 0)), dict(wpacked=None), dict(tail_wpacked=None),
           dict(inp=L.View(a, 48, 8)), dict(inp=L.View(a, 44, 0)), dict(res=L.View(a + S, 40, 0)), dict(out0=L.View(a + 2 * S, 40, 0)),
           dict(out0=L.View(a + 2 * S, 64, 20)), dict(out0=L.View(a, 96, 48)), dict(out0=L.View(a + S, 96, 48)),      # a result in x's / s's tensor
           dict(hilo=L.HILO_RES, hilo_stride=S),                                                                       # s's low parts where y is
           dict(out0=L.View(a + 16, 48, 0)), dict(out0=L.View(a + S + 122880 - 16, 48, 0)), dict(inp=L.View(a + 2 * S + 64, 64, 0))]   # y's bytes meet x's / s's
    for kw in bad:
        assert run(**kw) == -1, kw                                                               # ESR_ERR_BAD_ARG
    if torch.cuda.device_count() == 0:
        assert run() == -3 and run(cin=64, cout=64, inp=L.View(a, 64, 0), res=L.View(a + S, 64, 0), out0=L.View(a + 2 * S, 64, 0)) == -3
        op = L.Op()
        op.kind, op.conv = L.OP_PA_TAIL, tail()
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.conv = tail(store="f32")
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2


# ---- the shim, and everything else unchanged ------------------------------------------------------------------------------------------------
def test_shim_resolves_team10_repafdn():
    code = ("import json; from safetensors.torch import load_file; from models.team10_repafdn.repafdn import RePAFDN; "
            "m = RePAFDN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, RePAFDN is e.RePAFDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.repafdn", True, 326040]
