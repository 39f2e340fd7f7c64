"""CPU: BMDN (NTIRE 2022 ESR team 37, models.team37_bmdn.BMDN) on the engine -- checkpoint surface, complexity counters in both forms of the
distillation step and every storage, plan shape, the folded 3x3 blob of the one-launch step, the shim import path, and the C ABI's validation
of esr_distill_step_s16 without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team37_bmdn.safetensors")


def _bmdn(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import BMDN
    m = BMDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_step = fuse
    return m


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _bmdn()
    assert len(sd) == 152 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 193088
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert "B3.c2_b.weight" in sd and "B1.esa.conv3_.weight" in sd and "c.0.weight" in sd
    assert tuple(sd["B2.c1_r.weight"].shape) == (20, 40, 3, 3) and tuple(sd["B2.c2_r.weight"].shape) == (20, 20, 3, 3)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import BMDN
    for kw in (dict(upscale=2), dict(nf=80), dict(num_modules=6), dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            BMDN(**kw)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    want = json.load(open(os.path.join(GOLD, "summary_team37_bmdn.json")))
    assert want == {"activations": 90500128.0, "num_conv": 76, "flops": 11726033040.0, "num_parameters": 193088}
    assert model_complexity(_bmdn(store, fuse), (3, 256, 256)) == want


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
def test_plan_shape(store):
    from ntire2022_esr_amd import _lib as L
    s16 = store != "f32"
    per_op, fused = _plan(_bmdn(store, False), 2, 339, 510), _plan(_bmdn(store, True), 2, 339, 510)
    # per block: 3 steps of 3 launches, c4, c5 (16-bit: + esa.conv1 in its epilogue), the ESA branch, the apply; head (+ the 16-bit input
    # pack), c.0, LR_conv, upsampler
    assert len(per_op.ops) == 4 + s16 + 4 * (9 + 1 + (1 if s16 else 2) + 1 + 1)
    assert not any(o.kind == "distill" for o in per_op.ops)
    if not s16:                                   # an fp32 plan has the per-op form only
        assert [o.kind for o in fused.ops] == [o.kind for o in per_op.ops]
        return
    # the fused plan: exactly 6 launches fewer per block, none of them a pack or a copy
    assert len(per_op.ops) - len(fused.ops) == 4 * 6
    assert [o.kind for o in fused.ops].count("distill") == 12 and [o.kind for o in fused.ops].count("pack") == 1
    assert {o.kind for o in fused.ops} == {"pack", "conv", "distill", "lowres", "apply"}
    rest = [o for o in per_op.ops if not (o.kind == "conv" and o.w.split(".")[-1][:1] == "c" and o.w.split(".")[-1][2:] in ("_d", "_r", "_b"))]
    assert [(o.kind, getattr(o, "w", None)) for o in rest] == [(o.kind, getattr(o, "w", None)) for o in fused.ops if o.kind != "distill"]
    for o in fused.ops:
        if o.kind == "distill":
            cd, cb, cr = o.replaces
            assert (cd.w[-4:], cb.w[-4:], cr.w[-4:]) == (cd.w[-4:-1] + "d", cd.w[-4:-1] + "b", cd.w[-4:-1] + "r")
            assert (cd.cin, cd.cout, cr.cout) in ((40, 20, 20), (20, 20, 20)) and (cb.res is None) == (cd.cin == 40)
    # no torch.cat: c5 and c.0 read the planar concats through their cin_map
    c5 = [o for o in fused.ops if o.kind == "conv" and o.w.endswith(".c5")]
    assert len(c5) == 4 and all(o.cin == 128 and o.cin_alg == 80 and o.post is not None for o in c5)
    # the op list encodes (fake device addresses: no GPU needed) and names the kernel with every template argument
    m = _bmdn(store, True)
    m._repack("cpu")
    arr, _, _ = fused.finalize((0x10000000, fused.total_lo), m._packed)
    tf = "true" if store == "bf16" else "false"
    steps = [(arr[i].chain, c) for i, (o, c) in enumerate(zip(fused.ops, m.op_costs(fused, arr))) if o.kind == "distill"]
    assert all(arr[i].kind == L.OP_DISTILL_STEP for i, o in enumerate(fused.ops) if o.kind == "distill")
    for j, (d, c) in enumerate(steps):
        first = j % 3 == 0
        assert (d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout) == (2, 339, 510, 2, 40 if first else 20, 20, 20)
        assert d.res_mode == (L.RES_NONE if first else L.RES_PRE_ACT) and d.act == L.ACT_RELU
        assert (d.inp.pitch, d.post_out.pitch, d.post_cout, d.post2_out.pitch, d.post2_cout) == (40 if first else 32, 32, 32, 32, 32)
        assert c["kernel"] == f"distill_step_kernel<{tf}, {3 if first else 2}, {'false' if first else 'true'}>"
    if store == "bf16":                           # the long skip as hi + lo pairs
        assert [(o.w, o.hilo) for o in fused.ops if o.kind == "conv" and o.hilo] == [
            ("fea_conv#head", L.HILO_OUT), ("LR_conv", L.HILO_RES | L.HILO_OUT), ("upsampler.0", L.HILO_IN)]


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("hw", [128, 256])
def test_kernel_choice_does_not_depend_on_the_batch(store, fuse, hw):
    """the PLAN's choice: which ops it emits, what rides in whose launch, which kernel family runs them.  (Inside esr_conv2d_f32 the existing
    launchers still size a block -- NW = 4 or 8 waves of the same kernel -- by the grid, hence by n; that is theirs, predates BMDN and does
    not change a result: test_gpu_bmdn.py::test_batch_equals_per_image is bit-exact.  The wave count is therefore left out of the names.)"""
    import re
    m = _bmdn(store, fuse)
    m._repack("cpu")
    names = []
    for n in (1, 8):
        plan = _plan(m, n, hw, hw)
        arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
        names.append([(o.kind, getattr(o, "w", None), getattr(o, "post", None) is not None, re.sub(r",NW=\d", "", c["kernel"]))
                      for o, c in zip(plan.ops, m.op_costs(plan, arr))])
    assert names[0] == names[1]
    assert sum(k[0] == "distill" for k in names[0]) == (12 if fuse and store != "f32" else 0)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("cin", [40, 20])
def test_folded_blob_rows(store, cin):
    """pack_distill_s16: unpacked over ALL physical K slots, the image holds cat([W_r, W_b], 1) at slots [0, cin) and
    [round_up(cin, 16), + 20) -- the [in chunks | d chunks] order --, zeros in the pad rows, and the bias b_r + b_b"""
    from ntire2022_esr_amd.engine import distill_cin_map, pack_conv_s16, pack_distill_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(cin)
    w_r, b_r = torch.randn(20, cin, 3, 3, generator=g), torch.randn(20, generator=g)
    w_b, b_b = torch.randn(20, 20, 3, 3, generator=g), torch.randn(20, generator=g)
    blob = pack_distill_s16(w_r, b_r, w_b, b_b, store)
    ci = (cin + 15) // 16 * 16
    phys = ci + 32
    cmap = distill_cin_map(cin, 20)
    assert len(cmap) == phys and cmap[:cin] == list(range(cin)) and cmap[ci:ci + 20] == list(range(cin, cin + 20))
    assert all(v == -1 for v in cmap[cin:ci] + cmap[ci + 20:])
    w, b = unpack_conv_s16(blob, phys, 20, 3, store, cin_phys=phys)          # identity map: one row per physical slot
    assert torch.equal(b, b_r + b_b)
    assert not w[:, cin:ci].any() and not w[:, ci + 20:].any()
    # the taps are rounded to the storage type with error diffusion over the nine taps: within one step of the fold, the filter sums closer
    eps = 2.0 ** -8 if store == "bf16" else 2.0 ** -11
    fold = torch.cat([w_r, w_b], 1)
    got = torch.cat([w[:, :cin], w[:, ci:ci + 20]], 1)
    assert float((got - fold).abs().max()) <= 2 * eps * float(fold.abs().max())
    assert float((got.sum((2, 3)) - fold.sum((2, 3))).abs().max()) <= eps * float(fold.abs().max())
    # the same image as packing the fold through the map by hand
    assert torch.equal(blob, pack_conv_s16(fold, b_r + b_b, store, cin_map=cmap))
    # the model's blob is this fold of its own parameters
    m = _bmdn(store, True)
    m._repack("cpu")
    j = 1 if cin == 40 else 2
    want = pack_distill_s16(m.B2._modules[f"c{j}_r"].weight, m.B2._modules[f"c{j}_r"].bias, m.B2._modules[f"c{j}_b"].weight, m.B2._modules[f"c{j}_b"].bias, store)
    assert torch.equal(m._packed[f"B2.c{j}_r#fold"], want)


def test_small_inputs_are_refused():
    from ntire2022_esr_amd import _lib as L
    for store, fuse in (("f32", False), ("bf16", True)):
        m = _bmdn(store, fuse)
        for h, w in ((14, 20), (20, 14)):
            with pytest.raises(L.EsrError, match="H, W >= 15"):
                _plan(m, 1, h, w)
        _plan(m, 1, 15, 15)


def test_shim_resolves_team37_bmdn():
    code = ("import json; from safetensors.torch import load_file; from models.team37_bmdn import BMDN; m = BMDN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, BMDN is e.BMDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.bmdn", True, 193088]


def _step_desc(L, a, **kw):
    d = L.ChainDesc()
    d.n, d.h, d.w, d.n_layers = 1, 32, 40, 2
    d.cin, d.cmid, d.cout = 40, 20, 20
    d.act, d.res_mode = L.ACT_RELU, L.RES_NONE
    d.storage = d.compute = L.STORE["bf16"]
    d.inp = L.View(a, 40, 0)
    d.wpacked[0], d.wpacked[1] = a, a
    d.post_out, d.post_cout = L.View(a, 32, 0), 20
    d.post2_out, d.post2_cout = L.View(a, 32, 0), 32
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_distill_step_descriptor_validation_without_gpu():
    """esr_distill_step_supported / esr_distill_step_s16 validate before anything is launched: fp32 storage and shapes outside the
    predicate are ESR_ERR_UNSUPPORTED (never something approximate), null pointers and broken views ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    sup = lambda **kw: lib.esr_distill_step_supported(ctypes.byref(_step_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_distill_step_s16(ctypes.byref(_step_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(storage=L.STORE["f16"], compute=L.COMPUTE["f16"]) == 1
    assert sup(cin=20, res_mode=L.RES_PRE_ACT, inp=L.View(a, 32, 0)) == 1 and sup(cin=20) == 1 and sup(cin=48, inp=L.View(a, 48, 0)) == 1
    refused = [dict(storage=0, compute=0), dict(compute=L.COMPUTE["f16"]), dict(cin=16), dict(cin=49), dict(cmid=16), dict(cmid=33),
               dict(cout=16), dict(cout=33), dict(n_layers=3), dict(act=L.ACT_LRELU), dict(act=L.ACT_NONE), dict(res_mode=L.RES_POST_ACT),
               dict(res_mode=L.RES_GATE), dict(res_mode=L.RES_PRE_ACT), dict(post_wpacked=a), dict(post2_wpacked=a), dict(post_cout=19),
               dict(post_cout=33), dict(post2_cout=19), dict(post2_cout=40), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_distill_step_supported(None) == 0 and lib.esr_distill_step_s16(None, None) == -1
    for kw in (dict(inp=L.View(None, 40, 0)), dict(post_out=L.View(None, 32, 0)), dict(post2_out=L.View(None, 32, 0))):
        assert run(**kw) == -1, kw
    d = _step_desc(L, a)
    d.wpacked[1] = None
    assert lib.esr_distill_step_s16(ctypes.byref(d), None) == -1
    for kw in (dict(inp=L.View(a, 40, 8)), dict(inp=L.View(a, 44, 0)), dict(inp=L.View(a, 48, 4)),          # 40 channels leave the pixel; granule
               dict(post_out=L.View(a, 16, 0)), dict(post_out=L.View(a, 32, 16)), dict(post_out=L.View(a, 36, 0)),
               dict(post2_out=L.View(a, 24, 0)), dict(post2_out=L.View(a, 32, 8))):
        assert run(**kw) == -1, kw
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the LDS opt-in / the launch
        assert run() == -3
        # ... through the op list as well: ESR_OP_DISTILL_STEP dispatches to the same launcher
        op = L.Op()
        op.kind, op.chain = L.OP_DISTILL_STEP, _step_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.chain = _step_desc(L, a, cin=49)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2
