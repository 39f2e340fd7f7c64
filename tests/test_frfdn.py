"""CPU: FasterRFDN (NTIRE 2022 ESR team 25, models.team25_frfdn.FRFDN.FasterRFDN) on the engine -- checkpoint surface, complexity counters in
both forms of the refinement path and every storage, plan shape, the shim import path, and the C ABI's validation of esr_refine_cascade_s16
without a GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team25_frfdn.safetensors")


def _frfdn(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import FasterRFDN
    m = FasterRFDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_cascade = fuse
    return m


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _frfdn()
    assert len(sd) == 128 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 376432
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert "B3.c3_d.weight" in sd and "B1.esa.conv3_.weight" in sd and "c.0.weight" in sd
    assert tuple(sd["B2.c2_r.weight"].shape) == (32, 32, 3, 3) and tuple(sd["B2.c3_d.weight"].shape) == (16, 32, 1, 1)
    assert tuple(sd["B2.c4.weight"].shape) == (16, 16, 3, 3) and tuple(sd["B2.c5.weight"].shape) == (64, 96, 1, 1)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import FasterRFDN
    for kw in (dict(upscale=2), dict(nf=50), dict(nf=48), dict(num_modules=6), dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            FasterRFDN(**kw)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    want = json.load(open(os.path.join(GOLD, "summary_team25_frfdn.json")))
    assert want == {"activations": 113552640.0, "num_conv": 64, "flops": 22379010176.0, "num_parameters": 376432}
    assert model_complexity(_frfdn(store, fuse), (3, 256, 256)) == want


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


def test_logical_channel_counts_of_the_concat_convs():
    """c5 sees the 96 channels of cat(d1, d2, d3, r4), c.0 the 256 of the four block outputs, in every storage and both forms"""
    for store, fuse in (("f32", False), ("bf16", False), ("bf16", True), ("f16", True)):
        m = _frfdn(store, fuse)
        plan = _plan(m, 1, 32, 32)
        c5 = [m._counted_convs(plan, o)[0] for o in plan.ops if o.kind == "conv" and o.w.endswith(".c5")]
        c0 = [m._counted_convs(plan, o) for o in plan.ops if o.kind == "conv" and o.w == "c.0"]
        assert len(c5) == 4 and all(c[:3] == (96, 64, 1) for c in c5)
        assert c0 == [[(256, 64, 1, plan.npix, 1)]]


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_fused_plan_holds_four_cascade_ops_the_kernel_accepts(store):
    """a 16-bit plan at 2 x 45 x 70, finalized against a fake workspace: 4 cascade ops whose descriptors satisfy esr_refine_cascade_supported
    and stand for [c2_r, c3_d, c3_r, c4] of their block; d3 and r4 are the two halves of the third concat segment"""
    from ntire2022_esr_amd import _lib as L
    m = _frfdn(store, True)
    m._repack("cpu")
    plan = _plan(m, 2, 45, 70)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "cascade"]
    assert len(fused) == 4
    tf = "true" if store == "bf16" else "false"
    costs = m.op_costs(plan, arr)
    for k, (i, o) in enumerate(fused, 1):
        assert [c.w for c in o.replaces] == [f"B{k}.c2_r", f"B{k}.c3_d", f"B{k}.c3_r", f"B{k}.c4"]
        d = arr[i].chain
        assert arr[i].kind == L.OP_REFINE_CASCADE == 12
        assert L.lib().esr_refine_cascade_supported(ctypes.byref(d)) == 1
        assert (d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout) == (2, 45, 70, 4, 32, 16, 16)
        assert d.act == L.ACT_LRELU and abs(d.slope - 0.05) < 1e-9 and d.res_mode == L.RES_PRE_ACT
        assert (d.inp.pitch, d.inp.coff) == (32, 0)
        assert (d.post_out.pitch, d.post_out.coff, d.post_cout) == (32, 0, 16) and (d.post2_out.pitch, d.post2_out.coff, d.post2_cout) == (32, 16, 16)
        assert d.post_out.ptr == d.post2_out.ptr and d.post_out.ptr != d.inp.ptr
        assert all(d.wpacked[l] for l in range(4)) and not d.post_wpacked and not d.post2_wpacked
        assert costs[i]["kernel"] == f"refine_cascade_kernel<{tf}>"
    # the rest of the plan is the per-op plan without those sixteen convolutions
    per_op = _plan(_frfdn(store, False), 2, 45, 70)
    assert len(per_op.ops) - len(plan.ops) == 4 * 3 and not any(o.kind == "cascade" for o in per_op.ops)
    gone = re.compile(r"B\d\.(c2_r|c3_d|c3_r|c4)$")
    rest = [(o.kind, getattr(o, "w", None)) for o in per_op.ops if not (o.kind == "conv" and gone.match(o.w))]
    assert rest == [(o.kind, getattr(o, "w", None)) for o in plan.ops if o.kind != "cascade"]
    # c5 reads the three dense segments through an identity map: 96 physical = 96 logical channels, esa.conv1 in its epilogue
    c5 = [o for o in plan.ops if o.kind == "conv" and o.w.endswith(".c5")]
    assert len(c5) == 4 and all(o.cin == 96 and o.cin_alg == 96 and o.post is not None and len(o.src.segs) == 3 and o.src.pitch == 32 for o in c5)
    if store == "bf16":                           # the long skip as hi + lo pairs
        assert [(o.w, o.hilo) for o in plan.ops if o.kind == "conv" and o.hilo] == [
            ("fea_conv#head", L.HILO_OUT), ("LR_conv", L.HILO_RES | L.HILO_OUT), ("upsampler.0", L.HILO_IN)]


@pytest.mark.parametrize("store,fuse", [("f32", True), ("f32", False), ("bf16", False), ("f16", False)])
def test_no_cascade_op_in_fp32_plans_or_with_the_flag_off(store, fuse):
    m = _frfdn(store, fuse)
    m._repack("cpu")
    plan = _plan(m, 2, 45, 70)
    plan.finalize((0x10000000, plan.total_lo), m._packed)
    assert not any(o.kind == "cascade" for o in plan.ops)
    names = [o.w for o in plan.ops if o.kind == "conv"]
    assert all(f"B{k}.{c}" in names for k in range(1, 5) for c in ("c2_r", "c3_d", "c3_r", "c4"))
    if store == "f32":                            # one 96-wide concat buffer: d3 and r4 at channels 64 and 80
        c4 = next(o for o in plan.ops if o.kind == "conv" and o.w == "B1.c4")
        assert c4.dst[0].pitch == 96 and c4.dst[1:] == (80, 16)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("hw", [45, 128])
def test_op_kinds_do_not_depend_on_the_batch(store, fuse, hw):
    m = _frfdn(store, fuse)
    m._repack("cpu")
    names = []
    for n in (1, 8):
        plan = _plan(m, n, hw, hw)
        arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
        # (the kernel label of a plain conv is left out: inside esr_conv2d_f32 the existing launchers size a block -- 4 or 8 waves -- by the
        # grid, hence by n, and the label's POST suffix follows the wave count; that predates this network and changes no result)
        names.append([(o.kind, getattr(o, "w", None), getattr(o, "post", None) is not None, c["kernel"] if o.kind == "cascade" else None)
                      for o, c in zip(plan.ops, m.op_costs(plan, arr))])
    assert names[0] == names[1]
    assert sum(k[0] == "cascade" for k in names[0]) == (4 if fuse and store != "f32" else 0)


def test_small_inputs_are_refused():
    from ntire2022_esr_amd import _lib as L
    for store, fuse in (("f32", False), ("bf16", True)):
        m = _frfdn(store, fuse)
        for h, w in ((14, 20), (20, 14)):
            with pytest.raises(L.EsrError, match="H, W >= 15"):
                _plan(m, 1, h, w)
        _plan(m, 1, 15, 15)


def test_shim_resolves_team25_frfdn():
    code = ("import json; from safetensors.torch import load_file; from models.team25_frfdn.FRFDN import FasterRFDN; m = FasterRFDN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, FasterRFDN is e.FasterRFDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.frfdn", True, 376432]


def _casc_desc(L, a, **kw):
    """the model's own descriptor at 1 x 32 x 40: d2 a dense pitch-32 tensor, d3 and r4 the halves of another"""
    d = L.ChainDesc()
    d.n, d.h, d.w, d.n_layers = 1, 32, 40, 4
    d.cin, d.cmid, d.cout = 32, 16, 16
    d.act, d.slope, d.res_mode = L.ACT_LRELU, 0.05, L.RES_PRE_ACT
    d.storage = d.compute = L.STORE["bf16"]
    d.inp = L.View(a, 32, 0)
    for l in range(4):
        d.wpacked[l] = a
    d.post_out, d.post_cout = L.View(a + 4096, 32, 0), 16
    d.post2_out, d.post2_cout = L.View(a + 4096, 32, 16), 16
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_refine_cascade_descriptor_validation_without_gpu():
    """esr_refine_cascade_supported / esr_refine_cascade_s16 validate before anything is launched: fp32 storage and every shape but the
    model's are ESR_ERR_UNSUPPORTED (never something approximate), null pointers, broken views and an output in d2's tensor ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    b = a + 4096
    sup = lambda **kw: lib.esr_refine_cascade_supported(ctypes.byref(_casc_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_refine_cascade_s16(ctypes.byref(_casc_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(storage=L.STORE["f16"], compute=L.COMPUTE["f16"]) == 1
    assert sup(inp=L.View(a, 64, 32)) == 1 and sup(post_out=L.View(b, 16, 0), post2_out=L.View(b + 8192, 16, 0)) == 1
    refused = [dict(cin=31), dict(cin=33), dict(cmid=15), dict(cmid=17), dict(cout=15), dict(cout=17), dict(act=L.ACT_RELU), dict(act=L.ACT_NONE),
               dict(res_mode=L.RES_NONE), dict(res_mode=L.RES_POST_ACT), dict(res_mode=L.RES_GATE), dict(storage=0, compute=0),
               dict(compute=L.COMPUTE["f16"]), dict(n_layers=3), dict(n_layers=2), dict(post_wpacked=a), dict(post2_wpacked=a),
               dict(post_cout=8), dict(post_cout=32), dict(post2_cout=8), dict(post2_cout=32), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_refine_cascade_supported(None) == 0 and lib.esr_refine_cascade_s16(None, None) == -1
    for kw in (dict(inp=L.View(None, 32, 0)), dict(post_out=L.View(None, 32, 0)), dict(post2_out=L.View(None, 32, 16))):
        assert run(**kw) == -1, kw
    for l in range(4):
        d = _casc_desc(L, a)
        d.wpacked[l] = None
        assert lib.esr_refine_cascade_s16(ctypes.byref(d), None) == -1, l
    for kw in (dict(inp=L.View(a, 32, 8)), dict(inp=L.View(a, 36, 0)), dict(inp=L.View(a, 48, 20)), dict(inp=L.View(a, 24, 0)),      # 32 channels leave the pixel; granule
               dict(post_out=L.View(b, 8, 0)), dict(post_out=L.View(b, 32, 24)), dict(post_out=L.View(b, 36, 0)), dict(post_out=L.View(b, 32, 4)),
               dict(post2_out=L.View(b, 32, 20)), dict(post2_out=L.View(b, 24, 16)),
               dict(post_out=L.View(a, 64, 32)), dict(post2_out=L.View(a, 64, 48))):                # an output in d2's tensor: the halo is still being read
        assert run(**kw) == -1, kw
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the LDS opt-in / the launch
        assert run() == -3
        # ... through the op list as well: ESR_OP_REFINE_CASCADE dispatches to the same launcher
        op = L.Op()
        op.kind, op.chain = L.OP_REFINE_CASCADE, _casc_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.chain = _casc_desc(L, a, cin=33)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2
