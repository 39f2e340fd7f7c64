"""CPU: FMEN (NTIRE 2022 ESR team 03, team03_fmen.py) on the engine -- checkpoint surface, complexity counters, plan shape with and without the
fused HFAB, the shim import path, and the C ABI's ESR_RES_GATE validation (esr_conv_chain_supported's HFAB form, esr_conv2d_f32's gate rules)."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team03_fmen.safetensors")


def _fmen():
    from safetensors.torch import load_file
    from ntire2022_esr_amd import FMEN
    m = FMEN()
    m.load_state_dict(load_file(CKPT), strict=True)
    return m


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _fmen()
    assert len(sd) == 68 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 341066
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())


def test_model_complexity_equals_the_reference_model_summary():
    from ntire2022_esr_amd.summary import model_complexity
    want = json.load(open(os.path.join(GOLD, "summary_team03_fmen.json")))
    assert model_complexity(_fmen(), (3, 256, 256)) == want


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [True, False])
def test_plan_shape_with_and_without_the_fused_hfab(store, fuse):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    from ntire2022_esr_amd.summary import model_complexity
    m = _fmen()
    m.fuse_hfab = fuse
    plan = Plan(2, 40, 36, store)
    if store == "f16":
        # the checkpoint's HFAB activations (up to ~2e7) do not fit fp16: no fp16 plan, an error instead of Inf / NaN outputs
        with pytest.raises(L.EsrError, match="fp16"):
            m._build_plan(plan, 3)
        return
    m._build_plan(plan, 3)
    chains = [o for o in plan.ops if o.kind == "chain"]
    s16 = store != "f32"
    # f32: 34 convs; 16-bit: + the input pack; fused: each body HFAB's four convs are one op
    assert len(plan.ops) == 34 + s16 - (12 if (s16 and fuse) else 0)
    if s16:                                   # bf16: the long skip x and lr_conv's output as hi + lo pairs
        assert [(o.w, o.hilo) for o in plan.ops if o.kind == "conv" and o.hilo] == [
            ("head#head", L.HILO_OUT), ("lr_conv", L.HILO_RES | L.HILO_OUT), ("tail.0", L.HILO_IN)]
    assert len(chains) == (4 if (s16 and fuse) else 0)
    for i, o in enumerate(chains):
        assert o.gate and [s.w for s in o.replaces] == [f"hfabs.{i}.squeeze", f"hfabs.{i}.convs.0.conv1.rep_conv",
                                                                  f"hfabs.{i}.convs.0.conv2.rep_conv", f"hfabs.{i}.excitate"]
        assert o.replaces[-1].res_mode == L.RES_GATE and o.replaces[0].slope == 0.1
    gates = [o for o in plan.ops if o.kind == "conv" and o.res_mode == L.RES_GATE]
    assert len(gates) == (1 if (s16 and fuse) else 5)                 # the warmup HFAB stays on per-layer launches
    nf_bufs = {b.pitch for b in plan.buffers if b.name in ("x.0", "x", "ha", "hb")}
    assert nf_bufs == {56}                                            # tight pitch in 16-bit, whole fp32 chunks (56) in fp32
    # the complexity counters see the reference's 34 convolutions whichever way the plan runs them
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    ref = model_complexity(m, (3, 40, 36))
    assert (float(sum(t[0] for t in terms)) / 2, int(sum(t[2] for t in terms))) == (ref["flops"], ref["num_conv"])
    if s16 and fuse:
        m.compute = store
        m._repack("cpu")
        arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
        costs = m.op_costs(plan, arr)
        hf = [c for c in costs if c["kernel"].startswith("hfab_kernel")]
        assert len(hf) == 4 and all(c["kernel"] == f"hfab_kernel<{'true' if store == 'bf16' else 'false'}, 4>" for c in hf)
        npix = 2 * 40 * 36
        assert hf[0]["read_bytes"] == npix * 50 * 2 + 4.0 * 9 * (50 * 16 + 2 * 16 * 16 + 16 * 50)
        assert hf[0]["write_bytes"] == npix * 50 * 2
        assert hf[0]["stored_bytes"] == npix * 2 * (56 + 56) + 4.0 * 9 * (50 * 16 + 2 * 16 * 16 + 16 * 50)
        for i, o in enumerate(plan.ops):
            if o.kind == "chain":
                d = arr[i].chain
                assert (d.n_layers, d.cin, d.cmid, d.cout, d.res_mode, d.post_cout) == (4, 50, 16, 50, L.RES_GATE, 56)
                assert not d.post_wpacked and abs(d.slope - 0.1) < 1e-7


def test_fuse_hfab_is_a_plan_switch():
    m = _fmen()
    assert not m.fuse_hfab                    # off by default: slower than the per-layer launches at batch 32 (FMEN)
    m._dirty = False
    m.fuse_hfab = True
    assert m.fuse_hfab and m._dirty


def test_shim_resolves_team03_fmen():
    code = ("import json; from safetensors.torch import load_file; from models.team03_fmen import FMEN; m = FMEN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, FMEN is e.FMEN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.fmen", True, 341066]


def _chain_desc(L, a, **kw):
    d = L.ChainDesc()
    d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout = 1, 32, 40, 4, 50, 16, 50
    d.act, d.slope, d.res_mode = L.ACT_LRELU, 0.1, L.RES_GATE
    d.storage = d.compute = L.STORE["bf16"]
    d.inp, d.post_out = L.View(a, 56, 0), L.View(a, 56, 0)
    for i in range(4):
        d.wpacked[i] = a
    d.post_cout = 56
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_hfab_chain_descriptor_validation():
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    sup = lambda **kw: lib.esr_conv_chain_supported(ctypes.byref(_chain_desc(L, a, **kw)))
    assert sup() == 1
    assert sup(storage=L.STORE["f16"], compute=L.STORE["f16"]) == 1
    assert sup(cmid=12) == 1 and sup(cin=48, cout=48, post_cout=48) == 1
    assert sup(n_layers=6) == 0                                    # the warmup HFAB: per-layer launches
    assert sup(cmid=32) == 0
    assert sup(act=L.ACT_GELU) == 0
    assert sup(post_wpacked=a) == 0                                # GATE writes post_out itself: no post 1x1
    assert sup(post2_wpacked=a) == 0
    assert sup(cin=50, cout=48) == 0 and sup(cin=32, cout=32, post_cout=32) == 0
    assert sup(storage=0, compute=0) == 0
    assert sup(post_cout=40) == 0                                  # fewer channels than cout
    assert lib.esr_conv_chain_s16(ctypes.byref(_chain_desc(L, a, post_out=L.View(None, 56, 0))), None) == -1
    assert lib.esr_conv_chain_s16(ctypes.byref(_chain_desc(L, a, inp=L.View(a, 56, 8))), None) == -1      # 50 channels would leave the pixel
    assert lib.esr_conv_chain_s16(ctypes.byref(_chain_desc(L, a, post_out=L.View(a, 48, 0))), None) == -1  # 56 stored channels > pitch 48
    assert lib.esr_conv_chain_s16(ctypes.byref(_chain_desc(L, a, cmid=32)), None) == -2
    # the RLFB form is unchanged
    d = _chain_desc(L, a, n_layers=3, cin=46, cmid=48, cout=46, res_mode=L.RES_POST_ACT, slope=0.05, post_wpacked=a, post2_wpacked=a,
                    post_cout=46, post2_cout=16)
    d.inp, d.post_out, d.post2_out = L.View(a, 48, 0), L.View(a, 48, 0), L.View(a, 16, 0)
    assert lib.esr_conv_chain_supported(ctypes.byref(d)) == 1


def test_gate_descriptor_validation_without_gpu():
    """esr_conv2d_f32 with ESR_RES_GATE: an activation, a fused tail / post chain or the pixel-shuffle output are UNSUPPORTED (returned before any
    launch); the Winograd kernel never takes a gate"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)

    def desc(**kw):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 16, 16, 16, 48, 3
        d.in_layout, d.out_layout, d.res_mode = L.NHWC, L.NHWC, L.RES_GATE
        d.inp, d.res, d.out0 = L.View(a, 16, 0), L.View(a, 48, 0), L.View(a, 48, 0)
        d.wpacked = a
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    for store in ("f32", "bf16", "f16"):
        st = dict(storage=L.STORE[store], compute=L.COMPUTE[store])
        assert lib.esr_conv2d_f32(ctypes.byref(desc(act=L.ACT_LRELU, slope=0.1, **st)), None) == -2
        assert lib.esr_conv2d_f32(ctypes.byref(desc(act=L.ACT_RELU, **st)), None) == -2
        assert lib.esr_conv2d_f32(ctypes.byref(desc(post_wpacked=a, post_out=L.View(a, 16, 0), post_cout=16, **st)), None) == -2
        assert lib.esr_conv2d_f32(ctypes.byref(desc(out_layout=L.NCHW_SHUFFLE4, **st)), None) == -2
    assert lib.esr_wino_supported(ctypes.byref(desc(cin=48, inp=L.View(a, 48, 0)))) == 0
    assert lib.esr_wino_supported(ctypes.byref(desc(cin=48, inp=L.View(a, 48, 0), res_mode=L.RES_PRE_ACT))) == 1
