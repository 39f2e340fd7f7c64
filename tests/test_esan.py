"""CPU: ESAN (NTIRE 2022 ESR team 34, models.team34_esan.ESAN at level 1) on the engine -- checkpoint surface, refusals, plan shape in both forms
of the residual-block head, complexity counters in every storage and both forms, the shim import path, a torch restatement of the forward
against the reference's e2e golden, and the C ABI's validation of esr_resblock_head_s16 without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team34_esan.safetensors")


def _esan(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import ESAN
    m = ESAN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_head = fuse
    return m


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _esan()
    assert len(sd) == 262 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 358256
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert "upconv0.weight" in sd and "conv_first.0.bias" in sd and "upconv.0.weight" in sd and "recon_trunk.0.15.ESA.conv3_3.weight" in sd
    assert tuple(sd["recon_trunk.0.7.conv2.weight"].shape) == (32, 32, 3, 3) and tuple(sd["recon_trunk.0.0.ESA.conv1.weight"].shape) == (8, 32, 1, 1)


def test_unsupported_arguments_and_small_inputs_are_refused():
    from ntire2022_esr_amd import ESAN, _lib as L
    for kw in (dict(level=0), dict(level=2), dict(nf=64), dict(nf=40), dict(upscale=2)):
        with pytest.raises(NotImplementedError):
            ESAN(**kw)
    for store, fuse in (("f32", False), ("f16", True)):
        m = _esan(store, fuse)
        for h, w in ((14, 20), (20, 14)):
            with pytest.raises(L.EsrError, match="H, W >= 15"):
                _plan(m, 1, h, w)
        _plan(m, 1, 15, 15)


def test_plan_structure():
    from ntire2022_esr_amd import _lib as L
    is_add = lambda o: o.kind == "conv" and o.w == "ident"
    per_op, fused = _plan(_esan("f16", False), 1, 45, 70), _plan(_esan("f16", True), 1, 45, 70)
    assert sum(map(is_add, per_op.ops)) == 16 and not any(o.kind == "reshead" for o in per_op.ops)
    assert [o.kind for o in fused.ops].count("reshead") == 16 and sum(map(is_add, fused.ops)) == 1
    # the fused plan: the first block's head replaces three launches, the others' four; nothing else changes
    assert len(per_op.ops) - len(fused.ops) == 2 + 15 * 3
    assert {o.kind for o in fused.ops} == {"pack", "conv", "reshead", "lowres", "apply"}
    rest = [o for o in per_op.ops if not (o.kind == "conv" and o.w.endswith((".conv1", ".conv2")))]
    rest = [o for i, o in enumerate(rest) if not (is_add(o) and i < len(rest) - 2)]          # (the last add stays: the output convolution follows it)
    assert [(o.kind, getattr(o, "w", None)) for o in rest] == [(o.kind, getattr(o, "w", None)) for o in fused.ops if o.kind != "reshead"]
    heads = [o for o in fused.ops if o.kind == "reshead"]
    assert len(heads[0].replaces) == 3 and all(len(o.replaces) == 4 for o in heads[1:])
    for k, o in enumerate(heads):
        assert [c.w for c in o.replaces[-3:]] == [f"recon_trunk.0.{k}.{s}" for s in ("conv1", "conv2", "ESA.conv1")]
    # x is never stored over the x or the g it is made from
    for o in heads[1:]:
        add = o.replaces[0]
        assert add.dst is not add.res and add.dst is not add.src
    # an fp32 plan never fuses
    f32a, f32b = _plan(_esan("f32", False), 1, 45, 70), _plan(_esan("f32", True), 1, 45, 70)
    assert [o.kind for o in f32a.ops] == [o.kind for o in f32b.ops] and not any(o.kind == "reshead" for o in f32b.ops)
    # the op list encodes (fake device addresses: no GPU needed) and names the kernel with every template argument
    for store in ("bf16", "f16"):
        m = _esan(store, True)
        m._repack("cpu")
        plan = _plan(m, 2, 45, 70)
        arr, in_idx, out_idx = plan.finalize((0x10000000, plan.total_lo), m._packed)
        assert len(in_idx) == 1 and len(out_idx) == 1
        tf = "true" if store == "bf16" else "false"
        j = 0
        for i, (o, c) in enumerate(zip(plan.ops, m.op_costs(plan, arr))):
            if o.kind != "reshead":
                continue
            d = arr[i].conv
            assert arr[i].kind == L.OP_RESBLOCK_HEAD and (d.n, d.h, d.w, d.cin, d.cout, d.ksize) == (2, 45, 70, 32, 32, 3)
            assert d.res_mode == (L.RES_PRE_ACT if j else L.RES_NONE) and d.act == L.ACT_RELU
            assert (d.inp.pitch, d.out1.pitch, d.post_out.pitch, d.post_cout) == (32, 32, 16, 16)
            assert bool(d.out0.ptr) == bool(j) and d.out0.ptr != d.inp.ptr
            assert c["kernel"] == f"resblock_head_kernel<{tf}, {'true' if j else 'false'}>"
            j += 1
        assert j == 16


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("n", [1, 8])
def test_plan_choice_does_not_depend_on_the_batch(store, fuse, n):
    kinds = lambda p: [(o.kind, getattr(o, "w", None)) for o in p.ops]
    m = _esan(store, fuse)
    assert kinds(_plan(m, n, 45, 70)) == kinds(_plan(m, 1, 45, 70))


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    want = json.load(open(os.path.join(GOLD, "summary_team34_esan.json")))
    assert want["num_conv"] == 131 and want["num_parameters"] == 358256
    m = _esan(store, fuse)
    assert model_complexity(m, (3, 256, 256)) == want
    # ... and over the plan of THIS storage and form (model_complexity counts on an fp32 plan)
    plan = _plan(m, 1, 256, 256)
    assert any(o.kind == "reshead" for o in plan.ops) == (fuse and store != "f32")
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    got = {"activations": float(sum(t[1] for t in terms)), "num_conv": sum(t[2] for t in terms), "flops": float(sum(t[0] for t in terms)),
           "num_parameters": want["num_parameters"]}
    assert got == want


def test_shim_resolves_team34_esan():
    code = ("import json; from safetensors.torch import load_file; from models.team34_esan import ESAN, make_model; m = make_model(1); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, ESAN is e.ESAN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.esan", True, 358256]


def _restated_forward(sd, x):
    """the network as this project states it (esan.py's docstring), in fp64 torch ops on the checkpoint"""
    p = {k: v.double() for k, v in sd.items()}
    conv = lambda name, v, **kw: F.conv2d(v, p[name + ".weight"], p[name + ".bias"], **kw)
    x = x.double()
    t = conv("conv_first.0", x, padding=1)
    for k in range(16):
        b = f"recon_trunk.0.{k}."
        u = conv(b + "conv2", F.relu(conv(b + "conv1", t, padding=1)), padding=1)
        c1 = conv(b + "ESA.conv1", u)
        c3 = F.max_pool2d(conv(b + "ESA.conv2", c1, stride=2), 7, 3)
        c3 = F.relu(conv(b + "ESA.conv3_1", c3, padding=1))
        c3 = F.relu(conv(b + "ESA.conv3_2", c3, padding=1))
        c3 = conv(b + "ESA.conv3_3", c3, padding=1)
        c3 = F.interpolate(c3, u.shape[2:], mode="bilinear", align_corners=False)
        t = t + u * torch.sigmoid(conv(b + "ESA.conv4", c3 + c1))
    # the sum in the 48-channel domain, as ONE 3x3 over [trunk | x_in] with the folded weights and the summed bias
    w = torch.cat([p["upconv.0.weight"], p["upconv0.weight"]], 1)
    return F.pixel_shuffle(F.conv2d(torch.cat([t, x], 1), w, p["upconv.0.bias"] + p["upconv0.bias"], padding=1), 4)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_restated_forward_matches_the_reference_golden(case):
    from safetensors.torch import load_file
    g = np.load(os.path.join(GOLD, "e2e_team34_esan.npz"))
    y = _restated_forward(load_file(CKPT), torch.from_numpy(g["x" + case])).numpy()
    ref = g["yd_s3"] if case == "d" else g["y" + case]
    y = y[:, :, ::3, ::3] if case == "d" else y
    assert y.shape == ref.shape
    assert float(np.abs(y - ref).max()) <= 2e-5 * max(float(g["data_range"]), float(np.abs(ref).max()))


def _head_desc(L, a, **kw):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 32, 40, 32, 32, 3
    d.act, d.res_mode = L.ACT_RELU, L.RES_PRE_ACT
    d.storage = d.compute = L.STORE["f16"]
    d.inp, d.res, d.out0, d.out1 = L.View(a, 32, 0), L.View(a + 64, 32, 0), L.View(a + 128, 32, 0), L.View(a + 192, 32, 0)
    d.post_out, d.post_cout = L.View(a, 16, 0), 16
    d.wpacked = d.tail_wpacked = d.post_wpacked = a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_resblock_head_descriptor_validation_without_gpu():
    """esr_resblock_head_supported / esr_resblock_head_s16 validate before anything is launched: fp32 storage and shapes outside the predicate
    are ESR_ERR_UNSUPPORTED (never something approximate), null pointers, broken views and an x stored over its sources ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 256)()
    a = ctypes.addressof(buf)
    sup = lambda **kw: lib.esr_resblock_head_supported(ctypes.byref(_head_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_resblock_head_s16(ctypes.byref(_head_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(storage=L.STORE["bf16"], compute=L.COMPUTE["bf16"]) == 1 and sup(res_mode=L.RES_NONE) == 1 and sup(post_cout=8) == 1
    refused = [dict(storage=0, compute=0), dict(compute=L.COMPUTE["bf16"]), dict(cin=33), dict(cin=16), dict(cout=33), dict(cout=48), dict(ksize=1),
               dict(act=L.ACT_NONE), dict(act=L.ACT_LRELU), dict(res_mode=L.RES_POST_ACT), dict(res_mode=L.RES_GATE), dict(post_cout=0),
               dict(post_cout=17), dict(post_act=L.ACT_RELU), dict(post2_wpacked=a), dict(border_bias=a),
               dict(hilo=L.HILO_OUT), dict(out_layout=L.NCHW_SHUFFLE4), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_resblock_head_supported(None) == 0 and lib.esr_resblock_head_s16(None, None) == -1
    for kw in (dict(inp=L.View(None, 32, 0)), dict(res=L.View(None, 32, 0)), dict(out0=L.View(None, 32, 0)), dict(out1=L.View(None, 32, 0)),
               dict(post_out=L.View(None, 16, 0)), dict(wpacked=None), dict(tail_wpacked=None), dict(post_wpacked=None),
               dict(inp=L.View(a, 32, 8)), dict(inp=L.View(a, 36, 0)), dict(res=L.View(a + 64, 40, 12)), dict(out0=L.View(a + 128, 24, 0)),
               dict(out1=L.View(a + 192, 48, 24)), dict(post_out=L.View(a, 8, 0)), dict(post_out=L.View(a, 16, 4)),
               dict(out0=L.View(a, 32, 0)), dict(out0=L.View(a + 64, 32, 0)), dict(out1=L.View(a, 32, 0))):          # x over xin, x over g, u over xin
        assert run(**kw) == -1, kw
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the LDS opt-in / the launch
        assert run() == -3 and run(res_mode=L.RES_NONE) == -3
        # ... through the op list as well: ESR_OP_RESBLOCK_HEAD dispatches to the same launcher
        op = L.Op()
        op.kind, op.conv = L.OP_RESBLOCK_HEAD, _head_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.conv = _head_desc(L, a, cin=33)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2
