"""CPU: EFDN (NTIRE 2022 ESR team 05, models.team05_efdn.plainsr.PLAINRFDN) on the engine -- checkpoint surface, complexity counters, plan shape
per storage and fuse_esa_lowres setting, the shim import path, and the C ABI's validation of the stride-7 ESA branch (esr_esa_lowres_f32 with
w_s2 = NULL, esr_maxpool7s7_f32) without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team05_efdn.safetensors")


def _efdn():
    from safetensors.torch import load_file
    from ntire2022_esr_amd import PLAINRFDN
    m = PLAINRFDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    return m


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _efdn()
    assert len(sd) == 118 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 272038
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert "B3.c2_r.conv3x3.weight" in sd and "B1.esa.conv_23.weight" in sd and "c.0.weight" not in sd


def test_model_complexity_equals_the_reference_model_summary():
    from ntire2022_esr_amd.summary import model_complexity
    want = json.load(open(os.path.join(GOLD, "summary_team05_efdn.json")))
    assert want == {"activations": 79585152.0, "num_conv": 59, "flops": 16859552000.0, "num_parameters": 272038}
    assert model_complexity(_efdn(), (3, 256, 256)) == want


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [True, False])
def test_plan_shape(store, fuse):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    from ntire2022_esr_amd.summary import model_complexity
    m = _efdn()
    m.fuse_esa_lowres = fuse
    plan = Plan(2, 339, 510, store)
    m._build_plan(plan, 3)
    s16 = store != "f32"
    kinds = [o.kind for o in plan.ops]
    names = [getattr(o, "w", None) for o in plan.ops]
    assert "c.0" not in names and not any(n and n.endswith("c.0") for n in names)
    lows = [o for o in plan.ops if o.kind == "lowres"]
    if fuse:                                  # one low-resolution op per block, pooled from the conv1 map (no stride-2 conv)
        assert len(lows) == 4 and "pool7" not in kinds
        for k, o in enumerate(lows, 1):
            assert o.w is None and (o.dst.h, o.dst.w) == (48, 73) and (o.pooled.h, o.pooled.w) == (48, 73)
            assert [(ly.kind, ly.act, ly.w, ly.w_dw) for ly in o.layers] == [
                (2, L.ACT_RELU, f"B{k}.esa.conv_2", f"B{k}.esa.conv_3"), (3, L.ACT_NONE, f"B{k}.esa.conv_23", None)]
            assert [r.kind for r in o.replaces] == ["pool7", "conv", "conv", "conv"]
    else:
        assert not lows and kinds.count("pool7") == 4
        for o in plan.ops:
            if o.kind == "conv" and o.hw is not None:
                assert o.hw == (48, 73) and o.w.split(".")[-1] in ("conv_2", "conv_3", "conv_23")
    # per block: c1_d (16-bit blocks 2..4: in the previous ESA apply), c1_r, c2_d, c2_r, c3_d, c3_r, c4, c5 (16-bit: + esa.conv1 in its epilogue),
    # the branch (1 or 4 ops), the apply; head (+ the 16-bit input pack), LR_conv, upsampler
    per_block = 8 + (0 if s16 else 1) + (1 if fuse else 4) + 1
    assert len(plan.ops) == 3 + s16 + 4 * per_block - (3 if s16 else 0)
    applies = [o for o in plan.ops if o.kind == "apply"]
    assert [bool(o.post) for o in applies] == ([True, True, True, False] if s16 else [False] * 4)
    c5 = [o for o in plan.ops if o.kind == "conv" and o.w.endswith(".c5")]
    assert all((o.post is not None) == s16 for o in c5) and all(o.cin == 64 and o.cin_alg == 40 for o in c5)
    nf_bufs = {b.pitch for b in plan.buffers if b.name in ("fea", "fea.0", "r1", "r2", "v", "bo0", "bo1")}
    assert nf_bufs == {48}
    if store == "bf16":                       # the long skip as hi + lo pairs
        assert [(o.w, o.hilo) for o in plan.ops if o.kind == "conv" and o.hilo] == [
            ("fea_conv#head", L.HILO_OUT), ("LR_conv", L.HILO_RES | L.HILO_OUT), ("upsampler.0", L.HILO_IN)]
    # the counters see the reference's 59 convolutions, conv_2 / conv_3 / conv_23 at 48 x 73 pixels
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    ref = model_complexity(m, (3, 339, 510))
    assert (sum(t[0] for t in terms) / 2, sum(t[1] for t in terms) / 2, sum(t[2] for t in terms)) == \
        (ref["flops"], ref["activations"], ref["num_conv"])
    lowres_convs = [c for o in plan.ops for c in m._counted_convs(plan, o) if c[3] == 2 * 48 * 73]
    assert sorted(c[:3] for c in lowres_convs) == sorted([(10, 10, 3), (10, 10, 3), (20, 10, 3)] * 4)
    # the op list encodes (fake device addresses: no GPU needed)
    m.compute = store
    m._repack("cpu")
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    for i, o in enumerate(plan.ops):
        if o.kind == "lowres":
            d = arr[i].lo
            assert arr[i].kind == L.OP_ESA_LOWRES and not d.w_s2 and d.n_layers == 2 and (d.h, d.w, d.f) == (339, 510, 10)
            assert (d.layer[0].kind, d.layer[1].kind) == (2, 3) and d.layer[0].w_dw and not d.layer[1].w_dw
        if o.kind == "pool7":
            e = arr[i].esa
            assert arr[i].kind == L.OP_MAXPOOL7S7 and (e.h, e.w, e.h_lo, e.w_lo) == (339, 510, 48, 73) and e.storage == L.STORE[store]
    costs = m.op_costs(plan, arr)
    if fuse:
        lk = [c for c in costs if "pool7_branch" in c["kernel"]]
        assert len(lk) == 4 and lk[0]["kernel"] == f"esa_pool7_kernel<{L.STORE[store]}> + esa_pool7_branch_kernel"
        assert lk[0]["flops"] == 2.0 * 2 * 48 * 73 * (2 * 9 * 100 + 9 * 200)


def test_conv_23_blob_holds_the_halves_at_rows_0_and_16():
    import torch
    m = _efdn()
    m._repack("cpu")
    blob = m._packed["B2.esa.conv_23#dense"]
    assert blob.numel() == 9 * 32 * 16 + 16
    w = m.B2.esa.conv_23.weight.detach()
    img = blob[:9 * 32 * 16].view(3, 3, 32, 16)                 # [tap][row][cout]
    assert torch.equal(img[..., :10, :10].permute(3, 2, 0, 1), w[:, :10])
    assert torch.equal(img[..., 16:26, :10].permute(3, 2, 0, 1), w[:, 10:])
    assert not img[..., 10:16, :].any() and not img[..., 26:, :].any() and not img[..., 10:].any()
    assert torch.equal(blob[9 * 32 * 16:9 * 32 * 16 + 10], m.B2.esa.conv_23.bias.detach()) and not blob[-6:].any()


def test_small_inputs_are_refused():
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    m = _efdn()
    for h, w in ((4, 20), (20, 7)):
        with pytest.raises(L.EsrError, match="PLAINRFDN needs"):
            m._build_plan(Plan(1, h, w), 3)
    m._build_plan(Plan(1, 5, 8), 3)


def test_shim_resolves_team05_efdn():
    code = ("import json; from safetensors.torch import load_file; from models.team05_efdn.plainsr import PLAINRFDN; m = PLAINRFDN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, PLAINRFDN is e.PLAINRFDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.efdn", True, 272038]


def _lowres_desc(L, a, **kw):
    d = L.EsaLowresDesc()
    d.n, d.h, d.w, d.f, d.storage, d.n_layers = 1, 32, 40, 10, L.STORE["bf16"], 2
    d.x = L.View(a, 16, 0)
    d.w_s2, d.pooled, d.y = None, a, a
    d.layer[0].kind, d.layer[0].act, d.layer[0].w, d.layer[0].w_dw = 2, L.ACT_RELU, a, a
    d.layer[1].kind, d.layer[1].act, d.layer[1].w = 3, L.ACT_NONE, a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_pool7_descriptor_validation_without_gpu():
    """the w_s2 = NULL form of esr_esa_lowres_f32 and esr_maxpool7s7_f32 validate before anything is launched"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    run = lambda d: lib.esr_esa_lowres_f32(ctypes.byref(d), None)
    assert run(_lowres_desc(L, a, f=0)) == -1 and run(_lowres_desc(L, a, f=17)) == -1          # bad f
    d = _lowres_desc(L, a)
    d.layer[0].w_dw = None                                                                       # the pair's second 3x3 missing
    assert run(d) == -1
    d = _lowres_desc(L, a)
    d.layer[1].w = None                                                                          # conv_23 missing
    assert run(d) == -1
    d = _lowres_desc(L, a)
    d.layer[1].kind = 0                                                                          # kind 3 must follow the pair
    assert run(d) == -1
    assert run(_lowres_desc(L, a, n_layers=3)) == -1
    assert run(_lowres_desc(L, a, pooled=None)) == -1 and run(_lowres_desc(L, a, storage=3)) == -1
    assert run(_lowres_desc(L, a, x=L.View(a, 32, 0))) == -1
    assert run(_lowres_desc(L, a, h=4)) == -4                                                    # ESR_ERR_TOO_SMALL
    assert run(_lowres_desc(L, a, w=4)) == -4 and run(_lowres_desc(L, a, h=4, w=4)) == -4
    # RFDN's form is unchanged: a stride-2 weight and kind-0 layers, H, W >= 15
    d = _lowres_desc(L, a, w_s2=a, h=14, n_layers=1)
    d.layer[0].kind = 0
    assert run(d) == -4
    # the per-op pooling
    e = L.EsaDesc()
    e.n, e.h, e.w, e.h_lo, e.w_lo, e.storage = 1, 339, 510, 48, 73, L.STORE["f16"]
    e.x, e.y = L.View(a, 16, 0), L.View(a, 16, 0)
    pool = lambda **kw: lib.esr_maxpool7s7_f32(ctypes.byref(_set(e, **kw)), None)
    assert pool(h_lo=49) == -1 and pool(w_lo=72) == -1                                           # pooled size (h - 5) / 7 + 1
    assert pool(h=4, h_lo=0) == -4 and pool(w=4, w_lo=0) == -4
    assert pool(x=L.View(a, 32, 0)) == -1 and pool(y=L.View(None, 16, 0)) == -1
    assert pool(storage=5) == -1


def _set(e, **kw):
    e2 = type(e).from_buffer_copy(e)
    for k, v in kw.items():
        setattr(e2, k, v)
    return e2
