"""CPU: RFDNeXt (NTIRE 2022 ESR team 38, models.team38_rfdnext.RFDN.RFDN) on the engine -- checkpoint surface, complexity counters in both
forms of the ConvNeXt block and every storage, plan shape, the packers (depthwise 7x7, the fused block's 1x1 pair, the c1_d-into-c1_r fold),
the shim import path, and the C ABI's validation of esr_dwconv7x7 / esr_cx_block_s16 without a GPU."""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team38_rfdnext.safetensors")
WANT = {"activations": 150601728.0, "num_conv": 48, "flops": 18946457600.0, "num_parameters": 290048}


def _rfdnext(store="f32", fuse=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import RFDNeXt
    m = RFDNeXt(block_type="RFDB", act_type="lrelu")
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_cx = fuse
    return m


def test_checkpoint_loads_strict_with_the_reference_parameter_count():
    from safetensors.torch import load_file
    sd = load_file(CKPT)
    m = _rfdnext()
    assert len(sd) == 96 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 290048
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert tuple(sd["B2.esa.conv.0.weight"].shape) == (50, 1, 7, 7) and tuple(sd["B2.esa.conv.1.weight"].shape) == (200, 50, 1, 1)
    assert tuple(sd["B2.esa.conv.3.weight"].shape) == (50, 200, 1, 1) and tuple(sd["B2.c1_r.weight"].shape) == (25, 50, 3, 3)
    assert tuple(sd["B2.c5.weight"].shape) == (50, 100, 1, 1) and tuple(sd["c.0.weight"].shape) == (50, 200, 1, 1)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import RFDNeXt
    for kw in (dict(block_type="MRB"), dict(act_type="gelu"), dict(act_type="relu"), dict(nf=48), dict(nf=64), dict(upscale=2),
               dict(num_modules=6), dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            RFDNeXt(**kw)
    RFDNeXt(block_type="RFDB", act_type="lrelu")


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    assert json.load(open(os.path.join(GOLD, "summary_team38_rfdnext.json"))) == WANT
    assert model_complexity(_rfdnext(store, fuse), (3, 256, 256)) == WANT


def _plan(m, n, h, w):
    from ntire2022_esr_amd.engine import Plan
    plan = Plan(n, h, w, m._store())
    m._build_plan(plan, 3)
    return plan


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("nhw", [(1, 5, 9), (2, 45, 70)])
def test_plans_build_and_finalize_in_every_storage_and_both_forms(store, fuse, nhw):
    from ntire2022_esr_amd import _lib as L
    m = _rfdnext(store, fuse)
    m._repack("cpu")
    plan = _plan(m, *nhw)                           # (no ESA: nothing below 15 x 15 is refused)
    arr, in_idx, out_idx = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [o for o in plan.ops if o.kind == "cx"]
    assert len(fused) == (4 if fuse and store != "f32" else 0)
    dws = [i for i, o in enumerate(plan.ops) if o.kind == "dw7"]
    assert len(dws) == 4 - len(fused) and all(arr[i].kind == L.OP_DWCONV7 == 13 and L.lib().esr_dwconv7x7_supported(ctypes.byref(arr[i].conv)) for i in dws)
    assert len(in_idx) == 1 and len(out_idx) == 1
    # the counted convolutions: c1_d and c1_r are two of them although c1_d is also folded into c1_r's centre tap
    names = [o.w for o in plan.ops if o.kind == "conv"]
    assert all(f"B{k}.c1_d" in names and f"B{k}.c1_r#fold" in names for k in range(1, 5))


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_fuse_cx_replaces_exactly_three_ops_per_block(store):
    """a 16-bit plan at 2 x 45 x 70: 4 cx ops whose descriptors satisfy esr_cx_block_supported; each stands for [dw7, 1x1 50 -> 200 + lrelu,
    1x1 200 -> 50 + v] of its block, and the rest of the plan is the per-op plan without the ConvNeXt blocks' launches"""
    from ntire2022_esr_amd import _lib as L
    m = _rfdnext(store, True)
    m._repack("cpu")
    plan = _plan(m, 2, 45, 70)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "cx"]
    assert len(fused) == 4
    tf = "true" if store == "bf16" else "false"
    costs = m.op_costs(plan, arr)
    for k, (i, o) in enumerate(fused, 1):
        assert len(o.replaces) == 3
        assert [(c.kind, c.w) for c in o.replaces] == [("dw7", f"B{k}.esa.conv.0"), ("conv", f"B{k}.esa.conv.1"), ("conv", f"B{k}.esa.conv.3")]
        d = arr[i].chain
        assert arr[i].kind == L.OP_CX_BLOCK == 14
        assert L.lib().esr_cx_block_supported(ctypes.byref(d)) == 1
        assert (d.n, d.h, d.w, d.n_layers, d.cin, d.cmid, d.cout) == (2, 45, 70, 3, 50, 200, 50)
        assert d.act == L.ACT_LRELU and abs(d.slope - 0.05) < 1e-9 and d.res_mode == L.RES_POST_ACT
        assert (d.inp.pitch, d.inp.coff) == (56, 0) and (d.post_out.pitch, d.post_out.coff, d.post_cout) == (56, 0, 56)
        assert d.post_out.ptr != d.inp.ptr and all(d.wpacked[l] for l in range(3)) and not d.wpacked[3]
        assert not d.post_wpacked and not d.post2_wpacked
        assert costs[i]["kernel"] == f"cx_block_kernel<{tf}>"
    per_op = _plan(_rfdnext(store, False), 2, 45, 70)
    cx = re.compile(r"B\d\.esa\.conv\.")
    is_cx = lambda o: o.kind == "dw7" or (o.kind == "conv" and cx.match(o.w))
    # per op a block's ConvNeXt tail is the depthwise 7x7, four output-channel slices of the first 1x1 and the second 1x1
    assert [o.w for o in per_op.ops if is_cx(o)][:6] == ["B1.esa.conv.0"] + [f"B1.esa.conv.1#o{j}" for j in range(4)] + ["B1.esa.conv.3"]
    assert not any(o.kind == "cx" for o in per_op.ops)
    rest = [(o.kind, getattr(o, "w", None)) for o in per_op.ops if not is_cx(o)]
    assert rest == [(o.kind, getattr(o, "w", None)) for o in plan.ops if o.kind != "cx"]
    # ... and only the per-op plan keeps the buffers between those launches (at 32 x 256 x 256 they are a quarter of its workspace)
    assert {"t", "hid"} <= {b.name for b in per_op.buffers} and not {"t", "hid"} & {b.name for b in plan.buffers}
    assert plan.total < per_op.total
    # the hidden slices tile 200 channels of one buffer
    sl = [o for o in per_op.ops if o.kind == "conv" and o.w.startswith("B1.esa.conv.1#o")]
    assert [(o.dst[1], o.dst[2]) for o in sl] == [(0, 64), (64, 64), (128, 64), (192, 8)] and len({id(o.dst[0]) for o in sl}) == 1


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


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("nhw", [(1, 5, 9), (2, 45, 70), (32, 256, 256)])
def test_every_view_of_every_op_lies_inside_the_workspace(store, fuse, nhw):
    """the finalized descriptors, not the plan's bookkeeping: every tensor a launch addresses -- n x h x w pixels of its pitch from the
    view's pointer -- lies inside the plan.total bytes the engine allocates, also where a fully fused plan has given buffers back"""
    m = _rfdnext(store, fuse)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    base = 1 << 44                                  # (far from every host address a weight blob may have)
    arr, _, _ = plan.finalize((base, plan.total_lo), m._packed)
    assert plan.total_lo == 0
    es = plan.esize
    seen = 0
    for i, o in enumerate(plan.ops):
        for name, v in _views(arr[i]):
            if not v.ptr:
                continue
            seen += 1
            lo, hi = v.ptr - base, v.ptr - base + plan.n * plan.h * plan.w * v.pitch * es
            assert 0 <= lo and hi <= plan.total, (i, o.kind, getattr(o, "w", None), name, lo, hi, plan.total)
    assert seen > 2 * len(plan.ops) - 4
    # the buffers tile the arena, and release() takes only the last allocations
    assert max(b.offset + plan.n * b.h * b.w * b.pitch * b.esize for b in plan.buffers) <= plan.total
    from ntire2022_esr_amd import _lib as L
    with pytest.raises(L.EsrError, match="last full-resolution allocations"):
        plan.release([plan.buffers[0]])


def test_fp32_plan_slices_the_first_pointwise_for_conv_f32_kernel():
    plan = _plan(_rfdnext("f32", True), 1, 32, 32)
    sl = [o for o in plan.ops if o.kind == "conv" and o.w.startswith("B3.esa.conv.1#o")]
    assert [(o.dst[1], o.dst[2]) for o in sl] == [(0, 56), (56, 56), (112, 56), (168, 32)] and all(o.cout <= 64 for o in sl)
    assert sl[0].dst[0].pitch == 200 and not any(o.kind == "cx" for o in plan.ops)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("fuse", [False, True])
def test_op_kinds_do_not_depend_on_the_batch(store, fuse):
    m = _rfdnext(store, fuse)
    kinds = [[(o.kind, getattr(o, "w", None)) for o in _plan(m, n, 45, 45).ops] for n in (1, 8)]
    assert kinds[0] == kinds[1]


# ---- packers ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 33, 50, 64])
def test_dw7_pack_unpack_round_trip(c):
    from ntire2022_esr_amd.engine import pack_dw7, unpack_dw7
    g = torch.Generator().manual_seed(c)
    w, b = torch.randn(c, 1, 7, 7, generator=g), torch.randn(c, generator=g)
    blob = pack_dw7(w, b)
    cp = (c + 7) // 8 * 8
    assert blob.numel() == 50 * cp
    w2, b2 = unpack_dw7(blob, c)
    assert torch.equal(w2, w) and torch.equal(b2, b)
    img = blob.reshape(50, cp)
    assert not bool(img[:, c:].any())                                   # pad channels: zero weights, zero bias
    assert float(img[3 * 7 + 5, c - 1]) == float(w[c - 1, 0, 3, 5])      # [tap = ky * 7 + kx][channel]


def _mfma(a, b):
    """v_mfma_f32_16x16x32's operand layout in fp64: a [64 lanes, 8] holds A[row l & 15][k = 8 (l >> 4) + j], b [64, 8] holds
    B[k = 8 (l >> 4) + j][col l & 15]; returns D as [64 lanes, 4]: D[row 4 (l >> 4) + i][col l & 15]"""
    A, B = np.zeros((16, 32)), np.zeros((32, 16))
    for l in range(64):
        A[l & 15, 8 * (l >> 4):8 * (l >> 4) + 8] = a[l]
        B[8 * (l >> 4):8 * (l >> 4) + 8, l & 15] = b[l]
    D = A @ B
    return np.stack([[D[4 * (l >> 4) + i, l & 15] for i in range(4)] for l in range(64)])


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("c,m", [(50, 200), (33, 129), (64, 256)])
def test_permuted_pointwise_pair_evaluates_to_the_same_function(store, c, m):
    """cx_block_kernel's data flow replayed in numpy fp64 on the packed fragment images -- t fragments from a [pixel][64 channels] tile, the first
    GEMM's accumulators of two output tiles packed into the second GEMM's B fragment without leaving the lane -- equals
    W2 . lrelu(W1 . t + b1) + b2 on the weights rounded once to the storage type, to 1e-12"""
    from ntire2022_esr_amd.engine import cx_pw_fragments, pack_cx_pw
    dt = torch.bfloat16 if store == "bf16" else torch.float16
    g = torch.Generator().manual_seed(c + m)
    w1, b1 = torch.randn(m, c, 1, 1, generator=g) * 0.1, torch.randn(m, generator=g) * 0.1
    w2, b2 = torch.randn(c, m, 1, 1, generator=g) * 0.05, torch.randn(c, generator=g) * 0.1
    A1, B1, A2, B2 = cx_pw_fragments(*pack_cx_pw(w1, b1, w2, b2, store), m, store)
    nhp = (m + 31) // 32
    assert A1.shape == (2 * nhp, 2, 64, 8) and A2.shape == (nhp, 4, 64, 8) and B1.shape == (32 * nhp,) and B2.shape == (64,)
    t = np.zeros((16, 64))
    t[:, :c] = torch.randn(16, c, generator=g).double().numpy()
    lanes = np.arange(64)
    px, kq = lanes & 15, lanes >> 4
    bt = [np.stack([t[px[l], ks * 32 + kq[l] * 8:ks * 32 + kq[l] * 8 + 8] for l in range(64)]) for ks in range(2)]
    acc2 = [np.stack([B2[mt * 16 + kq[l] * 4:mt * 16 + kq[l] * 4 + 4] for l in range(64)]) for mt in range(4)]
    for hp in range(nhp):
        h = []
        for j in range(2):
            acc = np.stack([B1[(hp * 2 + j) * 16 + kq[l] * 4:(hp * 2 + j) * 16 + kq[l] * 4 + 4] for l in range(64)])
            acc = acc + _mfma(A1[hp * 2 + j, 0], bt[0]) + _mfma(A1[hp * 2 + j, 1], bt[1])
            h.append(np.where(acc > 0, acc, 0.05 * acc))
        bh = np.concatenate(h, axis=1)                                   # the lane's 8 values: tile 0's four, tile 1's four
        for mt in range(4):
            acc2[mt] = acc2[mt] + _mfma(A2[hp, mt], bh)
    got = np.zeros((16, 64))
    for mt in range(4):
        for l in range(64):
            got[px[l], mt * 16 + kq[l] * 4:mt * 16 + kq[l] * 4 + 4] = acc2[mt][l]
    w1e, w2e = w1.to(dt).double().reshape(m, c).numpy(), w2.to(dt).double().reshape(c, m).numpy()
    hid = t[:, :c] @ w1e.T + b1.double().numpy()
    ref = np.where(hid > 0, hid, 0.05 * hid) @ w2e.T + b2.double().numpy()
    assert np.abs(got[:, :c] - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    assert not got[:, c:].any()                                          # pad output channels: zero rows, zero bias


def test_c1d_folded_into_c1r_equals_their_sum():
    from ntire2022_esr_amd.engine import fold_center
    g = torch.Generator().manual_seed(5)
    w_r, b_r = torch.randn(25, 50, 3, 3, generator=g), torch.randn(25, generator=g)
    w_d, b_d = torch.randn(25, 50, 1, 1, generator=g), torch.randn(25, generator=g)
    w, b = fold_center(w_r, b_r, w_d, b_d)
    assert w.dtype == torch.float32 and torch.equal(w[:, :, 0, 0], w_r[:, :, 0, 0]) and torch.equal(w[:, :, 1, 1], w_r[:, :, 1, 1] + w_d[:, :, 0, 0])
    x = torch.randn(1, 50, 9, 9, generator=g).double()
    ref = F.conv2d(x, w_r.double(), b_r.double(), padding=1) + F.conv2d(x, w_d.double(), b_d.double())
    # arbitrary fp32 weights: the fold is summed in fp32, so it agrees with the unfolded sum to fp32's rounding
    got = F.conv2d(x, w.double(), b.double(), padding=1)
    assert float((got - ref).abs().max()) <= 2.0 ** -22 * float(ref.abs().max())
    # weights as the checkpoints hold them (bf16-representable, tools/gen_golden_rfdnext.py): the fp32 sums are exact and the fold IS the sum
    q = lambda t: t.to(torch.bfloat16).float()
    w_r, b_r, w_d, b_d = q(w_r), q(b_r), q(w_d), q(b_d)
    w, b = fold_center(w_r, b_r, w_d, b_d)
    ref = F.conv2d(x, w_r.double(), b_r.double(), padding=1) + F.conv2d(x, w_d.double(), b_d.double())
    got = F.conv2d(x, w.double(), b.double(), padding=1)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # the model packs exactly this fold
    m = _rfdnext()
    m._repack("cpu")
    from ntire2022_esr_amd.engine import pack_conv
    wf, bf = fold_center(m._leaf("B3.c1_r").weight, m._leaf("B3.c1_r").bias, m._leaf("B3.c1_d").weight, m._leaf("B3.c1_d").bias)
    assert torch.equal(m._packed["B3.c1_r#fold"], pack_conv(wf, bf))


def test_shim_resolves_team38_rfdnext():
    code = ("import json; from safetensors.torch import load_file; from models.team38_rfdnext.RFDN import RFDN; "
            "m = RFDN(block_type='RFDB', act_type='lrelu'); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, RFDN is e.RFDNeXt, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.rfdnext", True, 290048]


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def _cx_desc(L, a, **kw):
    """the model's own descriptor at 1 x 32 x 40: v and the result in two pitch-56 tensors"""
    d = L.ChainDesc()
    d.n, d.h, d.w, d.n_layers = 1, 32, 40, 3
    d.cin, d.cmid, d.cout = 50, 200, 50
    d.act, d.slope, d.res_mode = L.ACT_LRELU, 0.05, L.RES_POST_ACT
    d.storage = d.compute = L.STORE["bf16"]
    d.inp = L.View(a, 56, 0)
    for l in range(3):
        d.wpacked[l] = a
    d.post_out, d.post_cout = L.View(a + 4096, 56, 0), 56
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_cx_block_descriptor_validation_without_gpu():
    """esr_cx_block_supported / esr_cx_block_s16 validate before anything is launched: fp32 storage and every shape outside the ranges are
    ESR_ERR_UNSUPPORTED, null pointers, broken views and a result in v's tensor ESR_ERR_BAD_ARG"""
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    b = a + 4096
    sup = lambda **kw: lib.esr_cx_block_supported(ctypes.byref(_cx_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_cx_block_s16(ctypes.byref(_cx_desc(L, a, **kw)), None)
    assert sup() == 1 and sup(storage=L.STORE["f16"], compute=L.COMPUTE["f16"]) == 1
    assert sup(cin=33, cout=33, post_cout=40) == 1 and sup(cin=64, cout=64, post_cout=64, inp=L.View(a, 64, 0), post_out=L.View(b, 64, 0)) == 1
    assert sup(cmid=129) == 1 and sup(cmid=256) == 1 and sup(post_cout=64, post_out=L.View(b, 64, 0)) == 1
    refused = [dict(cin=32, cout=32), dict(cin=65, cout=65), dict(cout=49), dict(cmid=128), dict(cmid=257), dict(act=L.ACT_RELU), dict(act=L.ACT_NONE),
               dict(res_mode=L.RES_NONE), dict(res_mode=L.RES_PRE_ACT), dict(res_mode=L.RES_GATE), dict(storage=0, compute=0),
               dict(compute=L.COMPUTE["f16"]), dict(n_layers=2), dict(n_layers=4), dict(post_wpacked=a), dict(post2_wpacked=a),
               dict(post_cout=48), dict(post_cout=50), dict(post_cout=72), dict(n=0), dict(h=0), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_cx_block_supported(None) == 0 and lib.esr_cx_block_s16(None, None) == -1
    for kw in (dict(inp=L.View(None, 56, 0)), dict(post_out=L.View(None, 56, 0))):
        assert run(**kw) == -1, kw
    for l in range(3):
        d = _cx_desc(L, a)
        d.wpacked[l] = None
        assert lib.esr_cx_block_s16(ctypes.byref(d), None) == -1, l
    for kw in (dict(inp=L.View(a, 56, 8)), dict(inp=L.View(a, 60, 0)), dict(inp=L.View(a, 48, 0)), dict(inp=L.View(a, 64, 12)),
               dict(post_out=L.View(b, 48, 0)), dict(post_out=L.View(b, 64, 16)), dict(post_out=L.View(b, 60, 0)), dict(post_out=L.View(b, 64, 4)),
               dict(post_out=L.View(a, 112, 56)), dict(inp=L.View(a, 112, 0), post_out=L.View(a, 112, 56))):     # a result in v's tensor: the halo is still being read
        assert run(**kw) == -1, kw
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the LDS opt-in / the launch
        assert run() == -3
        op = L.Op()
        op.kind, op.chain = L.OP_CX_BLOCK, _cx_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
        op.chain = _cx_desc(L, a, cmid=128)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -2


def _dw_desc(L, a, store="f32", **kw):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = 1, 32, 40, 50, 50, 7
    d.in_layout = d.out_layout = L.NHWC
    d.storage = L.STORE[store]
    d.inp, d.out0 = L.View(a, 56, 0), L.View(a + 4096, 56, 0)
    d.wpacked = a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_dwconv7x7_descriptor_validation_without_gpu():
    from ntire2022_esr_amd import _lib as L
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    a = ctypes.addressof(buf)
    b = a + 4096
    sup = lambda store="f32", **kw: lib.esr_dwconv7x7_supported(ctypes.byref(_dw_desc(L, a, store, **kw)))
    run = lambda store="f32", **kw: lib.esr_dwconv7x7(ctypes.byref(_dw_desc(L, a, store, **kw)), None)
    assert sup() == 1 and sup("bf16") == 1 and sup("f16") == 1
    assert all(sup(st, cin=c, cout=c, inp=L.View(a, 64, 0), out0=L.View(b, 64, 0)) == 1 for st in ("f32", "bf16", "f16") for c in (1, 33, 64))
    for kw in (dict(ksize=3), dict(cout=49), dict(cin=65, cout=65), dict(cin=0, cout=0), dict(act=L.ACT_LRELU), dict(res_mode=L.RES_PRE_ACT),
               dict(in_layout=L.NCHW_IN), dict(out_layout=L.NCHW_SHUFFLE4), dict(storage=7), dict(n=0), dict(w=0),
               # features of esr_conv_desc the launch does not implement are refused, not dropped
               dict(post_wpacked=a), dict(post2_wpacked=a), dict(tail_wpacked=a), dict(split=8), dict(out1=L.View(b, 56, 0)), dict(hilo=L.HILO_OUT),
               dict(border_bias=a), dict(blocked8=L.BLOCKED_IN), dict(in_seg_stride=4096), dict(wino_wpacked=a)):
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw
    assert lib.esr_dwconv7x7_supported(None) == 0 and lib.esr_dwconv7x7(None, None) == -1
    for kw in (dict(inp=L.View(None, 56, 0)), dict(out0=L.View(None, 56, 0)), dict(wpacked=None), dict(inp=L.View(a, 48, 0)), dict(out0=L.View(b, 56, 8)),
               dict(inp=L.View(a, 54, 0)), dict(out0=L.View(a, 112, 56))):
        assert run(**kw) == -1, kw
    assert run("bf16", inp=L.View(a, 52, 0)) == -1                                  # 16-bit storage needs round_up(50, 8) channels ...
    if torch.cuda.device_count() == 0:
        # a VALID descriptor on a host without a GPU passes every check and fails in the launch
        assert run() == -3 and run("bf16") == -3
        assert run("f32", inp=L.View(a, 52, 0)) == -3                               # ... fp32 round_up(50, 4)
        op = L.Op()
        op.kind, op.conv = L.OP_DWCONV7, _dw_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
