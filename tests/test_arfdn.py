"""CPU: ARFDN (NTIRE 2022 ESR team 14, models.team14_arfdn.ARFDN.ARFDN) on the engine -- checkpoint surface and refusals, the 3-tap packer
read back, the per-layer fold of a step restated in fp64 against the plain step, complexity counters in every storage and both forms, plan
shape, esr_asym_step's validation without a GPU, and the shim and registry paths."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import _arfdn as A
from conftest import GOLD, REPO

SHIM = os.path.join(REPO, "shim")
CKPT = os.path.join(GOLD, "team14_arfdn.safetensors")
WANT = {"activations": 151355840.0, "num_conv": 100, "flops": 14506603360.0, "num_parameters": 241548}
STORES = ["f32", "bf16", "f16"]


def _arfdn(store="f32", fuse=True):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import ARFDN
    m = ARFDN()
    m.load_state_dict(load_file(CKPT), strict=True)
    m.set_compute(store)
    m.fuse_asym = fuse
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
    m = _arfdn()
    assert len(sd) == 200 and set(m.state_dict()) == set(sd)
    assert sum(p.numel() for p in m.parameters()) == 241548
    assert all(tuple(m.state_dict()[k].shape) == tuple(v.shape) for k, v in sd.items())
    assert tuple(sd["B1.c1_l1.weight"].shape) == (25, 50, 3, 1) and tuple(sd["B1.c1_m1.weight"].shape) == (25, 50, 1, 3)
    assert tuple(sd["B2.c3_l2.weight"].shape) == (25, 25, 1, 3) and tuple(sd["B2.c3_m2.weight"].shape) == (25, 25, 3, 1)
    assert tuple(sd["B3.c0_d.weight"].shape) == (25, 50, 1, 1) and tuple(sd["B3.c2_d.weight"].shape) == (25, 25, 1, 1)
    assert tuple(sd["B4.c5.weight"].shape) == (50, 100, 1, 1) and tuple(sd["B4.mpa.conv_max.weight"].shape) == (12, 12, 3, 3)
    assert tuple(sd["c.0.weight"].shape) == (50, 200, 1, 1) and "c.1.weight" not in sd and hasattr(m, "set_scale")
    # the unrounded checkpoint: the same keys, fp32, under the file size limit; the fixture is its RNE rounding to bf16
    p = os.path.join(GOLD, "team14_arfdn_f32.safetensors")
    assert os.path.getsize(p) <= 1 << 20
    true = load_file(p)
    assert set(true) == set(sd) and all(v.dtype == torch.float32 for v in true.values())
    assert all(torch.equal(true[k].to(torch.bfloat16).view(torch.int16), sd[k].view(torch.int16)) for k in sd)
    m.load_state_dict(true, strict=True)


def test_unsupported_constructor_arguments_are_refused():
    from ntire2022_esr_amd import ARFDN
    for kw in (dict(nf=48), dict(nf=64), dict(num_modules=3), dict(num_modules=6), dict(in_nc=5), dict(out_nc=5)):
        with pytest.raises(NotImplementedError):
            ARFDN(**kw)
    ARFDN(in_nc=3, out_nc=3, nf=50, num_modules=4)
    ARFDN(in_nc=1, out_nc=4)


@pytest.mark.parametrize("store", STORES)
def test_inputs_below_15_pixels_are_refused_with_the_reason(store):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import Plan
    m = _arfdn(store)
    for h, w in ((14, 40), (40, 14)):
        with pytest.raises(L.EsrError, match="H, W >= 15"):
            _plan(m, 1, h, w)
    _plan(m, 1, 15, 15)
    with pytest.raises(L.EsrError, match="3 input channels"):
        m._build_plan(Plan(1, 20, 20, store), 4)


def test_c1_carries_slope_0_1_and_the_blocks_0_05():
    """block.py's activation() defaults to 0.1 and conv_block passes no slope: c.1 is LeakyReLU(0.1), every other one LeakyReLU(0.05)"""
    from ntire2022_esr_amd import _lib as L
    for store in STORES:
        for fuse in (False, True):
            plan = _plan(_arfdn(store, fuse), 1, 20, 24)
            c0 = [o for o in plan.ops if o.kind == "conv" and o.w == "c.0"]
            assert len(c0) == 1 and c0[0].act == L.ACT_LRELU and c0[0].slope == 0.1
            for o in plan.ops:
                for q in getattr(o, "replaces", [o]):
                    if q.kind == "conv" and q.w != "c.0" and q.act == L.ACT_LRELU:
                        assert q.slope == 0.05, q.w


# ---- the 3-tap packer ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("cin,c", [(50, 25), (25, 25), (17, 17), (32, 32), (33, 20), (64, 32)])
def test_asym_blob_round_trip(store, cin, c):
    """pack, then read the effective weights back: each weight rounded once (RNE) to the storage type, the biases fp32 with b_l2 + b_m2 summed;
    zero rows and columns beyond c / cin; the documented fragment order; the model packs exactly this"""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_asym_s16, unpack_asym_s16
    dt = A.DT[store]
    g = torch.Generator().manual_seed(100 * cin + c)
    ws = [torch.randn(c, cin, 3, 1, generator=g), torch.randn(c, cin, 1, 3, generator=g), torch.randn(c, c, 1, 3, generator=g), torch.randn(c, c, 3, 1, generator=g)]
    bs = [torch.randn(c, generator=g) for _ in range(4)]
    blob = pack_asym_s16(ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], ws[3], bs[3], store)
    nkp = 2 if cin > 32 else 1
    nfrag = 2 * 3 * nkp * 2 + 2 * 3 * 2
    assert blob.numel() * 4 == nfrag * 1024 + 3 * 32 * 4 == L.lib().esr_packed_asym_s16_bytes(cin, c)
    we, be = unpack_asym_s16(blob, cin, c, store)
    for got, w in zip(we, ws):
        assert got.shape == w.shape and torch.equal(got, w.to(dt).float())
    assert torch.equal(be[0], bs[0]) and torch.equal(be[1], bs[1]) and torch.equal(be[2], bs[2] + bs[3])
    img = blob.view(torch.uint8)[:nfrag * 1024].view(dt).reshape(nfrag, 64, 8)
    # lane (row, kq) element e of fragment (tap, kp, o) of l1 = W_l1[16 o + row][32 kp + 8 kq + e][tap]; m2's image is the last
    tap, kp, o, row, kq, e = 2, nkp - 1, 1, 0, 0, 0
    assert float(img[(tap * nkp + kp) * 2 + o, 16 * kq + row, e]) == float(ws[0][16 + row, 32 * kp + e, tap, 0].to(dt))
    assert float(img[nfrag - 6 + 1 * 2 + 0, 16 * 1 + 2, 4]) == float(ws[3][2, 12, 1, 0].to(dt))
    full = img.float()
    assert int((full != 0).sum()) <= 3 * c * (2 * cin + 2 * c)                     # nothing beyond c rows / cin columns
    for bad in ((16, 16), (65, 25), (25, 33)):
        with pytest.raises(Exception):
            pack_asym_s16(torch.zeros(bad[1], bad[0], 3, 1), None, torch.zeros(bad[1], bad[0], 1, 3), None, torch.zeros(bad[1], bad[1], 1, 3), None,
                          torch.zeros(bad[1], bad[1], 3, 1), None, store)
    with pytest.raises(Exception):                                                  # a transposed pair
        pack_asym_s16(ws[1], bs[0], ws[0], bs[1], ws[2], bs[2], ws[3], bs[3], store)
    if (cin, c) == (50, 25):
        m = _arfdn(store)
        m._repack("cpu")
        leaf = lambda n: m._leaf("B2.c1_" + n)
        want = pack_asym_s16(*(t for n in ("l1", "m1", "l2", "m2") for t in (leaf(n).weight, leaf(n).bias)), store)
        assert torch.equal(m._packed["B2.c1_l1#asym"], want)


# ---- the per-layer fold -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j,s16", [(1, False), (2, False), (3, False), (3, True)])
def test_per_layer_fold_equals_the_plain_step_in_fp64(j, s16):
    """arfdn.py's fold -- [a_l | a_m] as one plus-shaped 3x3, then one 3x3 over a slot range of the block buffer with c_l2 in the middle row,
    c_m2 in the middle column and identity centre taps for the distilled maps, `+ r` as the residual; a 16-bit plan's third step with
    q = d_2 + d_1 in one slot -- restated in torch fp64 equals the plain ARFDB step (block.py:233-254) to 1e-12 at 5 x 7, border rows and
    columns included"""
    from ntire2022_esr_amd import arfdn as M
    dc, cin, slope = 25, (50 if j == 1 else 25), 0.05
    g = torch.Generator().manual_seed(j)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    r = rn(2, cin, 5, 7)
    ds = [rn(2, dc, 5, 7) for _ in range(j - 1)]                  # d_{j-1} .. d_1, nearest first
    wd, bd = rn(dc, cin, 1, 1) * 0.2, rn(dc)
    wl1, bl1, wm1, bm1 = rn(dc, cin, 3, 1) * 0.2, rn(dc), rn(dc, cin, 1, 3) * 0.2, rn(dc)
    wl2, bl2, wm2, bm2 = rn(dc, dc, 1, 3) * 0.2, rn(dc), rn(dc, dc, 3, 1) * 0.2, rn(dc)
    lrelu = lambda v: F.leaky_relu(v, slope)
    # the plain step
    d = lrelu(F.conv2d(r, wd, bd))
    l = F.conv2d(lrelu(F.conv2d(r, wl1, bl1, padding=(1, 0))), wl2, bl2, padding=(0, 1))
    mm = F.conv2d(lrelu(F.conv2d(r, wm1, bm1, padding=(0, 1))), wm2, bm2, padding=(1, 0))
    want = lrelu(l + mm + (r if j > 1 else 0) + d + sum(ds))
    # the fold, on the physical slots of the block buffer: NaN wherever nothing was written
    dj, ps, (lo, hi), ident = M.ARFDN._step(j, s16)
    assert hi - lo == {(1, False): 96, (2, False): 128, (3, False): 160, (3, True): 128}[(j, s16)] and (not s16 or hi - lo <= M.KMAX) and lo % 16 == 0
    S = torch.full((2, M.SPITCH, 5, 7), float("nan"), dtype=torch.float64)
    for s0 in [dj] + list(ps) + [M.A, M.A + 32] + ([M.Q] if s16 else []):
        S[:, s0:s0 + M.SEG] = 0.0                                 # (a producer writes its slice's pad channels as zeros)
    S[:, dj:dj + dc] = d
    for s0, t in zip(ps, ds):
        S[:, s0:s0 + dc] = t
    if s16:
        S[:, M.Q:M.Q + dc] = ds[0] + ds[1]
    wa, ba = M.fold_a(wl1, bl1, wm1, bm1)
    assert wa.shape == (2 * dc, cin, 3, 3) and int((wa != 0).sum()) == 2 * 3 * dc * cin and not bool(wa[:, :, 0, 0].any()) and not bool(wa[:, :, 2, 2].any())
    S[:, M.A:M.A + 2 * dc] = lrelu(F.conv2d(r, wa, ba, padding=1))
    wb, bb = M.fold_b(wl2, bl2, wm2, bm2, hi - lo, M.A - lo, [s0 - lo for s0 in ident])
    v = F.conv2d(S[:, lo:hi], wb, bb, padding=1)
    got = lrelu(v + r if j > 1 else v)
    assert bool(torch.isfinite(got).all())                        # every slot the second convolution reads is written first
    err = (got - want).abs()
    assert float(err.max()) <= 1e-12 and float(err[:, :, [0, -1], :].max()) <= 1e-12 and float(err[:, :, :, [0, -1]].max()) <= 1e-12, float(err.max())
    # teeth: a transposed pair is far away
    wt, _ = M.fold_b(wm2.transpose(2, 3), bl2, wl2.transpose(2, 3), bm2, hi - lo, M.A - lo, [s0 - lo for s0 in ident])
    assert float((lrelu(F.conv2d(S[:, lo:hi], wt, bb, padding=1) + (r if j > 1 else 0)) - want).abs().max()) > 1e-3


def test_restatement_equals_the_plain_step():
    """tests/_arfdn.py's step_ref (what the GPU tests hold the kernel to) with no rounding in between -- fp64 'storage' -- is the plain step"""
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c, cin = 25, 25
    x, ps = rn(2, cin, 5, 7), [rn(2, c, 5, 7), rn(2, c, 5, 7)]
    w = A.SimpleNamespace(d=rn(c, cin, 1, 1), bd=rn(c), l1=rn(c, cin, 3, 1), bl1=rn(c), m1=rn(c, cin, 1, 3), bm1=rn(c), l2=rn(c, c, 1, 3), m2=rn(c, c, 3, 1), b2=rn(c))
    lrelu = lambda v: F.leaky_relu(v, 0.05)
    d = lrelu(F.conv2d(x, w.d, w.bd))
    l = F.conv2d(lrelu(F.conv2d(x, w.l1, w.bl1, padding=(1, 0))), w.l2, padding=(0, 1))
    mm = F.conv2d(lrelu(F.conv2d(x, w.m1, w.bm1, padding=(0, 1))), w.m2, padding=(1, 0))
    want = lrelu(l + mm + w.b2[None, :, None, None] + x + d + ps[0] + ps[1])
    old = A.stored
    A.stored = lambda v, dt: v
    try:
        ref = A.step_ref(x, w, 0.05, True, ps, torch.bfloat16)
        wrong = A.step_ref(x, w, 0.05, True, ps, torch.bfloat16, bias_pad=True)
    finally:
        A.stored = old
    assert float((ref.out - want).abs().max()) <= 1e-12 and float((ref.d - d).abs().max()) == 0.0
    inner = (wrong.out - want).abs()[:, :, 1:-1, 1:-1]
    assert float(inner.max()) <= 1e-12 and float((wrong.out - want).abs().max()) > 1e-3


# ---- complexity and plans -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_model_complexity_equals_the_reference_model_summary(store, fuse):
    from ntire2022_esr_amd.summary import model_complexity
    assert json.load(open(os.path.join(GOLD, "summary_team14_arfdn.json"))) == WANT
    m = _arfdn(store, fuse)
    assert model_complexity(m, (3, 256, 256)) == WANT
    # ... and from the plan of that storage itself (model_complexity builds an fp32-storage plan)
    plan = _plan(m, 1, 256, 256)
    terms = [m._complexity_terms(plan, o) for o in plan.ops]
    assert [float(sum(t[i] for t in terms)) for i in range(3)] == [WANT["flops"], WANT["activations"], float(WANT["num_conv"])]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("nhw", [(1, 15, 15), (2, 45, 70), (32, 256, 256)], ids=lambda s: "x".join(str(v) for v in s))
def test_plan_shape(store, nhw):
    """Per-layer form: three launches per step on the existing kernels in every storage.  Fused form (16-bit plans): ONE asym op per step
    whose descriptor satisfies esr_asym_step_supported -- `in` and out in tensors of their own, d and the earlier maps as slices of the
    block buffer, `+ in` from the second step on -- and the rest of the plan unchanged.  fuse_asym is on by default and shapes no fp32 plan."""
    from ntire2022_esr_amd import ARFDN, _lib as L
    assert ARFDN().fuse_asym is True
    per = _arfdn(store, False)
    per._repack("cpu")
    pp = _plan(per, *nhw)
    parr, _, _ = pp.finalize((0x10000000, pp.total_lo), per._packed)
    kinds = [o.kind for o in pp.ops]
    assert kinds.count("asym") == 0 and kinds.count("apply") == 4 and kinds.count("lowres") == 4
    # (a 16-bit plan's third step has a fourth launch, q = d_2 + d_1: the existing 16-bit 3x3 takes at most 144 input slots)
    assert len(pp.ops) == (60 if store == "f32" else 61) and kinds.count("pack") == (0 if store == "f32" else 1)
    names = [o.w for o in pp.ops if o.kind == "conv"]
    for k in range(1, 5):
        for j in (1, 2, 3):
            i = names.index(f"B{k}.c{j - 1}_d")
            mid = [f"B{k}.c3_l2#q"] if (j == 3 and store != "f32") else []
            assert names[i:i + 3 + len(mid)] == [f"B{k}.c{j - 1}_d", f"B{k}.c{j}_l1#a"] + mid + [f"B{k}.c{j}_l2#b"]
    for i, o in enumerate(pp.ops):
        if o.kind == "conv" and o.k == 3 and o.hw is None and store != "f32":
            assert parr[i].conv.cin <= 144, o.w
    m = _arfdn(store, True)
    m._repack("cpu")
    plan = _plan(m, *nhw)
    arr, _, _ = plan.finalize((0x10000000, plan.total_lo), m._packed)
    fused = [(i, o) for i, o in enumerate(plan.ops) if o.kind == "asym"]
    if store == "f32":
        assert not fused and [o.kind for o in plan.ops] == kinds
        return
    assert len(fused) == 12 and len(plan.ops) == len(pp.ops) - 28 and plan.total == pp.total
    key = lambda q: (q.kind, getattr(q, "w", None))
    assert [key(q) for q in plan.ops if q.kind != "asym"] == [key(q) for q in pp.ops if not (q.kind == "conv" and (q.w.endswith(("#a", "#b", "#q", "_d"))))]
    n, h, w = nhw
    for idx, (i, o) in enumerate(fused):
        k, j = idx // 3 + 1, idx % 3 + 1
        d = arr[i].conv
        assert arr[i].kind == L.OP_ASYM_STEP == 19 and L.lib().esr_asym_step_supported(ctypes.byref(d)) == 1
        assert [q.w for q in o.replaces] == [f"B{k}.c{j - 1}_d", f"B{k}.c{j}_l1#a", f"B{k}.c{j}_l2#b"]
        assert (d.n, d.h, d.w, d.cin, d.post_cout, d.ksize) == (n, h, w, 50 if j == 1 else 25, 25, 3) and d.cout in (25, 32)
        assert d.act == d.post_act == L.ACT_LRELU and abs(d.slope - 0.05) < 1e-9 and d.res_mode == (L.RES_NONE if j == 1 else L.RES_PRE_ACT)
        assert d.storage == d.compute == L.STORE[store]
        assert d.wpacked == m._packed[f"B{k}.c{j}_l1#asym"].data_ptr() and d.post_wpacked == m._packed[f"B{k}.c{j - 1}_d#s16"].data_ptr()
        # d_1, d_2, d_3 and the earlier maps: slices 64, 32, 160 of the block buffer; out and in: other tensors
        slot = {1: 64, 2: 32, 3: 160}
        assert (d.post_out.pitch, d.post_out.coff) == (224, slot[j])
        want_p = [(224, slot[q]) for q in range(j - 1, 0, -1)]
        got_p = [(v.pitch, v.coff) for v in (d.res, d.tail_cat) if v.ptr]
        assert got_p == want_p and all(v.ptr == d.post_out.ptr for v in (d.res, d.tail_cat) if v.ptr)
        assert len({d.inp.ptr, d.out0.ptr, d.post_out.ptr}) == 3 and d.out0.coff == 0 and d.inp.coff == 0
        cost = m.op_costs(plan, arr)[i]
        assert cost["kernel"] == f"asym_step_kernel<{'true' if store == 'bf16' else 'false'}, {2 if j == 1 else 1}, {'false' if j == 1 else 'true'}>"
        cin = 50 if j == 1 else 25
        assert cost["flops"] == 2.0 * n * h * w * (cin * 25 + 6 * cin * 25 + 6 * 25 * 25)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("fuse", [False, True])
def test_op_kinds_do_not_depend_on_the_batch(store, fuse):
    m = _arfdn(store, fuse)
    kinds = [[(o.kind, getattr(o, "w", None), getattr(getattr(o, "post", None), "w", None) if o.kind == "conv" else None) for o in _plan(m, n, 45, 45).ops]
             for n in (1, 8)]
    assert kinds[0] == kinds[1]


# ---- the C ABI without a GPU ----------------------------------------------------------------------------------------------------------------
def test_asym_step_descriptor_validation_without_gpu():
    """esr_asym_step_supported / esr_asym_step validate before anything is launched (tests/_arfdn.py: check_refusals); a VALID descriptor on a
    host without a GPU passes every check and fails in the launch"""
    from ntire2022_esr_amd import _lib as L
    A.check_refusals(L, no_gpu=torch.cuda.device_count() == 0)
    assert "esr_asym_step" in L.EXPORTS and "esr_pack_asym_s16" in L.EXPORTS and "esr_unpack_asym_s16" in L.EXPORTS


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_exact_grid_cases_are_exact(store):
    """the derivation behind tests/test_gpu_arfdn.py's bit-for-bit test holds for every case it runs, and integer weights pass the packers
    unchanged"""
    for v in A.STEP_CASES:
        case = A.grid_case(store, *v)
        w, w0 = A.weights64(case.W, store), A.weights64(case.W)
        assert all(torch.equal(getattr(w, k), getattr(w0, k)) for k in vars(w)), v
        ref = A.step_ref(A.nchw(case.x), w, case.slope, case.res, [A.nchw(p) for p in case.ps], case.dt)
        assert A.grid_is_exact(case, ref, w), v
        assert float(ref.out.abs().max()) > 4 and float(ref.a_l.abs().max()) >= 1 and float(ref.a_m.abs().max()) >= 1, v


# ---- the shim, the registry, and everything else unchanged ----------------------------------------------------------------------------------
def test_shim_resolves_team14_arfdn():
    code = ("import json; from safetensors.torch import load_file; from models.team14_arfdn.ARFDN import ARFDN; "
            "m = ARFDN(); "
            f"m.load_state_dict(load_file({CKPT!r}), strict=True); import ntire2022_esr_amd as e; "
            "print(json.dumps([type(m).__module__, ARFDN is e.ARFDN, sum(p.numel() for p in m.parameters())]))")
    env = dict(os.environ, PYTHONPATH=SHIM + os.pathsep + REPO)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=SHIM, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == ["ntire2022_esr_amd.arfdn", True, 241548]


def test_select_model_serves_id_14(tmp_path):
    """`harness --model_id 14`: the reference's name and data_range (tests/golden/registry.json); the checkpoint from a model_zoo whose keys
    carry test_demo.py's `module.` prefix, or the unrounded fixture; supported_ids() -- the ids with weights under weights/ -- is unchanged"""
    from safetensors.torch import load_file
    from ntire2022_esr_amd import ARFDN, registry
    ref = json.load(open(os.path.join(GOLD, "registry.json")))["14"]
    m, name, dr, tile = registry.select_model(14, "cpu")
    assert isinstance(m, ARFDN) and name == ref["name"] == "14_ARFDN" and dr == ref["data_range"] == 1.0 and tile is None
    assert 14 not in registry.supported_ids() and 14 not in registry._entries()
    true = load_file(os.path.join(GOLD, "team14_arfdn_f32.safetensors"))
    assert all(torch.equal(v, true[k]) for k, v in m.state_dict().items())
    torch.save({"module." + k: v for k, v in true.items()}, str(tmp_path / "team14_arfdn.pth"))
    m2, _, _, _ = registry.select_model(14, "cpu", model_zoo=str(tmp_path))
    assert all(torch.equal(v, true[k]) for k, v in m2.state_dict().items())
