"""-m gpu: esr_conv_prelu (conv_prelu_kernel) and esr_mdsa_gate (mdsa_gate_kernel, csrc/esr_mdsa.hip) against their fp64 restatements, and MDGN
(NTIRE 2022 ESR team 24) end to end against the reference's goldens (tools/gen_golden_mdgn.py) in fp32, bf16 and fp16 storage, per layer and
with either fused launch.  CPU side: tests/_mdgn.py, tests/test_mdgn.py."""
import os

import numpy as np
import pytest
import torch

import _guarded as G
import _mdgn as M
import _poison as P
import _resdn as R
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAME = M.NAME
STORES = ["f32", "bf16", "f16"]
KINDS_16 = ["bf16", "f16"]
BUDGET = M.BUDGET
MAX_REL = M.max_rel()                                       # from the reference's own 16-bit emulation (tests/_mdgn.py), not from the engine
SENTINEL = 777.0
TF = {"bf16": "true", "f16": "false"}


# ---- esr_conv_prelu ------------------------------------------------------------------------------------------------------------------------
def _run_conv(case, x_pitch=64, x_coff=0, nan=False):
    """the launch through ops.conv_prelu under kernel_trace; x in a tensor of pitch x_pitch from x_coff, y in channels 8 .. 71 of an 80-wide
    tensor.  nan: every slot that is no input is NaN"""
    from ntire2022_esr_amd import ops
    dt = case["dt"]
    n, h, w, _ = case["x"].shape
    x = torch.full((n, h, w, x_pitch), float("nan") if nan else 0.0).to(dt)
    x[..., x_coff:x_coff + 64] = case["x"]
    y = torch.full((n, h, w, 80), SENTINEL, dtype=dt).to(DEV)
    with ops.kernel_trace() as names:
        yy = ops.conv_prelu(x.to(DEV), case["w"], case["b"], case["a"], x_coff=x_coff, out=y, out_coff=8)
    torch.cuda.synchronize()
    assert names == [f"conv_prelu_kernel<{TF[case['store']]}>"], names
    yc = yy.cpu()
    assert bool((yc[..., :8] == SENTINEL).all()) and bool((yc[..., 72:] == SENTINEL).all()), "y's tensor outside its slice"
    return yc[..., 8:72]


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("hw", M.CONV_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_conv_prelu_is_bit_exact_on_the_exact_grid(store, hw):
    """inputs and sparse weights in {-1, 0, 1}, integer biases, slopes from {-2, -1/2, 1/2, 2}: the CPU asserts every partial sum exact and every
    value representable (tests/_mdgn.py: conv_grid_is_exact), then the result equals the fp64 restatement bit for bit"""
    case = M.conv_case("grid", store, hw)
    ref = M.conv_case_ref(case)
    assert M.conv_grid_is_exact(case, ref) and float(ref["f"].abs().max()) >= 2 and bool((ref["v"] < 0).any())
    y = _run_conv(case)
    assert torch.equal(y.double(), ref["f"]), float((y.double() - ref["f"]).abs().max())


@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("hw", M.CONV_SIZES, ids=lambda v: f"{v[0]}x{v[1]}")
def test_conv_prelu_matches_fp64_restatement(store, hw):
    """random data, slopes with negatives and values above 1, against the restatement on the blob's effective weights within the one-store
    bound; NaN in every slot that is no input changes no bit"""
    case = M.conv_case("random", store, hw)
    assert int((case["a"] < 0).sum()) and int((case["a"] > 1).sum())
    ref = M.conv_case_ref(case)
    bound = M.one_store_bound(ref["f_raw"], case["dt"])
    y = _run_conv(case)
    ratio = float(((y.double() - ref["f_raw"]).abs() / bound).max())
    print(f"conv_prelu {store} {hw}: {ratio:.2f} of the one-store bound")
    assert ratio <= 1, ratio
    y2 = _run_conv(case, x_pitch=88, x_coff=16, nan=True)
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("store", KINDS_16)
def test_conv_prelu_is_not_max_v_av(store):
    """with every slope above 1 the max(v, a v) reading is more than 30 bounds away -- shown on the CPU --, and the kernel is held to
    v >= 0 ? v : a v"""
    case = M.conv_case("random", store, (16, 17), seed=3)
    case["a"] = case["a"].abs() + 1.25
    ref = M.conv_case_ref(case)
    w, b = M.conv_effective(case)
    wrong = M.conv_prelu_max_ref(case["x"], w, b, case["a"])
    bound = M.one_store_bound(ref["f_raw"], case["dt"])
    assert float(((wrong - ref["f_raw"]).abs() / bound).max()) > 30
    y = _run_conv(case)
    assert bool(((y.double() - ref["f_raw"]).abs() <= bound).all())


@pytest.mark.parametrize("store", KINDS_16)
def test_conv_prelu_pads_with_zeros_not_with_prelu_of_the_bias(store):
    """bias 3 on the exact grid: the CPU first shows that the two readings of the ring around the image -- 0, or prelu(b) -- differ on the
    border only; the kernel equals the zero-padded one bit for bit"""
    case = M.conv_case("grid", store, (16, 17), bias=3.0)
    ref, ringed = M.conv_case_ref(case), M.conv_case_ref(case, pad="prelu_bias")
    assert M.conv_grid_is_exact(case, ref)
    diff = (ref["f"] - ringed["f"]).abs()
    assert float(diff[:, 1:-1, 1:-1].max()) == 0 and float(diff.max()) >= 1
    y = _run_conv(case)
    assert torch.equal(y.double(), ref["f"])


@pytest.mark.parametrize("store", KINDS_16)
def test_conv_prelu_stays_inside_its_views(store):
    """tests/_guarded.py: NaN in front of and behind x and in every slot of its tensor that is no input, sentinel bytes around and inside y's
    tensor, of which only the 64 channels are declared writable: at 33 x 18 (halo loads next to the last pixel, ragged tiles) and at a single
    pixel no NaN reaches the result, it equals the plain run bit for bit, and no other byte changes"""
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    for hw in ((33, 18), (1, 1)):
        case = M.conv_case("random", store, hw)
        y0 = _run_conv(case)
        n, (h, w) = 2, hw
        x = torch.full((n, h, w, 80), float("nan")).to(dt)
        x[..., 8:72] = case["x"]
        arena = G.Arena(DEV, fill="nan")
        arena.add_input("x", x)
        arena.add_output("y", (n, h, w, 96), dt, writable=(-1, 16, 64))
        arena.build()
        ops.conv_prelu(arena["x"], case["w"], case["b"], case["a"], x_coff=8, out=arena["y"], out_coff=16)
        arena.check_untouched()
        y = arena.written("y").cpu()
        assert bool(torch.isfinite(y.float()).all()) and torch.equal(y.view(torch.int16), y0.contiguous().view(torch.int16))


def test_conv_prelu_refusals_launch_nothing():
    from ntire2022_esr_amd import _lib as L, ops
    case = M.conv_case("grid", "bf16", (4, 5))
    args = [case[k] for k in ("w", "b", "a")]
    x = case["x"].to(DEV)
    big = torch.zeros(2, 4, 5, 128, dtype=torch.bfloat16, device=DEV)
    ops.conv_prelu(big, *args, x_coff=0, out=big, out_coff=64)                          # disjoint channel slices of one pixel grid are fine
    with pytest.raises(L.EsrError):                                                     # y over x: the neighbouring tiles read x as halo
        ops.conv_prelu(x, *args, out=x)
    with pytest.raises(L.EsrError):                                                     # ... as channel ranges of one tensor too
        ops.conv_prelu(big, *args, x_coff=0, out=big, out_coff=32)
    with pytest.raises(L.EsrError):                                                     # coff is not whole granules
        ops.conv_prelu(big, *args, x_coff=4)
    with pytest.raises(L.EsrError):                                                     # the view does not hold 64 channels
        ops.conv_prelu(big, *args, x_coff=72)
    with pytest.raises(L.EsrError):                                                     # another width
        ops.conv_prelu(x, torch.zeros(48, 64, 3, 3), torch.zeros(48), torch.zeros(48))
    with pytest.raises(L.EsrError):                                                     # fp32 storage
        ops.conv_prelu(x.float(), *args)
    with pytest.raises(L.EsrError):
        ops.conv_prelu(x.cpu(), *args)


# ---- esr_mdsa_gate -------------------------------------------------------------------------------------------------------------------------
GATE_PARAMS = [pytest.param(s, id="x".join(map(str, s))) for s in M.GATE_SHAPES]
FORMS_F = ["one_view", "planar"]


def _run_gate(case, form, nan=False):
    """the launch through ops.mdsa_gate under kernel_trace.  one_view: f as 192 channels from 8 of a 208-wide tensor; planar: three dense
    72-wide tensors a stride apart, 64 channels from 8.  x: 64 channels from 16 of an 88-wide tensor; y: channels 8 .. 71 of an 80-wide one.
    nan: every slot that is no input is NaN"""
    from ntire2022_esr_amd import ops
    dt = case["dt"]
    n, h, w, _ = case["x"].shape
    fill = float("nan") if nan else 0.0
    if form == "planar":
        f = M.stacked(case["f"], 72, 8, fill)
    else:
        f = torch.full((n, h, w, 208), fill).to(dt)
        f[..., 8:200] = case["f"]
    x = torch.full((n, h, w, 88), fill).to(dt)
    x[..., 16:80] = case["x"]
    y = torch.full((n, h, w, 80), SENTINEL, dtype=dt).to(DEV)
    with ops.kernel_trace() as names:
        yy = ops.mdsa_gate(f.to(DEV), x.to(DEV), case["w_f"], case["b_f"], case["a_f"], case["w_s"], case["b_s"], f_coff=8, x_coff=16, out=y, out_coff=8)
    torch.cuda.synchronize()
    assert names == [f"mdsa_gate_kernel<{TF[case['store']]}>"], names
    yc = yy.cpu()
    assert bool((yc[..., :8] == SENTINEL).all()) and bool((yc[..., 72:] == SENTINEL).all()), "y's tensor outside its slice"
    return yc[..., 8:72]


@pytest.mark.parametrize("form", FORMS_F)
@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("shape", GATE_PARAMS)
def test_mdsa_gate_is_bit_exact_on_the_exact_grid(store, shape, form):
    """w_s = 0, b_s = 0: the CPU asserts s = 1/2 exactly and every sum exact; y = store(f / 2) bit for bit"""
    case = M.gate_case("grid", store, shape, gate=False)
    ref = M.gate_case_ref(case)
    assert M.gate_grid_is_exact(case, ref) and bool((ref["raw"] < 0).any())
    y = _run_gate(case, form)
    assert torch.equal(y.double(), ref["y"]), float((y.double() - ref["y"]).abs().max())


@pytest.mark.parametrize("form", FORMS_F)
@pytest.mark.parametrize("store", KINDS_16)
@pytest.mark.parametrize("shape", GATE_PARAMS)
def test_mdsa_gate_matches_fp64_restatement(store, shape, form):
    """random data (gate arguments within +-8), slopes with negatives and values above 1, against fp64 on the blob's effective weights within
    the one-store bound; NaN in every slot that is no input changes no bit"""
    case = M.gate_case("random", store, shape)
    assert int((case["a_f"] < 0).sum()) and int((case["a_f"] > 1).sum())
    ref = M.gate_case_ref(case)
    bound = M.one_store_bound(ref["y_raw"], case["dt"])
    y = _run_gate(case, form)
    ratio = float(((y.double() - ref["y_raw"]).abs() / bound).max())
    print(f"mdsa_gate {store} {shape} {form}: {ratio:.2f} of the one-store bound, |arg|max {float(ref['arg'].abs().max()):.2f}")
    assert ratio <= 1, ratio
    y2 = _run_gate(case, form, nan=True)
    assert torch.equal(y2.view(torch.int16), y.view(torch.int16))


@pytest.mark.parametrize("store", KINDS_16)
def test_mdsa_gate_prelu_is_not_max_v_av(store):
    case = M.gate_case("random", store, (1, 17, 33), seed=5)
    case["a_f"] = case["a_f"].abs() + 1.25
    ref, wrong = M.gate_case_ref(case), M.gate_case_ref(case, act=R.prelu_max_f64)
    bound = M.one_store_bound(ref["y_raw"], case["dt"])
    assert float(((wrong["y_raw"] - ref["y_raw"]).abs() / bound).max()) > 30
    y = _run_gate(case, "planar")
    assert bool(((y.double() - ref["y_raw"]).abs() <= bound).all())


@pytest.mark.parametrize("form", FORMS_F)
@pytest.mark.parametrize("store", KINDS_16)
def test_mdsa_gate_stays_inside_its_views(store, form):
    """tests/_guarded.py: NaN around the sources and in every slot of their tensors that is no input, sentinel bytes around and inside y's tensor;
    at 17 x 33 (a ragged last group of 16 pixels) and at a single pixel no NaN reaches the result and no byte outside y's 64 channels changes"""
    from ntire2022_esr_amd import ops
    dt = R.DT[store]
    for shape in ((1, 17, 33), (1, 1, 1)):
        case = M.gate_case("random", store, shape)
        y0 = _run_gate(case, form)
        n, h, w = shape
        if form == "planar":
            f = M.stacked(case["f"], 72, 8, float("nan"))
        else:
            f = torch.full((n, h, w, 208), float("nan")).to(dt)
            f[..., 8:200] = case["f"]
        x = torch.full((n, h, w, 88), float("nan")).to(dt)
        x[..., 16:80] = case["x"]
        arena = G.Arena(DEV, fill="nan")
        arena.add_input("f", f)
        arena.add_input("x", x)
        arena.add_output("y", (n, h, w, 96), dt, writable=(-1, 16, 64))
        arena.build()
        ops.mdsa_gate(arena["f"], arena["x"], case["w_f"], case["b_f"], case["a_f"], case["w_s"], case["b_s"], f_coff=8, x_coff=16, out=arena["y"], out_coff=16)
        arena.check_untouched()
        y = arena.written("y").cpu()
        assert bool(torch.isfinite(y.float()).all()) and torch.equal(y.view(torch.int16), y0.contiguous().view(torch.int16))


def test_mdsa_gate_refusals_launch_nothing():
    from ntire2022_esr_amd import _lib as L, ops
    case = M.gate_case("grid", "bf16", (1, 3, 5))
    args = [case[k] for k in ("w_f", "b_f", "a_f", "w_s", "b_s")]
    f, x = case["f"].to(DEV), case["x"].to(DEV)
    ops.mdsa_gate(f, x, *args)
    fat = torch.zeros(1, 3, 5, 256, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.EsrError):                                                     # y in a source's tensor, even in other channels
        ops.mdsa_gate(fat, x, *args, out=fat, out_coff=192)
    with pytest.raises(L.EsrError):                                                     # y over x
        ops.mdsa_gate(f, x, *args, out=x)
    st = M.stacked(case["f"]).to(DEV)
    with pytest.raises(L.EsrError):                                                     # y over f3 of the planar form
        ops.mdsa_gate(st, x, *args, out=st[2])
    with pytest.raises(L.EsrError):                                                     # coff is not whole granules
        ops.mdsa_gate(fat, x, *args, f_coff=4)
    with pytest.raises(L.EsrError):                                                     # the view does not hold 192 channels
        ops.mdsa_gate(fat, x, *args, f_coff=72)
    with pytest.raises(L.EsrError):                                                     # fp32 storage
        ops.mdsa_gate(f.float(), x.float(), *args)


# ---- the network ------------------------------------------------------------------------------------------------------------------------------
_models = {}
# (compute, fuse_conv_prelu, fuse_mdsa_gate): an fp32 plan has the per-layer form only
FORMS = [("f32", False, False)] + [(c, cp, mg) for c in KINDS_16 for cp in (False, True) for mg in (False, True)]
FORM_IDS = [f"{c}-cp{int(cp)}-mg{int(mg)}" for c, cp, mg in FORMS]


def _mdgn(compute, cp=False, mg=False, true_weights=False):
    from ntire2022_esr_amd import MDGN
    key = "true" if true_weights else "m"
    if key not in _models:
        m = MDGN()
        m.load_state_dict(M.load_parts(NAME + ("_f32" if true_weights else "")), strict=True)
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.set_compute(compute)
    m.fuse_conv_prelu, m.fuse_mdsa_gate = cp, mg
    m.use_graphs = True
    return m


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _kinds(m, shape):
    return [o.kind for o in m._plans[_key(shape)].plan.ops]


def _check_form(m, shape, compute, cp, mg):
    kinds = _kinds(m, shape)
    s16 = compute != "f32"
    assert kinds.count("convprelu") == (12 if cp and s16 else 0) and kinds.count("mdsagate") == (4 if mg and s16 else 0)
    assert len(kinds) == 39 + s16 - (12 if cp and s16 else 0) - (8 if mg and s16 else 0), len(kinds)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_fp32_matches_reference_e2e(case):
    """the reference's fp32 outputs for crops of test.bmp at 0 .. 255, the 3 x 5 and the 1 x 1 image included"""
    g = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
    m = _mdgn("f32")
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"MDGN e2e {case} {tuple(x.shape)}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


_big = {}


@pytest.mark.parametrize("compute,cp,mg", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, cp, mg):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_{NAME}_{h}x{w}.npz"))
    m = _mdgn(compute, cp, mg)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"MDGN {h}x{w} {compute} conv_prelu={int(cp)} mdsa_gate={int(mg)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB "
          f"(d = {psnr - float(g['psnr']):+.4f}), max|dy|/range = {rel:.2e} (bound {MAX_REL[compute]:.2e})")
    _check_form(m, (1, 3, h, w), compute, cp, mg)
    assert bool(torch.isfinite(y).all())                    # (fp16: the reference's largest activation on this image is 4 239 < 65 504)
    _big[(h, w, compute, cp, mg)] = y[0, :, ::9, ::9].cpu().double() / dr
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    assert rel <= MAX_REL[compute], rel


@pytest.mark.parametrize("compute", KINDS_16)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_fused_against_per_layer(h, w, compute):
    """Each fused launch rounds once where the per-layer form rounds two or three times: the forms differ, and each is within MAX_REL of the
    reference (the PSNR test).  Their mutual distances are printed; two results that are each within MAX_REL of one reference are within
    twice that of each other, which is all this asserts."""
    keys = [(h, w, compute, cp, mg) for cp in (False, True) for mg in (False, True)]
    for k in keys:
        if k not in _big:
            test_psnr_against_reference_at_stated_size(*k)
    per = _big[keys[0]]
    for k in keys[1:]:
        rel = float((per - _big[k]).abs().max())
        print(f"MDGN {h}x{w} {compute}: conv_prelu={int(k[3])} mdsa_gate={int(k[4])} against per-layer max|dy|/range = {rel:.2e}")
        assert rel <= 2 * MAX_REL[compute], rel


@pytest.mark.parametrize("compute,cp,mg", FORMS, ids=FORM_IDS)
def test_batch_equals_per_image(compute, cp, mg):
    m = _mdgn(compute, cp, mg)
    x = (torch.rand(2, 3, 45, 70, generator=torch.Generator().manual_seed(45)) * 255.0).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    _check_form(m, x.shape, compute, cp, mg)
    _check_form(m, (1, 3, 45, 70), compute, cp, mg)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,cp,mg", FORMS, ids=FORM_IDS)
def test_graph_forward_equals_run_ops(compute, cp, mg):
    from ntire2022_esr_amd import _lib as L
    m = _mdgn(compute, cp, mg)
    shape = (1, 3, 40, 52)
    g = torch.Generator().manual_seed(9)
    xs = [(torch.rand(*shape, generator=g) * 255.0).to(DEV) for _ in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]
    torch.cuda.synchronize()
    ent = m._plans[shape + (torch.device(DEV),)]
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


@pytest.mark.parametrize("shape", [(1, 3, 1, 1), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,cp,mg", FORMS, ids=FORM_IDS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, cp, mg, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit"""
    m = _mdgn(compute, cp, mg)
    assert not m.rezero_on_switch
    dev = torch.device(DEV)
    x = (torch.rand(*shape, generator=torch.Generator().manual_seed(17 * shape[2] + shape[3])) * 255.0).to(DEV)
    try:
        results = []
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()                                     # a fresh context: prepare() zero-fills the workspace
            ent = m.prepare(shape, DEV)
            ctx = m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]
            assert ctx.ws_owner == _key(shape) and not bool(ctx.ws.any())
            _check_form(m, shape, compute, cp, mg)
            y0 = m(x).clone()
            if graphs:
                m(x)                                            # the second forward of a shape captures the graph; replays from here on
                assert ent.graph is not None
            assert bool(torch.isfinite(y0).all())
            results.append(y0)
            for pat in P.PATTERNS:
                ctx.ws.copy_(P.pattern(pat, ctx.ws.numel(), ctx.lo_cap, compute, shape[2]).to(DEV))      # ws_owner stays: no zero fill
                y = m(x)
                assert m._plans[_key(shape)] is ent and ctx.ws_owner == _key(shape)
                assert torch.equal(y, y0), (pat, graphs, float((y - y0).abs().max()), int((y != y0).sum()))
        assert torch.equal(results[0], results[1])
    finally:
        m.invalidate_workspaces()                               # the next forward of this model starts from zeros again


# ---- the unrounded checkpoint ---------------------------------------------------------------------------------------------------------------
_true = {}


def _true_golden():
    if "g" not in _true:
        g = dict(np.load(os.path.join(GOLD, f"true_{NAME}.npz")))
        e2e = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
        g["xb"], g["xc"] = e2e["xb"], e2e["xc"]
        g["lr"] = np.load(os.path.join(GOLD, f"big_{NAME}_256x256.npz"))["lr"]
        _true["g"] = g
    return _true["g"]


@pytest.mark.parametrize("case", ["b", "c"])
def test_fp32_matches_reference_e2e_true_weights(case):
    g = _true_golden()
    m = _mdgn("f32", true_weights=True)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x" + case]).to(DEV)).cpu().numpy()
    err = float(np.abs(y.astype(np.float64) - g["y" + case]).max())
    print(f"MDGN true weights e2e {case}: max|y - ref| = {err:.3e}")
    assert err <= 2e-5 * max(1.0, float(np.abs(g["y" + case]).max())), err


@pytest.mark.parametrize("compute,cp,mg", FORMS, ids=FORM_IDS)
def test_true_weights_at_256(compute, cp, mg):
    """the 256 x 256 image with the unrounded checkpoint: max |dy| / range within MAX_REL plus the reference's own figure for rounding every
    weight once to the type (the generator's dw_rel_*), and the PSNR within the type's budget plus what that same rounding costs the reference
    (dw_psnr_*: -0.0256 dB in bf16 on this network, more than the budget by itself)"""
    from ntire2022_esr_amd import image_util as util
    g = _true_golden()
    m = _mdgn(compute, cp, mg, true_weights=True)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    assert y.shape == (1, 3, 1024, 1024) and bool(torch.isfinite(y).all())
    dpsnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(1024, 1024), border=4) - float(g["psnr"])
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    bound = MAX_REL[compute] + (float(g["dw_rel_" + compute]) if compute != "f32" else 0.0)
    budget = BUDGET[compute] + (abs(float(g["dw_psnr_" + compute])) if compute != "f32" else 0.0)
    print(f"MDGN true weights 256x256 {compute} conv_prelu={int(cp)} mdsa_gate={int(mg)}: dPSNR = {dpsnr:+.4f} dB (budget {budget:.4f}), "
          f"max|dy|/range = {rel:.2e} (bound {bound:.2e})")
    assert abs(dpsnr) <= budget, dpsnr
    assert rel <= bound, (rel, bound)
