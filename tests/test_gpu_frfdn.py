"""-m gpu: FasterRFDN (models.team25_frfdn.FRFDN.FasterRFDN) on the MI355X.

  * the one-launch refinement cascade (esr_refine_cascade_s16, refine_cascade_kernel) against the four launches it replaces, bit for bit, and
    those four launches stage by stage against an fp64 restatement on the values each reads and the blobs' EFFECTIVE weights (zero padding of
    every stored tensor included) -- together they pin the fused kernel to the mathematics without a chained tolerance; nothing outside the
    declared views read or written;
  * the network against the reference's goldens (tools/gen_golden_frfdn.py): fp32 e2e vectors, PSNR at 256 x 256 and 339 x 510 in every
    storage and both forms of the refinement path;
  * the fused form against the per-op form, a batch against its single images, graph replay against esr_run_ops, and no dependence on what
    the workspace held before."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _guarded as G
import _poison as P
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.05
# PSNR against the reference's, dB: the project's budgets.  The fixture checkpoint is the reference's ROUNDED TO BF16 (tools/gen_golden_frfdn.py), so
# nothing here sees a weight the storage types cannot hold; tests/test_gpu_true_weights.py holds the same budgets with the unrounded checkpoint
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}
# max |y - y_ref| / data_range on the big goldens' ::9 sample.  f32: the project's bound.  bf16 / f16: twice the largest value measured on the
# MI355X over both sizes and both forms of the refinement path (bf16 7.69e-3, f16 1.34e-3, both at 339 x 510; the two forms are
# bit-identical); the result is deterministic, the margin is for other content
MAX_REL = {"f32": 2e-5, "bf16": 1.54e-2, "f16": 2.68e-3}
# smaller than the halo; a lone partial tile; one column / one row spilling into a second tile; interior tiles
SIZES = [(4, 5), (15, 15), (16, 17), (33, 18), (40, 52)]


def _tol(ref, dt):
    """tests/test_gpu_c64m.py's bound for one 16-bit store"""
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    return ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))


def _lrelu(v):
    return F.leaky_relu(v, SLOPE)


_cases = {}


def _case(store, hw, n=2, bias=None):
    """d2 rounded to the storage type, the weights, the blobs' effective weights, and what the four launches store -- computed once per case
    and left unchanged.  bias: a large positive bias on c2_r, c3_d and c3_r (the border case), every weight small"""
    key = (store, hw, n, bias)
    if key not in _cases:
        from ntire2022_esr_amd import ops, _lib as L
        from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
        g = torch.Generator().manual_seed(100 * hw[0] + hw[1] + (store == "f16") + (1000 if bias else 0))
        x = torch.randn(n, hw[0], hw[1], 32, generator=g).to(DT[store])
        rnd = lambda *s: torch.randn(*s, generator=g)
        w = [(rnd(32, 32, 3, 3) * 0.05, rnd(32) * 0.1), (rnd(16, 32, 1, 1) * 0.15, rnd(16) * 0.2),
             (rnd(16, 16, 3, 3) * 0.07, rnd(16) * 0.1), (rnd(16, 16, 3, 3) * 0.07, rnd(16) * 0.1)]
        if bias is not None:
            w = [(wt, torch.full_like(b, float(bias)) if i < 3 else b) for i, (wt, b) in enumerate(w)]
        eff = [unpack_conv_s16(pack_conv_s16(wt, b, store), wt.shape[1], wt.shape[0], wt.shape[2], store) for wt, b in w]
        # the per-op form: the four launches on the existing kernels, every 3x3 with its input as the residual
        xd = x.to(DEV)
        kw = dict(act=L.ACT_LRELU, slope=SLOPE)
        pre = dict(res_mode=L.RES_PRE_ACT)
        r2 = ops.conv2d(xd, *w[0], res=xd, **pre, **kw)
        d3 = ops.conv2d(r2, *w[1], **kw)
        r3 = ops.conv2d(d3, *w[2], res=d3, **pre, **kw)
        r4 = ops.conv2d(r3, *w[3], res=r3, **pre, **kw)
        torch.cuda.synchronize()
        flat = [t for pair in w for t in pair]
        _cases[key] = dict(x=x, w=flat, eff=eff, per_op=[t.cpu() for t in (r2, d3, r3, r4)])
    return _cases[key]


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _stage_refs(c):
    """fp64 restatement of each stage on what the previous launch STORED (zero padding = conv2d's padding): r2, d3, r3, r4"""
    (w2, b2), (wd, bd), (w3, b3), (w4, b4) = [(a.double(), b.double()) for a, b in c["eff"]]
    x = _nchw(c["x"])
    r2s, d3s, r3s, _ = [_nchw(t) for t in c["per_op"]]
    return [_lrelu(F.conv2d(x, w2, b2, padding=1) + x), _lrelu(F.conv2d(r2s, wd, bd)),
            _lrelu(F.conv2d(d3s, w3, b3, padding=1) + d3s), _lrelu(F.conv2d(r3s, w4, b4, padding=1) + r3s)]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_cascade_equals_the_four_launches_it_replaces(store, hw):
    from ntire2022_esr_amd import ops
    c = _case(store, hw)
    with ops.kernel_trace() as names:
        d3, r4 = ops.refine_cascade(c["x"].to(DEV), *c["w"], slope=SLOPE)
    torch.cuda.synchronize()
    assert names == [f"refine_cascade_kernel<{'true' if store == 'bf16' else 'false'}>"], names
    _, d3p, _, r4p = c["per_op"]
    assert d3.shape == d3p.shape == (2, hw[0], hw[1], 16) and r4.shape == r4p.shape
    nd, nr = int((d3.cpu().view(torch.int16) != d3p.view(torch.int16)).sum()), int((r4.cpu().view(torch.int16) != r4p.view(torch.int16)).sum())
    print(f"cascade {store} {hw}: {nd} of {d3p.numel()} d3 values and {nr} of {r4p.numel()} r4 values differ from the four launches")
    assert torch.equal(d3.cpu(), d3p) and torch.equal(r4.cpu(), r4p)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_per_op_stages_match_fp64_restatement(store, hw):
    c = _case(store, hw)
    dt = DT[store]
    for name, got, ref in zip(("r2", "d3", "r3", "r4"), c["per_op"], _stage_refs(c)):
        err = (_nchw(got) - ref).abs()
        print(f"per-op {store} {hw} {name}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
        assert int((err > _tol(ref, dt)).sum()) == 0, (name, float(err.max()))


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_intermediates_are_zero_padded_not_bias_padded(store):
    """The reference zero-pads the stored d3 and r3: a halo pixel outside the image is 0, not lrelu(bias).  With b = 3 on c2_r, c3_d and c3_r
    the two readings differ at the border by far more than the bound, which the CPU-side assertion shows before the kernel is held to the
    right one: bit-identical to the four launches, which are within the bound of the zero-padded restatement stage by stage."""
    from ntire2022_esr_amd import ops
    hw = (33, 18)
    c = _case(store, hw, bias=3.0)
    dt = DT[store]
    refs = _stage_refs(c)
    for name, got, ref in zip(("r2", "d3", "r3", "r4"), c["per_op"], refs):
        err = (_nchw(got) - ref).abs()
        assert int((err > _tol(ref, dt)).sum()) == 0, (name, float(err.max()))
    # the wrong restatement: the stored intermediate padded with lrelu(bias of the layer that made it) instead of 0, then a valid 3x3
    (_, _), (_, bd), (w3, b3), (w4, b4) = [(a.double(), b.double()) for a, b in c["eff"]]
    _, d3s, r3s, _ = [_nchw(t) for t in c["per_op"]]

    def bias_padded(t, b):
        p = _lrelu(b).view(1, -1, 1, 1).expand(t.shape[0], -1, t.shape[2] + 2, t.shape[3] + 2).clone()
        p[:, :, 1:-1, 1:-1] = t
        return p

    for name, src, bsrc, wt, b, ref in (("r3", d3s, bd, w3, b3, refs[2]), ("r4", r3s, b3, w4, b4, refs[3])):
        wrong = _lrelu(F.conv2d(bias_padded(src, bsrc), wt, b) + src)
        border = torch.ones_like(ref, dtype=torch.bool)
        border[:, :, 1:-1, 1:-1] = False
        ratio = ((wrong - ref).abs() / _tol(ref, dt))[border]
        print(f"border {store} {name}: the bias-padded restatement is off by up to {float(ratio.max()):.1f} x the bound at the border")
        assert float(ratio.max()) > 10.0 and float((wrong - ref).abs()[~border].max()) < 1e-9, (name, float(ratio.max()))
    d3, r4 = ops.refine_cascade(c["x"].to(DEV), *c["w"], slope=SLOPE)
    torch.cuda.synchronize()
    assert torch.equal(d3.cpu(), c["per_op"][1]) and torch.equal(r4.cpu(), c["per_op"][3])


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("joint", [True, False], ids=["one-pitch-32-tensor", "separate-tensors"])
def test_nothing_outside_the_declared_views_is_read_or_written(store, joint):
    """d2 at channel offset 16 of a pitch-64 tensor with NaN in the foreign channels, in the guards around it and behind it; d3 and r4 at
    offsets 0 and 16 of one pitch-32 tensor, or at offsets 8 and 24 of two wider ones"""
    from ntire2022_esr_amd import ops
    hw = (33, 18)
    c = _case(store, hw)
    dt = DT[store]
    n = c["x"].shape[0]
    wide = torch.full((n, hw[0], hw[1], 64), float("nan"), dtype=dt)
    wide[..., 16:48] = c["x"]
    a = G.Arena(DEV, fill="nan", seed=3)
    a.add_input("d2", wide)
    if joint:
        a.add_output("cat2", (n, hw[0], hw[1], 32), dt, writable="all")
    else:
        a.add_output("d3", (n, hw[0], hw[1], 48), dt, writable=(-1, 8, 16))
        a.add_output("r4", (n, hw[0], hw[1], 40), dt, writable=(-1, 24, 16))
    a.build()
    if joint:
        ops.refine_cascade(a["d2"], *c["w"], slope=SLOPE, in_coff=16, d3_out=a["cat2"], d3_coff=0, r4_out=a["cat2"], r4_coff=16)
    else:
        ops.refine_cascade(a["d2"], *c["w"], slope=SLOPE, in_coff=16, d3_out=a["d3"], d3_coff=8, r4_out=a["r4"], r4_coff=24)
    a.check_untouched()
    got_d3, got_r4 = (a["cat2"][..., :16], a["cat2"][..., 16:]) if joint else (a.written("d3"), a.written("r4"))
    assert torch.equal(got_d3.cpu(), c["per_op"][1]) and torch.equal(got_r4.cpu(), c["per_op"][3])


def test_an_output_in_d2s_tensor_is_refused():
    from ntire2022_esr_amd import ops, _lib as L
    c = _case("bf16", (16, 17))
    wide = torch.zeros(2, 16, 17, 64, dtype=torch.bfloat16, device=DEV)
    wide[..., :32] = c["x"].to(DEV)
    for kw in (dict(d3_out=wide, d3_coff=32), dict(r4_out=wide, r4_coff=48), dict(d3_out=wide, d3_coff=32, r4_out=wide, r4_coff=48)):
        with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
            ops.refine_cascade(wide, *c["w"], slope=SLOPE, **kw)
    torch.cuda.synchronize()
    assert not bool(wide[..., 32:].any())


_models = {}


def _frfdn(compute, fuse):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import FasterRFDN
    if "m" not in _models:
        m = FasterRFDN()
        m.load_state_dict(load_file(os.path.join(GOLD, "team25_frfdn.safetensors")), strict=True)
        _models["m"] = m.eval().to(DEV)
    m = _models["m"]
    m.set_compute(compute)
    m.fuse_cascade = fuse
    m.use_graphs = True
    return m


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-op form only)


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _n_fused(m, shape):
    return sum(o.kind == "cascade" for o in m._plans[_key(shape)].plan.ops)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, "e2e_team25_frfdn.npz"))
    m = _frfdn("f32", False)
    dr = float(g["data_range"])
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"FasterRFDN e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * dr, err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_team25_frfdn_{h}x{w}.npz"))
    m = _frfdn(compute, fuse)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    assert _n_fused(m, (1, 3, h, w)) == (4 if fuse else 0)
    assert bool(torch.isfinite(y).all())
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"FasterRFDN {h}x{w} {compute} fuse_cascade={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB "
          f"(d = {psnr - float(g['psnr']):+.4f}), max|dy|/range = {rel:.2e}")
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    assert rel <= MAX_REL[compute], rel


@pytest.mark.parametrize("compute", ["bf16", "f16"])
def test_fused_forward_equals_per_op_forward(compute):
    x = torch.rand(2, 3, 45, 70, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        m = _frfdn(compute, False)
        per_op = m(x).clone()
        assert _n_fused(m, x.shape) == 0
        m = _frfdn(compute, True)
        fused = m(x).clone()
    assert _n_fused(m, x.shape) == 4
    assert torch.equal(fused, per_op), float((fused - per_op).abs().max())


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("hw", [128, 256])
def test_batch_equals_per_image(compute, fuse, hw):
    m = _frfdn(compute, fuse)
    x = torch.rand(2, 3, hw, hw, generator=torch.Generator().manual_seed(hw)).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    assert _n_fused(m, x.shape) == _n_fused(m, (1, 3, hw, hw)) == (4 if fuse else 0)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", [("f32", False), ("bf16", False), ("bf16", True)])
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _frfdn(compute, fuse)
    shape = (1, 3, 40, 52)
    g = torch.Generator().manual_seed(9)
    xs = [torch.rand(*shape, generator=g).to(DEV) for _ in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]               # forwards 2 .. 4 are graph launches with new x / y each
    torch.cuda.synchronize()
    ent = m._plans[_key(shape)]
    assert _n_fused(m, shape) == (4 if fuse else 0)
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


@pytest.mark.parametrize("shape", [(1, 3, 15, 15), (1, 3, 24, 31), (2, 3, 45, 70)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit"""
    m = _frfdn(compute, fuse)
    assert not m.rezero_on_switch
    dev = torch.device(DEV)
    x = torch.rand(*shape, generator=torch.Generator().manual_seed(17 * shape[2] + shape[3])).to(DEV)
    try:
        results = []
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()                                     # a fresh context: prepare() zero-fills the workspace
            ent = m.prepare(shape, DEV)
            ctx = m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]
            assert ctx.ws_owner == _key(shape) and not bool(ctx.ws.any())
            assert _n_fused(m, shape) == (4 if fuse else 0)
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
