"""-m gpu: ARFDN (models.team14_arfdn.ARFDN.ARFDN) on the MI355X.

  * the one-launch step (esr_asym_step, asym_step_kernel) against the fp64 restatement of tests/_arfdn.py on the values the kernel reads and
    the blobs' EFFECTIVE weights: bit for bit on an exact grid (integer-valued data, slope 1/2: derived and asserted on the CPU first, so
    the summation order cannot matter), within a derived bound on random data, the zero padding of the never-stored maps at the image
    border, nothing beyond cin or behind a tensor read, nothing outside the declared views written, the documented refusals;
  * the network against the reference's goldens (tools/gen_golden_arfdn.py): fp32 e2e vectors, PSNR at 256 x 256 and 339 x 510 in every
    storage and both forms of the step, and with the unrounded checkpoint as tests/test_gpu_true_weights.py holds the other networks;
  * the fused form against the per-layer form, a batch against its single images, graph replay against esr_run_ops."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _arfdn as A
import _poison as P
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = A.DT
NAME = "team14_arfdn"
# PSNR against the reference's, dB: the project's budgets.  The fixture checkpoint is the reference's ROUNDED TO BF16 (tools/gen_golden_arfdn.py);
# the unrounded one is held to the same budgets below
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}
# max |y - y_ref| / data_range on the big goldens' ::9 sample.  f32: the project's bound.  bf16 / f16: twice the largest value measured on the
# MI355X over both sizes and both forms of the step (bf16 1.23e-2, per-layer at 256 x 256; f16 2.05e-3, per-layer at 339 x 510);
# the result is deterministic, the margin is for other content
MAX_REL = {"f32": 2e-5, "bf16": 2.46e-2, "f16": 4.10e-3}
STEP_PARAMS = [pytest.param(*v, id=A.case_id(v)) for v in A.STEP_CASES]
WIDTH_PARAMS = [pytest.param(*wd, id="-".join(str(int(v)) for v in wd)) for wd in A.ARFDN_WIDTHS + A.NEW_WIDTHS]
TF = {True: "true", False: "false"}


def _tol(ref, dt):
    """tests/test_gpu_c64m.py's bound for one 16-bit store"""
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    return ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))


_cases = {}


def _case(kind, store, hw, cin, c, res, np_, **kw):
    """a case's inputs, weights, effective weights and restatement inputs: computed once and left unchanged"""
    key = (kind, store, hw, cin, c, res, np_, tuple(sorted(kw.items())))
    if key not in _cases:
        case = (A.grid_case if kind == "grid" else A.random_case)(store, hw, cin, c, res, np_, **kw)
        case.w = A.weights64(case.W, store)
        case.xs, case.pss = A.nchw(case.x).double(), [A.nchw(p).double() for p in case.ps]
        _cases[key] = case
    return _cases[key]


def _padded(t, pitch):
    return F.pad(t, (0, pitch - t.shape[-1])).contiguous().to(DEV)


def _run(case, pitch=None, x=None, ps=None, **kw):
    """one launch; x / ps: tensors to pass in place of the case's, padded to round_up(channels, 8)"""
    from ntire2022_esr_amd import _lib as L, ops
    W = case.W
    x = _padded(case.x, A.r8(case.cin) if pitch is None else pitch) if x is None else x
    ps = [_padded(p, A.r8(case.c)) for p in case.ps] if ps is None else ps
    pk = dict(zip(("p1", "p2"), ps))
    d, y = ops.asym_step(x, W["w_d"], W["b_d"], W["w_l1"], W["b_l1"], W["w_l2"], W["b_l2"], W["w_m1"], W["b_m1"], W["w_m2"], W["b_m2"],
                         res=case.res, act=L.ACT_LRELU, slope=case.slope, cin=case.cin, **pk, **kw)
    torch.cuda.synchronize()
    return d.cpu(), y.cpu()


def _kernel(case):
    return f"asym_step_kernel<{TF[case.store == 'bf16']}, {2 if case.cin > 32 else 1}, {TF[case.res]}>"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("hw,cin,c,res,np_", STEP_PARAMS)
def test_step_is_bit_exact_on_the_exact_grid(store, hw, cin, c, res, np_):
    """Integer-valued inputs and weights, slope 1/2: every d, a_l and a_m of the restatement is representable in the storage type and every
    partial sum exact in fp32 (A.grid_is_exact asserts both), so d and out must equal the restatement bit for bit whatever the summation
    order -- a wrong tap, a transposed pair, a missing residual or a bias-padded halo cannot hide in a tolerance."""
    from ntire2022_esr_amd import ops
    case = _case("grid", store, hw, cin, c, res, np_)
    ref = A.step_ref(case.xs, case.w, case.slope, res, case.pss, case.dt)
    assert A.grid_is_exact(case, ref, case.w)
    with ops.kernel_trace() as names:
        d, y = _run(case)
    assert names == [_kernel(case)], names
    want_d, want_y = ref.d.to(torch.float32).to(case.dt), ref.out.to(torch.float32).to(case.dt)
    got_d, got_y = A.nchw(d[..., :c]), A.nchw(y[..., :c])
    nd, ny = int((got_d.double() != want_d.double()).sum()), int((got_y.double() != want_y.double()).sum())
    print(f"grid {store} {A.case_id((hw, cin, c, res, np_))}: {nd} of {got_d.numel()} values of d and {ny} of out differ; max|out| = {float(ref.out.abs().max())}")
    assert nd == 0 and ny == 0
    assert not bool(d[..., c:].any()) and not bool(y[..., c:].any())


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("hw,cin,c,res,np_", STEP_PARAMS)
def test_step_matches_fp64_restatement(store, hw, cin, c, res, np_):
    """Random data.  d: the one-store bound.  out, restated from the d THE KERNEL STORED (the two checks are independent): that bound plus
    |W_l2| (*) ulp(a_l) + |W_m2| (*) ulp(a_m) per element -- the kernel's a_l / a_m come from fp32 sums in another order and may round to
    the neighbouring storage value.  Both outputs go into sentinel-filled tensors: pad channels zero up to the 16-byte granule, the
    sentinel intact beyond."""
    from ntire2022_esr_amd import ops
    case = _case("random", store, hw, cin, c, res, np_)
    dt, n = case.dt, case.x.shape[0]
    mk = lambda: torch.full((n, hw[0], hw[1], 48), 7.0, dtype=dt, device=DEV)
    with ops.kernel_trace() as names:
        d, y = _run(case, d_out=mk(), out=mk())
    assert names == [_kernel(case)], names
    d_stored = A.nchw(d[..., :c])
    ref = A.step_ref(case.xs, case.w, case.slope, res, case.pss, dt, d_used=d_stored)
    err_d = (d_stored.double() - ref.d).abs()
    share_d = float((err_d / _tol(ref.d, dt)).max())
    bound = _tol(ref.out, dt) + ref.extra
    err_y = (A.nchw(y[..., :c]).double() - ref.out).abs()
    print(f"step {store} {A.case_id((hw, cin, c, res, np_))}: max|d - ref| = {float(err_d.max()):.3e} ({share_d:.3f} of the bound), "
          f"max|out - ref| = {float(err_y.max()):.3e} ({float((err_y / bound).max()):.3f} of the bound; the never-stored term is at most "
          f"{float((ref.extra / bound).max()):.3f} of it)")
    assert int((err_d > _tol(ref.d, dt)).sum()) == 0, float(err_d.max())
    assert int((err_y > bound).sum()) == 0, float(err_y.max())
    for t in (d, y):
        assert torch.all(t[..., c:A.r8(c)] == 0) and torch.all(t[..., A.r8(c):] == 7.0)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("cin,c,res,np_", WIDTH_PARAMS)
def test_never_stored_maps_are_zero_padded_not_bias_padded(store, cin, c, res, np_):
    """The reference zero-pads a_l and a_m: a halo pixel outside the image is 0, not act(b_l1).  With b_l1 = b_m1 = 3 the two readings differ
    on the border by far more than the bound and by nothing inside, which the CPU-side assertion shows before the kernel is held to the
    right one."""
    hw = (33, 18)
    case = _case("random", store, hw, cin, c, res, np_, b1=3.0)
    dt = case.dt
    d, y = _run(case)
    d_stored = A.nchw(d[..., :c])
    ref = A.step_ref(case.xs, case.w, case.slope, res, case.pss, dt, d_used=d_stored)
    wrong = A.step_ref(case.xs, case.w, case.slope, res, case.pss, dt, d_used=d_stored, bias_pad=True)
    bound = _tol(ref.out, dt) + ref.extra
    border = torch.ones_like(ref.out, dtype=torch.bool)
    border[:, :, 1:-1, 1:-1] = False
    ratio = ((wrong.out - ref.out).abs() / bound)[border]
    assert float(ratio.max()) > 10.0 and float((wrong.out - ref.out).abs()[~border].max()) < 1e-9, float(ratio.max())
    err = (A.nchw(y[..., :c]).double() - ref.out).abs()
    print(f"border {store} {cin}-{c}: the bias-padded reading is off by up to {float(ratio.max()):.1f} bounds; max|out - ref| = {float(err.max()):.3e} "
          f"({float((err / bound).max()):.3f} of the bound)")
    assert int((err > bound).sum()) == 0, float(err.max())


def _nan_behind(t, pitch):
    """t [n, h, w, c] in a NaN-filled allocation: pitch `pitch` (the pad slots are NaN) and 4096 NaNs right behind the tensor"""
    n, h, w, c = t.shape
    numel = n * h * w * pitch
    flat = torch.full((numel + 4096,), float("nan"), dtype=t.dtype)
    flat[:numel].view(n, h, w, pitch)[..., :c] = t
    flat = flat.to(DEV)
    return flat, flat[:numel].view(n, h, w, pitch)


NAN_PARAMS = [pytest.param(*wd, p, id="-".join(str(int(v)) for v in wd + (p,)))
              for wd in A.ARFDN_WIDTHS + A.NEW_WIDTHS for p in sorted({A.r8(wd[0]), (wd[0] + 15) // 16 * 16})]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("cin,c,res,np_,pitch", NAN_PARAMS)
def test_nothing_beyond_the_channels_or_behind_a_tensor_is_read(store, cin, c, res, np_, pitch):
    """NaNs in the pad slots of `in` (pitch round_up(cin, 8) and round_up(cin, 16)) and of the earlier maps, and right behind every input
    tensor: the results are those of the clean run, bit for bit"""
    hw = (33, 18)
    case = _case("random", store, hw, cin, c, res, np_)
    clean_d, clean_y = _run(case, pitch=pitch)
    keep = [_nan_behind(case.x, pitch)] + [_nan_behind(p, A.r8(c) if i == 0 else A.r8(c) + 8) for i, p in enumerate(case.ps)]
    d, y = _run(case, x=keep[0][1], ps=[k[1] for k in keep[1:]])
    assert bool(torch.isfinite(d.float()).all()) and bool(torch.isfinite(y.float()).all())
    assert torch.equal(d.view(torch.int16), clean_d.view(torch.int16)) and torch.equal(y.view(torch.int16), clean_y.view(torch.int16))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("cin,c,res,np_", [pytest.param(*wd, id="-".join(str(int(v)) for v in wd)) for wd in A.ARFDN_WIDTHS])
def test_nothing_outside_the_views_is_written(store, cin, c, res, np_):
    """d as a slice of the concat tensor that holds the earlier maps, out as a slice of a tensor of its own, sentinels everywhere else in
    and right behind both: the results of the dense run inside the views, every sentinel intact -- the earlier maps included"""
    hw = (16, 17)
    case = _case("random", store, hw, cin, c, res, np_)
    dt, n = case.dt, case.x.shape[0]
    clean_d, clean_y = _run(case)
    numel = n * hw[0] * hw[1]
    cat = torch.full((numel * 128 + 4096,), 7.0, dtype=dt)
    catv = cat[:numel * 128].view(n, hw[0], hw[1], 128)
    for i, p in enumerate(case.ps):                         # p1 at slots 64 .., p2 at 96 ..; d goes to 32 ..
        catv[..., 64 + 32 * i:64 + 32 * i + c] = p
    cat = cat.to(DEV)
    catv = cat[:numel * 128].view(n, hw[0], hw[1], 128)
    before = cat.cpu().clone()
    yflat = torch.full((numel * 48 + 4096,), 7.0, dtype=dt, device=DEV)
    yv = yflat[:numel * 48].view(n, hw[0], hw[1], 48)
    _run(case, ps=[catv] * np_, **dict(zip(("p1_coff", "p2_coff"), (64, 96)[:np_])), d_out=catv, d_coff=32, out=yv, out_coff=16)
    cat, yflat = cat.cpu(), yflat.cpu()
    catv, yv = cat[:numel * 128].view(n, hw[0], hw[1], 128), yflat[:numel * 48].view(n, hw[0], hw[1], 48)
    w8 = A.r8(c)
    assert torch.equal(catv[..., 32:32 + w8].view(torch.int16), clean_d[..., :w8].view(torch.int16))
    assert torch.equal(yv[..., 16:16 + w8].view(torch.int16), clean_y[..., :w8].view(torch.int16))
    catv[..., 32:32 + w8] = before[:numel * 128].view(n, hw[0], hw[1], 128)[..., 32:32 + w8]
    assert torch.equal(cat.view(torch.int16), before.view(torch.int16))
    assert torch.all(yv[..., :16] == 7.0) and torch.all(yv[..., 16 + w8:] == 7.0) and torch.all(yflat[numel * 48:] == 7.0)


def test_refusals_launch_nothing():
    """fp32 storage, c 16 and 33, cin 65, `+ in` with cin != c, null, misaligned and too-narrow views, each overlapping output: the
    documented codes, returned before a launch (the descriptors hold stand-in addresses)"""
    from ntire2022_esr_amd import _lib as L, ops
    A.check_refusals(L, no_gpu=False)
    x = torch.zeros(1, 4, 4, 32, dtype=torch.float32, device=DEV)
    w = lambda *s: torch.zeros(*s)
    with ops.kernel_trace() as names:
        with pytest.raises(L.EsrError):
            ops.asym_step(x, w(25, 25, 1, 1), w(25), w(25, 25, 3, 1), w(25), w(25, 25, 1, 3), w(25), w(25, 25, 1, 3), w(25), w(25, 25, 3, 1), w(25))
        x16 = x.to(torch.bfloat16)
        with pytest.raises(L.EsrError):                    # out where `in` is
            ops.asym_step(x16, w(25, 25, 1, 1), w(25), w(25, 25, 3, 1), w(25), w(25, 25, 1, 3), w(25), w(25, 25, 1, 3), w(25), w(25, 25, 3, 1), w(25), out=x16)
    assert names == []


# ---- the network --------------------------------------------------------------------------------------------------------------------------
_models = {}


def _arfdn(compute, fuse, true_weights=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import ARFDN
    key = "true" if true_weights else "m"
    if key not in _models:
        m = ARFDN()
        m.load_state_dict(load_file(os.path.join(GOLD, NAME + ("_f32" if true_weights else "") + ".safetensors")), strict=True)
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.set_compute(compute)
    m.fuse_asym = fuse
    m.use_graphs = True
    return m


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-layer form only)


def _n_fused(m, shape):
    return sum(o.kind == "asym" for o in m._plans[tuple(shape) + (torch.device(DEV),)].plan.ops)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
    m = _arfdn("f32", False)
    dr = float(g["data_range"])
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"ARFDN e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * dr, err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


_big = {}


def _big_run(h, w, compute, fuse):
    """one forward per (size, form), shared by the tests below: only its figures are kept"""
    from ntire2022_esr_amd import image_util as util
    key = (h, w, compute, fuse)
    if key not in _big:
        g = np.load(os.path.join(GOLD, f"big_{NAME}_{h}x{w}.npz"))
        m = _arfdn(compute, fuse)
        dr = float(g["data_range"])
        with torch.no_grad():
            y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
        psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
        rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
        print(f"ARFDN {h}x{w} {compute} fuse_asym={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB "
              f"(d = {psnr - float(g['psnr']):+.4f}), max|dy|/range = {rel:.2e}")
        _big[key] = dict(psnr=psnr, ref=float(g["psnr"]), rel=rel, finite=bool(torch.isfinite(y).all()), n_fused=_n_fused(m, (1, 3, h, w)))
    return _big[key]


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    r = _big_run(h, w, compute, fuse)
    assert r["n_fused"] == (12 if fuse else 0) and r["finite"]
    assert abs(r["psnr"] - r["ref"]) <= BUDGET[compute]
    assert r["rel"] <= MAX_REL[compute], r["rel"]


@pytest.mark.parametrize("compute", ["bf16", "f16"])
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_fused_step_is_no_worse_than_per_layer(h, w, compute):
    """The two forms are not bit-identical (another summation order; the 3-tap weights rounded once where the folded 3x3s diffuse the rounding
    error).  The fused form's PSNR against the reference is no worse than the per-layer form's by more than the budget."""
    per, fused = _big_run(h, w, compute, False), _big_run(h, w, compute, True)
    assert fused["n_fused"] == 12 and per["n_fused"] == 0
    print(f"ARFDN {h}x{w} {compute}: |dPSNR| per-layer {abs(per['psnr'] - per['ref']):.4f}, fused {abs(fused['psnr'] - fused['ref']):.4f} dB")
    assert abs(fused["psnr"] - fused["ref"]) <= abs(per["psnr"] - per["ref"]) + BUDGET[compute]


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("hw", [64, 128])
def test_batch_equals_per_image(compute, fuse, hw):
    m = _arfdn(compute, fuse)
    x = torch.rand(2, 3, hw, hw, generator=torch.Generator().manual_seed(hw)).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    assert _n_fused(m, x.shape) == _n_fused(m, (1, 3, hw, hw)) == (12 if fuse else 0)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", [("f32", False), ("bf16", False), ("bf16", True), ("f16", True)])
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _arfdn(compute, fuse)
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
    ent = m._plans[shape + (torch.device(DEV),)]
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


@pytest.mark.parametrize("shape", [(1, 3, 15, 15), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit.  The per-layer form's
    second convolutions read slots of the block buffer that nothing writes (the last 8 of a_l a_m's 64) against zero weights; the fused
    plans never touch them"""
    m = _arfdn(compute, fuse)
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
            assert _n_fused(m, shape) == (12 if fuse else 0)
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


# ---- the unrounded checkpoint (tests/test_gpu_true_weights.py's checks for this network) ------------------------------------------------------
_true = {}


def _true_golden():
    if "g" not in _true:
        g = dict(np.load(os.path.join(GOLD, f"true_{NAME}.npz")))
        e2e = np.load(os.path.join(GOLD, f"e2e_{NAME}.npz"))
        g["xb"], g["xc"] = e2e["xb"], e2e["xc"]
        g["lr"] = np.load(os.path.join(GOLD, f"big_{NAME}_256x256.npz"))["lr"]
        _true["g"] = g
    return _true["g"]


def _true_big(m, g, batch):
    from ntire2022_esr_amd import image_util as util
    dr = float(g["data_range"])
    x = util.uint2tensor4(g["lr"], dr).to(DEV)
    with torch.no_grad():
        y = m(x.repeat(batch, 1, 1, 1).contiguous())
    assert y.shape == (batch, 3, 1024, 1024) and bool(torch.isfinite(y).all())
    psnr = util.calculate_psnr(util.tensor2uint(y[0:1], dr), _hr(1024, 1024), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    return y, psnr - float(g["psnr"]), rel


@pytest.mark.parametrize("case", ["b", "c"])
def test_fp32_matches_reference_e2e_true_weights(case):
    g = _true_golden()
    m = _arfdn("f32", False, true_weights=True)
    with torch.no_grad():
        y = m(torch.from_numpy(g["x" + case]).to(DEV)).cpu().numpy()
    err = float(np.abs(y.astype(np.float64) - g["y" + case]).max())
    print(f"ARFDN true weights e2e {case}: max|y - ref| = {err:.3e}")
    assert err <= 2e-5 * float(g["data_range"]), err


def test_fp32_matches_reference_at_256_true_weights():
    g = _true_golden()
    y, dpsnr, rel = _true_big(_arfdn("f32", False, true_weights=True), g, 1)
    mean = float(y.double().mean().item())
    print(f"ARFDN true weights 256x256 f32: dPSNR = {dpsnr:+.4f} dB, max|dy|/range = {rel:.2e}, mean {mean:.6f} vs {float(g['sr_mean']):.6f}")
    assert rel < 2e-5 and abs(dpsnr) <= 0.002 and abs(mean - float(g["sr_mean"])) <= 2e-5 * float(g["data_range"])


@pytest.mark.parametrize("compute,fuse", FORMS[1:])
def test_16bit_plans_with_true_weights(compute, fuse):
    """a batch of two copies of the 256 x 256 image: bit-identical outputs, the PSNR budget of the type, and max |dy| / range within the
    bound measured with exact weights plus the reference's own figure for rounding every weight once to the type"""
    g = _true_golden()
    m = _arfdn(compute, fuse, true_weights=True)
    y, dpsnr, rel = _true_big(m, g, 2)
    bound = MAX_REL[compute] + float(g["dw_rel_" + compute])
    print(f"ARFDN true weights 2x256x256 {compute} fuse_asym={int(fuse)}: dPSNR = {dpsnr:+.4f} dB (budget {BUDGET[compute]}), "
          f"max|dy|/range = {rel:.2e} (bound {MAX_REL[compute]:.2e} + {float(g['dw_rel_' + compute]):.2e})")
    assert _n_fused(m, (2, 3, 256, 256)) == (12 if fuse else 0)
    assert torch.equal(y[0], y[1]), float((y[0] - y[1]).abs().max())
    assert abs(dpsnr) <= BUDGET[compute], dpsnr
    assert rel <= bound, (rel, bound)
