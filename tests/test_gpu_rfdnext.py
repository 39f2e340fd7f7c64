"""-m gpu: RFDNeXt (models.team38_rfdnext.RFDN.RFDN) on the MI355X.

  * the depthwise 7x7 (esr_dwconv7x7, dwconv7x7_kernel) in fp32, bf16 and fp16 storage against an fp64 F.conv2d(groups=C) restatement;
  * the one-launch ConvNeXt block (esr_cx_block_s16, cx_block_kernel) against an fp64 restatement that rounds where the kernel rounds -- t, the
    activated hidden tensor, the result -- on the blobs' EFFECTIVE weights (the 1x1 weights rounded once to the storage type), and against
    the per-op form (dwconv7x7, 1x1 + lrelu in output-channel slices, 1x1 + v).  The fused kernel is NOT bit-identical to the per-op form (its
    1x1 weights are rounded once, conv_s16_kernel multiplies by hi + lo pairs), so both are held to the one-rounding bound of their own
    restatement; zero padding of v, views, pad slots, aliasing;
  * the network against the reference's goldens (tools/gen_golden_rfdnext.py): fp32 e2e vectors, PSNR at 256 x 256 and 339 x 510 in every
    storage and both forms of the ConvNeXt block; a batch against its single images, graph replay against esr_run_ops, and no dependence on
    what the workspace held before."""
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
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SLOPE = 0.05
# PSNR against the reference's, dB: the project's budgets.  The fixture checkpoint is the reference's ROUNDED TO BF16 (tools/gen_golden_rfdnext.py), so
# nothing here sees a weight the storage types cannot hold; tests/test_gpu_true_weights.py holds the same budgets with the unrounded checkpoint
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}
# (n, h, w): smaller than the halo, every pixel a border pixel; exactly one tile; one-pixel partial tiles, three tiles across; a batch
SIZES = [(1, 5, 9), (1, 16, 16), (1, 17, 33), (2, 20, 36)]
SIZE_IDS = [f"{n}x{h}x{w}" for n, h, w in SIZES]
WIDTHS = [(50, 200), (33, 129), (64, 256)]            # RFDNeXt's, and both ends of each accepted range


def _tol(ref, dt):
    """tests/test_gpu_c64m.py's bound for one 16-bit store; for fp32 the suite's 2e-5 of the largest value"""
    if dt == torch.float32:
        return torch.full_like(ref, 2e-5 * max(1.0, float(ref.abs().max())))
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    return ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))


def _r8(c):
    return (c + 7) // 8 * 8


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


def _rnd(t, dt):
    """one rounding to the storage type, as fp64"""
    return t.to(dt).double()


def _dw7_ref(x, w0, b0, pad_value=None):
    """fp64 nn.Conv2d(C, C, 7, 1, 3, groups=C) on NCHW x; pad_value: per-channel values for the out-of-image ring instead of zeros"""
    c = x.shape[1]
    if pad_value is None:
        return F.conv2d(x, w0.double(), b0.double(), padding=3, groups=c)
    p = pad_value.double().view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2] + 6, x.shape[3] + 6).clone()
    p[:, :, 3:-3, 3:-3] = x
    return F.conv2d(p, w0.double(), b0.double(), groups=c)


_cases = {}


def _case(store, nhw, c=50, m=200, bias=None, seed=0):
    """v rounded to the storage type, the weights, the 1x1 weights as the fused kernel's blobs hold them (rounded once) -- computed once per
    case and left unchanged.  bias: a large dw7 bias (the border case), the first 1x1 small: at |t| ~ 3 the hidden values would reach 8, where
    ONE 16-bit step of a hidden value, which no launch stores, times a weight of the second 1x1 is larger than the bound of the result.
    seed: other data of the same kind (tests/_walk_cases.py)"""
    key = (store, nhw, c, m, bias, seed)
    if key not in _cases:
        n, h, w = nhw
        g = torch.Generator().manual_seed(10000 * c + 100 * h + w + (store == "f16") + (7 if bias else 0) + 1000003 * seed)
        dt = DT[store]
        x = torch.randn(n, h, w, c, generator=g).to(dt)
        rnd = lambda *s: torch.randn(*s, generator=g)
        w0, b0 = rnd(c, 1, 7, 7) * 0.1, rnd(c) * 0.1
        w1, b1 = rnd(m, c, 1, 1) * 0.1, rnd(m) * 0.1
        w2, b2 = rnd(c, m, 1, 1) * 0.05, rnd(c) * 0.1
        if bias is not None:
            b0, w1 = torch.full((c,), float(bias)), w1 * 0.1
        _cases[key] = dict(x=x, w=(w0, b0, w1, b1, w2, b2), w1e=w1.to(dt).double() if store != "f32" else w1.double(),
                           w2e=w2.to(dt).double() if store != "f32" else w2.double())
    return _cases[key]


def _cx_ref(c, dt, t_stored=None, w1=None, w2=None, pad_value=None):
    """fp64 restatement of the block, rounded where the kernel stores: t (or `t_stored`, NCHW, what a launch stored), the activated hidden
    tensor, and the UNROUNDED result (the bound is for its one rounding).  w1 / w2: effective 1x1 weights (default: rounded once)"""
    w0, b0, _, b1, _, b2 = c["w"]
    w1 = c["w1e"] if w1 is None else w1
    w2 = c["w2e"] if w2 is None else w2
    x = _nchw(c["x"])
    t = _rnd(_dw7_ref(x, w0, b0, pad_value), dt) if t_stored is None else t_stored.double()
    h = _rnd(F.leaky_relu(F.conv2d(t, w1, b1.double()), SLOPE), dt)
    return F.conv2d(h, w2, b2.double()) + x


def _padded(x, pitch):
    return F.pad(x, (0, pitch - x.shape[-1])).contiguous()


# ---- the depthwise 7x7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("c", [50, 1, 64])
@pytest.mark.parametrize("nhw", SIZES, ids=SIZE_IDS)
def test_dwconv7x7_matches_fp64(store, c, nhw):
    from ntire2022_esr_amd import ops
    cs = _case(store, nhw, c=c, m=132)
    dt = DT[store]
    w0, b0 = cs["w"][:2]
    gran = 4 if store == "f32" else 8
    pitch = (c + gran - 1) // gran * gran
    out = torch.full(nhw + (pitch + gran,), 7.0, dtype=dt, device=DEV)
    with ops.kernel_trace() as names:
        y = ops.dwconv7x7(_padded(cs["x"], pitch).to(DEV), w0, b0, out=out)
    torch.cuda.synchronize()
    assert names == [f"dwconv7x7_kernel<{ {'f32': 0, 'bf16': 1, 'f16': 2}[store] }>"], names
    ref = _dw7_ref(_nchw(cs["x"]), w0, b0)
    err = (_nchw(y.cpu()[..., :c]) - ref).abs()
    print(f"dw7 {store} C={c} {nhw}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
    assert int((err > _tol(ref, dt)).sum()) == 0, float(err.max())
    assert torch.all(y[..., c:pitch] == 0) and torch.all(y[..., pitch:] == 7.0)      # the pad channels up to the granule: zeros; nothing beyond


# ---- the fused block ------------------------------------------------------------------------------------------------------------------------
def _run_cx(cs, **kw):
    from ntire2022_esr_amd import ops
    c = cs["x"].shape[-1]
    y = ops.cx_block(_padded(cs["x"], _r8(c)).to(DEV), *cs["w"], slope=SLOPE, **kw)
    torch.cuda.synchronize()
    return y.cpu()


CX_CASES = [pytest.param(nhw, 50, 200, id=f"{i}-50-200") for nhw, i in zip(SIZES, SIZE_IDS)] + \
           [pytest.param(nhw, c, m, id=f"{i}-{c}-{m}") for c, m in WIDTHS[1:] for nhw, i in zip(SIZES[2:], SIZE_IDS[2:])]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("nhw,c,m", CX_CASES)
def test_cx_block_matches_fp64_restatement(store, nhw, c, m):
    """The result against the restatement that rounds t and the hidden tensor where the kernel does; t once more from what esr_dwconv7x7
    stores (the fused kernel's t is that, bit for bit: test_fused_t_equals_what_dwconv7x7_stores_bit_for_bit), which takes the first stage's
    rounding out of the chain"""
    from ntire2022_esr_amd import ops
    cs = _case(store, nhw, c=c, m=m)
    dt = DT[store]
    with ops.kernel_trace() as names:
        y = _run_cx(cs)
    assert names == [f"cx_block_kernel<{'true' if store == 'bf16' else 'false'}>"], names
    assert y.shape == nhw + (_r8(c),) and torch.all(y[..., c:] == 0)
    got = _nchw(y[..., :c])
    t = ops.dwconv7x7(_padded(cs["x"], _r8(c)).to(DEV), *cs["w"][:2])
    torch.cuda.synchronize()
    worst = []
    for name, ref in (("fp64 chain", _cx_ref(cs, dt)), ("t as stored by dwconv7x7", _cx_ref(cs, dt, t_stored=_nchw(t.cpu()[..., :c])))):
        err = (got - ref).abs()
        worst.append(float((err / _tol(ref, dt)).max()))
        print(f"cx {store} C={c} M={m} {nhw} [{name}]: max|got - ref| = {float(err.max()):.3e} ({worst[-1]:.3f} of the bound)")
    ref = _cx_ref(cs, dt, t_stored=_nchw(t.cpu()[..., :c]))
    assert int(((got - ref).abs() > _tol(ref, dt)).sum()) == 0, worst


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("nhw", SIZES, ids=SIZE_IDS)
def test_fused_t_equals_what_dwconv7x7_stores_bit_for_bit(store, nhw):
    """t never leaves the fused kernel, so the block is made to hand it out: half of v's channels are zero, the first 1x1 is the identity with
    slope 1 (hidden channel c = t_c, exactly: t is a 16-bit value), the second routes hidden channel c to an output channel of the zero half,
    where the residual adds 0 -- out = t there with no rounding on the way.  Both halves in turn cover every channel."""
    from ntire2022_esr_amd import ops
    c, m, half = 50, 200, 25
    cs = _case(store, nhw)
    w0, b0 = cs["w"][:2]
    for live, dead in ((slice(0, half), slice(half, c)), (slice(half, c), slice(0, half))):
        x = cs["x"].clone()
        x[..., dead] = 0
        xd = _padded(x, 56).to(DEV)
        w1, w2 = torch.zeros(m, c, 1, 1), torch.zeros(c, m, 1, 1)
        for k in range(half):
            w1[live.start + k, live.start + k] = 1.0                      # hidden[live channel] = t[live channel]
            w2[dead.start + k, live.start + k] = 1.0                      # out[dead channel] = that hidden channel (+ v = 0)
        y = ops.cx_block(xd, w0, b0, w1, torch.zeros(m), w2, torch.zeros(c), slope=1.0)
        t = ops.dwconv7x7(xd, w0, b0)
        torch.cuda.synchronize()
        got, want = y.cpu()[..., dead], t.cpu()[..., live]
        nd = int((got != want).sum())
        print(f"fused t {store} {nhw} channels {live.start}..{live.stop - 1}: {nd} of {want.numel()} values differ from dwconv7x7_kernel's")
        assert bool(want.abs().max() > 0.5) and torch.equal(got, want)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("nhw", SIZES, ids=SIZE_IDS)
def test_fused_and_per_op_forms_meet_their_restatements(store, nhw):
    """Not bit-identical: the per-op 1x1s multiply by esr_pack_conv_s16's hi + lo weights, the fused kernel by weights rounded once.  Each form
    is within the one-rounding bound of the restatement on ITS effective weights; kernel_trace shows which kernels ran."""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    from ntire2022_esr_amd.rfdnext import _hidden_slices
    c, m = 50, 200
    cs = _case(store, nhw)
    dt = DT[store]
    w0, b0, w1, b1, w2, b2 = cs["w"]
    xd = _padded(cs["x"], 56).to(DEV)
    with ops.kernel_trace() as names:
        t = ops.dwconv7x7(xd, w0, b0)
        hid = torch.zeros(nhw + (208,), dtype=dt, device=DEV)
        for a, wd in _hidden_slices(m, store):
            ops.conv2d(t, w1[a:a + wd], b1[a:a + wd], act=L.ACT_LRELU, slope=SLOPE, cin=c, out=hid, out_coff=a)
        y = ops.conv2d(hid, w2, b2, res=xd, res_mode=L.RES_PRE_ACT, cin=m)
        fused = ops.cx_block(xd, *cs["w"], slope=SLOPE)
    torch.cuda.synchronize()
    assert names[0].startswith("dwconv7x7_kernel<") and all(k.startswith("conv_s16_kernel<") for k in names[1:-1]) and len(names) == 7, names
    assert names[-1] == f"cx_block_kernel<{'true' if store == 'bf16' else 'false'}>", names
    w1p = unpack_conv_s16(pack_conv_s16(w1, b1, store), c, m, 1, store)[0].double()
    w2p = unpack_conv_s16(pack_conv_s16(w2, b2, store), m, c, 1, store)[0].double()
    ts = _nchw(t.cpu()[..., :c])
    hs = _nchw(hid.cpu()[..., :m])
    # the per-op form stage by stage, each on what the previous launch stored
    ref_h = F.leaky_relu(F.conv2d(ts, w1p, b1.double()), SLOPE)
    ref_y = F.conv2d(hs, w2p, b2.double()) + _nchw(cs["x"])
    for name, got, ref in (("hidden", hs, ref_h), ("out", _nchw(y.cpu()[..., :c]), ref_y)):
        err = (got - ref).abs()
        print(f"per-op {store} {nhw} {name}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
        assert int((err > _tol(ref, dt)).sum()) == 0, (name, float(err.max()))
    ref_f = _cx_ref(cs, dt, t_stored=ts)
    err = (_nchw(fused.cpu()[..., :c]) - ref_f).abs()
    d = (fused.cpu()[..., :c].double() - y.cpu()[..., :c].double()).abs()
    print(f"fused {store} {nhw}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref_f, dt)).max()):.3f} of the bound); "
          f"fused against per-op: {int((d > 0).sum())} of {d.numel()} values differ, by at most {float(d.max()):.3e}")
    assert int((err > _tol(ref_f, dt)).sum()) == 0, float(err.max())


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_v_is_zero_padded_not_bias_padded(store):
    """The 7x7 window sees v zero-padded.  With a depthwise bias of 3 a restatement whose out-of-image ring holds that bias instead is off at
    the three-pixel border by far more than the bound and nowhere else, which the CPU-side assertion shows before the kernel is held to
    the zero-padded one."""
    from ntire2022_esr_amd import ops
    nhw = (1, 17, 33)
    cs = _case(store, nhw, bias=3.0)
    dt = DT[store]
    chain = _cx_ref(cs, dt)
    wrong = _cx_ref(cs, dt, pad_value=cs["w"][1])
    border = torch.ones_like(chain, dtype=torch.bool)
    border[:, :, 3:-3, 3:-3] = False
    ratio = ((wrong - chain).abs() / _tol(chain, dt))[border]
    print(f"border {store}: the bias-padded restatement is off by up to {float(ratio.max()):.1f} x the bound at the border")
    assert float(ratio.max()) > 10.0 and float((wrong - chain).abs()[~border].max()) < 1e-9
    # t as esr_dwconv7x7 stores it is the zero-padded one, and so is the fused kernel's
    t = _nchw(ops.dwconv7x7(_padded(cs["x"], 56).to(DEV), *cs["w"][:2]).cpu()[..., :50])
    ref_t = _dw7_ref(_nchw(cs["x"]), *cs["w"][:2])
    assert int(((t - ref_t).abs() > _tol(ref_t, dt)).sum()) == 0
    ref = _cx_ref(cs, dt, t_stored=t)
    got = _nchw(_run_cx(cs)[..., :50])
    err = (got - ref).abs()
    print(f"border {store}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
    assert int((err > _tol(ref, dt)).sum()) == 0, float(err.max())


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("joint", [True, False], ids=["one-arena", "split-arenas"])
def test_nothing_outside_the_declared_views_is_read_or_written(store, joint):
    """v at channel offset 8 of a pitch-72 tensor with NaN in the foreign channels and in the guards, the result at offset 16 of a pitch-80
    tensor; the same for esr_dwconv7x7.  The pad slots 50 .. 55 of v hold a hostile finite pattern (tests/_poison.py): the result is
    what the clean input gives, bit for bit."""
    from ntire2022_esr_amd import ops
    nhw = (2, 20, 36)
    cs = _case(store, nhw)
    dt = DT[store]
    clean = _run_cx(cs)
    t_clean = ops.dwconv7x7(_padded(cs["x"], 56).to(DEV), *cs["w"][:2]).cpu()
    wide = torch.full(nhw + (72,), float("nan"), dtype=dt)
    wide[..., 8:58] = cs["x"]
    pad = P.typed_noise(wide[..., 58:64].numel() * 2, 0, store, seed=5).view(dt)
    wide[..., 58:64] = pad.view(nhw + (6,))
    arenas = [G.Arena(DEV, fill="nan", seed=4)] if joint else [G.Arena(DEV, fill="nan", seed=4), G.Arena(DEV, fill="nan", seed=5)]
    a_in, a_out = arenas[0], arenas[-1]
    a_in.add_input("v", wide)
    a_out.add_output("y", nhw + (80,), dt, writable=(-1, 16, 56))
    a_out.add_output("t", nhw + (80,), dt, writable=(-1, 24, 56))
    for a in arenas:
        a.build()
    ops.cx_block(a_in["v"], *cs["w"], slope=SLOPE, in_coff=8, out=a_out["y"], out_coff=16)
    ops.dwconv7x7(a_in["v"], *cs["w"][:2], in_coff=8, out=a_out["t"], out_coff=24)
    for a in arenas:
        a.check_untouched()
    assert torch.equal(a_out.written("y").cpu(), clean) and torch.equal(a_out.written("t").cpu(), t_clean)


def test_an_output_in_vs_tensor_is_refused():
    from ntire2022_esr_amd import ops, _lib as L
    cs = _case("bf16", (1, 16, 16))
    wide = torch.zeros(1, 16, 16, 128, dtype=torch.bfloat16, device=DEV)
    wide[..., :50] = cs["x"].to(DEV)
    with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
        ops.cx_block(wide, *cs["w"], slope=SLOPE, out=wide, out_coff=64)
    with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
        ops.dwconv7x7(wide, *cs["w"][:2], out=wide, out_coff=64)
    torch.cuda.synchronize()
    assert not bool(wide[..., 56:].any())


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
_models = {}


def _rfdnext(compute, fuse):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import RFDNeXt
    if "m" not in _models:
        m = RFDNeXt(block_type="RFDB", act_type="lrelu")
        m.load_state_dict(load_file(os.path.join(GOLD, "team38_rfdnext.safetensors")), strict=True)
        _models["m"] = m.eval().to(DEV)
    m = _models["m"]
    m.set_compute(compute)
    m.fuse_cx = fuse
    m.use_graphs = True
    return m


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-op form only)


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _n_fused(m, shape):
    return sum(o.kind == "cx" for o in m._plans[_key(shape)].plan.ops)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, "e2e_team38_rfdnext.npz"))
    m = _rfdnext("f32", False)
    dr = float(g["data_range"])
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"RFDNeXt e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * dr, err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_team38_rfdnext_{h}x{w}.npz"))
    m = _rfdnext(compute, fuse)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    assert _n_fused(m, (1, 3, h, w)) == (4 if fuse else 0)
    assert bool(torch.isfinite(y).all())
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"RFDNeXt {h}x{w} {compute} fuse_cx={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB "
          f"(d = {psnr - float(g['psnr']):+.4f}), max|dy|/range = {rel:.2e}")
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    if compute == "f32":
        assert rel <= 2e-5, rel


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_batch_equals_per_image(compute, fuse):
    m = _rfdnext(compute, fuse)
    x = torch.rand(2, 3, 40, 52, generator=torch.Generator().manual_seed(40)).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    assert _n_fused(m, x.shape) == _n_fused(m, (1, 3, 40, 52)) == (4 if fuse else 0)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", [("f32", False), ("bf16", False), ("bf16", True)])
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _rfdnext(compute, fuse)
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


@pytest.mark.parametrize("shape", [(1, 3, 5, 9), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit"""
    m = _rfdnext(compute, fuse)
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
