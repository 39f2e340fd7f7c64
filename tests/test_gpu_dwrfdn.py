"""-m gpu: team 35's RFDN (models.team35_rfdn.rfdn.RFDN; ntire2022_esr_amd.DWRFDN) on the MI355X.

  * the one-launch refinement path (esr_dwpw_pair_s16, dwpw_pair_kernel) against an fp64 restatement that rounds where the kernel rounds -- u1,
    h, u2, the result -- on the blobs' EFFECTIVE weights (the 1x1 weights rounded once to the storage type), and against the per-op form (two
    esr_dwconv3x3_f32 launches with their input as the residual, two 1x1s).  The fused kernel is NOT bit-identical to the per-op form (its 1x1
    weights are rounded once, conv_s16_kernel multiplies by hi + lo pairs), so both are held to the one-rounding bound of their own
    restatement.  An EXACT case besides: values on binary grids so coarse that every sum of the chain is an fp32 number whatever the order --
    there the fp64 restatement is what any correct fp32 evaluation gives, and the kernel is held to it bit for bit.  Zero padding of h,
    views, pad slots, aliasing;
  * ESA's low-resolution branch (esr_esa_unshuffle_f32) in every storage against F.pixel_unshuffle / max_pool2d / conv2d(padding=1) in fp64;
  * the network against the reference's goldens (tools/gen_golden_dwrfdn.py): fp32 e2e vectors, PSNR at 256 x 256 and 339 x 510 in every
    storage and both forms of the refinement path; a batch against its single images, graph replay against esr_run_ops, and no dependence on
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
# PSNR against the reference's, dB: the project's budgets.  The fixture checkpoint is the reference's ROUNDED TO BF16 (tools/gen_golden_dwrfdn.py), so
# nothing here sees a weight the storage types cannot hold; tests/test_gpu_true_weights.py holds the same budgets with the unrounded checkpoint
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}
# (n, h, w): smaller than the halo; every pixel a border pixel; exactly one tile; one-pixel partial tiles, three tiles across; a batch
SIZES = [(1, 1, 1), (1, 3, 5), (1, 16, 16), (1, 17, 33), (2, 20, 36)]
SIZE_IDS = [f"{n}x{h}x{w}" for n, h, w in SIZES]
WIDTHS = [50, 33, 64]                                  # the network's, and both ends of the accepted range


def _tol(ref, dt):
    """tests/test_gpu_rfdnext.py's bound for one 16-bit store; for fp32 the suite's 2e-5 of the largest value"""
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


def _padded(x, pitch):
    return F.pad(x, (0, pitch - x.shape[-1])).contiguous()


def _dw3(x, w, b, ring=None):
    """fp64 Residual(nn.Conv2d(C, C, 3, 1, 1, groups=C)) on NCHW x: dw3(x) + x.  ring: per-channel values that stand in the out-of-image ring
    instead of zeros (the WRONG padding of the border tests)"""
    c = x.shape[1]
    if ring is None:
        return F.conv2d(x, w.double(), b.double(), padding=1, groups=c) + x
    p = ring.double().view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2] + 2, x.shape[3] + 2).clone()
    p[:, :, 1:-1, 1:-1] = x
    return F.conv2d(p, w.double(), b.double(), groups=c) + x


_cases = {}


def _effective(w, b, store):
    """the 1x1 as dwpw_pair_kernel multiplies by it: read back from the blob"""
    from ntire2022_esr_amd.engine import dwpw_pw_effective, pack_dwpw_pw
    we, be = dwpw_pw_effective(pack_dwpw_pw(w, b, store), w.shape[0], store)
    return we[:, :, None, None], be


def _split(c):
    """(live, dead) channel sets of a C-channel run, both ways round: the chain lives on 4/5 of the channels, the rest carry x = 0 and zero
    weights and are where a run hands a hidden tensor out (_observe).  Both arrangements together make every channel a live one."""
    nd = max(c // 5, 1)
    idx = list(range(c))
    return [(idx[nd:], idx[:nd]), (idx[:c - nd], idx[c - nd:])]


def _case(store, nhw, c=50, bias=None, which=0):
    """x rounded to the storage type and zero on the dead channels, the weights (zero outside the live block), the 1x1 weights as the fused
    kernel's blobs hold them (rounded once) -- computed once per case and left unchanged.  bias: a large dw_a bias and ba with a small Wa
    (the border case)"""
    key = (store, nhw, c, bias, which)
    if key not in _cases:
        n, h, w = nhw
        g = torch.Generator().manual_seed(10000 * c + 100 * h + w + (store == "f16") + (7 if bias else 0) + 13 * which)
        dt = DT[store]
        live, dead = _split(c)[which]
        lv = torch.zeros(c)
        lv[live] = 1.0
        x = (torch.randn(n, h, w, c, generator=g) * lv).to(dt)
        rnd = lambda *s: torch.randn(*s, generator=g)
        vec, dwm, pwm = lv, lv.view(c, 1, 1, 1), (lv.view(c, 1) * lv.view(1, c)).view(c, c, 1, 1)
        wda, bda = rnd(c, 1, 3, 3) * 0.1 * dwm, rnd(c) * 0.1 * vec
        wa, ba = rnd(c, c, 1, 1) * 0.1 * pwm, rnd(c) * 0.1 * vec
        wdb, bdb = rnd(c, 1, 3, 3) * 0.1 * dwm, rnd(c) * 0.1 * vec
        wb, bb = rnd(c, c, 1, 1) * 0.05 * pwm, rnd(c) * 0.1 * vec
        if bias is not None:
            bda, ba, wa = float(bias) * vec, float(bias) * vec, wa * 0.1
        _cases[key] = dict(x=x, w=(wda, bda, wa, ba, wdb, bdb, wb, bb), wae=_effective(wa, ba, store)[0], wbe=_effective(wb, bb, store)[0],
                           live=live, dead=dead)
    return _cases[key]


def _run_pair(cs, w=None, slope=SLOPE, **kw):
    from ntire2022_esr_amd import ops
    c = cs["x"].shape[-1]
    y = ops.dwpw_pair(_padded(cs["x"], _r8(c)).to(DEV), *(cs["w"] if w is None else w), slope=slope, **kw)
    torch.cuda.synchronize()
    return y.cpu()


def _observe(cs, stage):
    """A hidden tensor of the fused kernel, which no launch stores, handed out EXACTLY: the stages behind it are made identities (a zero
    depthwise layer leaves its input through the residual, slope 1 makes the last activation the identity) and the last 1x1 routes live
    channel j to a dead output channel, where the block input adds 0.  Every value on the way is a 16-bit number times 1.0 plus zeros, so
    nothing is rounded again.  The stages in front are the case's own, so what comes out is what the full run computes inside.  `stage`:
    "u1" (through the ReLU as relu(u1) - relu(-u1), two runs), "h", "u2".  Returns NCHW fp64 [n, C, h, w], zero on the dead channels."""
    wda, bda, wa, ba, wdb, bdb, wb, bb = cs["w"]
    c = wda.shape[0]
    live, dead = cs["live"], cs["dead"]
    z3, z1 = torch.zeros(c, 1, 3, 3), torch.zeros(c)
    out = torch.zeros(cs["x"].shape[:3] + (c,), dtype=torch.float64)
    for k in range(0, len(live), len(dead)):
        chunk = live[k:k + len(dead)]
        route = torch.zeros(c, c, 1, 1)
        for d, j in zip(dead, chunk):
            route[d, j] = 1.0
        keep = torch.zeros(c, c, 1, 1)
        for d in dead:
            keep[d, d] = 1.0
        if stage == "u1":
            pos = _run_pair(cs, (wda, bda, route, z1, z3, z1, keep, z1), slope=1.0)
            neg = _run_pair(cs, (wda, bda, -route, z1, z3, z1, keep, z1), slope=1.0)
            got = pos.double() - neg.double()
        elif stage == "h":
            got = _run_pair(cs, (wda, bda, wa, ba, z3, z1, route, z1), slope=1.0).double()
        else:
            got = _run_pair(cs, (wda, bda, wa, ba, wdb, bdb, route, z1), slope=1.0).double()
        out[..., chunk] = got[..., dead[:len(chunk)]]
    return _nchw(out)


def _stage_refs(cs, x, u1, h, u2, wa, wb, ring_x=None, ring_h=None):
    """fp64 restatement of each stage on the stage in front AS STORED / AS OBSERVED (NCHW fp64), unrounded: the bound is for its one rounding.
    wa / wb: the effective 1x1 weights.  ring_x / ring_h: the WRONG paddings of the border case"""
    wda, bda, _, ba, wdb, bdb, _, bb = cs["w"]
    return (("u1", _dw3(x, wda, bda, ring_x)), ("h", F.relu(F.conv2d(u1, wa, ba.double()))), ("u2", _dw3(h, wdb, bdb, ring_h)),
            ("out", F.leaky_relu(F.conv2d(u2, wb, bb.double()) + x, SLOPE)))


PAIR_CASES = [pytest.param(nhw, 50, id=f"{i}-50") for nhw, i in zip(SIZES, SIZE_IDS)] + \
             [pytest.param(nhw, c, id=f"{i}-{c}") for c in WIDTHS[1:] for nhw, i in zip(SIZES[3:], SIZE_IDS[3:])]


def _check_stages(tag, cs, dt, got, wa, wb):
    """got: {"u1", "h", "u2", "out"} NCHW fp64; every stage within one rounding of its restatement on the stage in front"""
    x = _nchw(cs["x"])
    for name, ref in _stage_refs(cs, x, got["u1"], got["h"], got["u2"], wa, wb):
        err = (got[name] - ref).abs()
        print(f"{tag} {name}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
        assert int((err > _tol(ref, dt)).sum()) == 0, (tag, name, float(err.max()))


# ---- the fused refinement path --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("which", [0, 1], ids=["dead-first", "dead-last"])
@pytest.mark.parametrize("nhw,c", PAIR_CASES)
def test_dwpw_pair_stages_match_fp64_restatement(store, nhw, c, which):
    """The result AND the three hidden tensors, each against the fp64 restatement of its stage on the stage in front as the kernel holds it
    (_observe): one rounding per stage.  (A restatement of the whole chain from x alone is not a bound for a correct kernel: where fp32 and
    fp64 sums straddle a rounding boundary of u1, h or u2, one 16-bit step of a hidden value times a weight reaches the result -- an fp32
    evaluation on the CPU leaves the chain's bound in about one case of ten.)"""
    from ntire2022_esr_amd import ops
    cs = _case(store, nhw, c=c, which=which)
    dt = DT[store]
    with ops.kernel_trace() as names:
        y = _run_pair(cs)
    assert names == [f"dwpw_pair_kernel<{'true' if store == 'bf16' else 'false'}>"], names
    assert y.shape == nhw + (_r8(c),) and torch.all(y[..., c:] == 0)
    got = dict(u1=_observe(cs, "u1"), h=_observe(cs, "h"), u2=_observe(cs, "u2"), out=_nchw(y[..., :c]))
    assert float(got["h"].abs().max()) > 0.1 and float(got["u2"].abs().max()) > 0.1
    _check_stages(f"dwpw {store} C={c} {nhw}", cs, dt, got, cs["wae"], cs["wbe"])


def _grid(g, shape, step, bound):
    """seeded multiples of `step` in [-bound, bound]"""
    k = int(round(bound / step))
    return torch.randint(-k, k + 1, shape, generator=g).double() * step


EXACT_CASES = [pytest.param(nhw, 50, id=f"{i}-50") for nhw, i in zip(SIZES, SIZE_IDS)] + \
              [pytest.param(nhw, c, id=f"{i}-{c}") for c in WIDTHS[1:] for nhw, i in zip(SIZES[3:], SIZE_IDS[3:])]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("nhw,c", EXACT_CASES)
def test_dwpw_pair_exact_case_bit_for_bit(store, nhw, c):
    """The whole chain from x alone, every channel live.  Every operand on a coarse binary grid: x in steps of 1/16, the depthwise weights
    of 1/8, the 1x1 weights of 1/16, the biases of 1/4.  Then every term of every sum of the chain is a multiple of a quantum q (2^-7, 2^-11,
    2^-14, 2^-18 from stage to stage; rounding only coarsens a grid) and, as asserted here on the CPU, the sum of the terms' magnitudes stays
    below 2^24 q: every partial sum in ANY order is an fp32 number, fp32 accumulation is exact, and a correct kernel returns the fp64
    restatement rounded once -- bit for bit."""
    from ntire2022_esr_amd import ops
    n, h, w = nhw
    dt = DT[store]
    g = torch.Generator().manual_seed(77 + 100 * h + w + c)
    x = _grid(g, (n, c, h, w), 1 / 16, 2.0)
    wda, bda = _grid(g, (c, 1, 3, 3), 1 / 8, 0.25), _grid(g, (c,), 1 / 4, 0.5)
    wdb, bdb = _grid(g, (c, 1, 3, 3), 1 / 8, 0.25), _grid(g, (c,), 1 / 4, 0.5)
    wa, ba = _grid(g, (c, c, 1, 1), 1 / 16, 0.125), _grid(g, (c,), 1 / 4, 0.5)
    wb, bb = _grid(g, (c, c, 1, 1), 1 / 16, 0.125), _grid(g, (c,), 1 / 4, 0.5)
    assert torch.equal(x, _rnd(x, dt)) and torch.equal(wa, _rnd(wa, dt)) and torch.equal(wb, _rnd(wb, dt))

    def exact(terms_abs, q):
        assert float(terms_abs.max()) < 2.0 ** 24 * q, (float(terms_abs.max()), q)

    dwabs = lambda t, wd, bd: F.conv2d(t.abs(), wd.abs(), bd.abs(), padding=1, groups=c) + t.abs()
    exact(dwabs(x, wda, bda), 2.0 ** -7)
    u1 = _rnd(_dw3(x, wda, bda), dt)
    exact(F.conv2d(u1.abs(), wa.abs(), ba.abs()), 2.0 ** -11)
    hh = _rnd(F.relu(F.conv2d(u1, wa, ba)), dt)
    exact(dwabs(hh, wdb, bdb), 2.0 ** -14)
    u2 = _rnd(_dw3(hh, wdb, bdb), dt)
    exact(F.conv2d(u2.abs(), wb.abs(), bb.abs()) + x.abs(), 2.0 ** -18)
    pre = F.conv2d(u2, wb, bb) + x
    assert torch.equal(pre, pre.float().double())
    # (the activation: slope * v is rounded to fp32 by the kernel before the maximum, and once more to the storage type)
    ref = torch.fmax(pre.float(), torch.tensor(SLOPE, dtype=torch.float32) * pre.float()).to(dt)
    xd = _padded(x.permute(0, 2, 3, 1).to(dt), _r8(c)).to(DEV)
    f32 = lambda *ts: [t.float() for t in ts]
    y = ops.dwpw_pair(xd, *f32(wda, bda, wa, ba, wdb, bdb, wb, bb), slope=SLOPE)
    torch.cuda.synchronize()
    got = y.cpu()[..., :c].permute(0, 3, 1, 2)
    nd = int((got != ref).sum())
    print(f"dwpw exact {store} C={c} {nhw}: {nd} of {ref.numel()} values differ from the restatement; max|h| = {float(hh.abs().max()):.2f}, "
          f"max|u2| = {float(u2.abs().max()):.2f}, max|r| = {float(ref.double().abs().max()):.2f}")
    assert float(hh.abs().max()) > 1.0 and float(u2.abs().max()) > 1.0 and nd == 0
    assert torch.all(y[..., c:] == 0)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("nhw", SIZES, ids=SIZE_IDS)
def test_fused_and_per_op_forms_meet_their_restatements(store, nhw):
    """Not bit-identical: the per-op 1x1s multiply by esr_pack_conv_s16's hi + lo weights, the fused kernel by weights rounded once.  Each form
    is checked stage by stage on ITS effective weights, each stage on what the stage in front stored (per-op) or holds (fused: _observe);
    kernel_trace shows which kernels ran."""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    c = 50
    cs = _case(store, nhw)
    dt = DT[store]
    wda, bda, wa, ba, wdb, bdb, wb, bb = cs["w"]
    xd = _padded(cs["x"], 56).to(DEV)
    with ops.kernel_trace() as names:
        u1 = ops.dwconv3x3(xd, wda, bda, res=xd, res_mode=L.RES_PRE_ACT)
        hd = ops.conv2d(u1, wa, ba, act=L.ACT_RELU, cin=c)
        u2 = ops.dwconv3x3(hd, wdb, bdb, res=hd, res_mode=L.RES_PRE_ACT)
        y = ops.conv2d(u2, wb, bb, act=L.ACT_LRELU, slope=SLOPE, res=xd, res_mode=L.RES_PRE_ACT, cin=c)
        fused = ops.dwpw_pair(xd, *cs["w"], slope=SLOPE)
    torch.cuda.synchronize()
    assert [k.split("<")[0] for k in names] == ["dwconv3x3_kernel", "conv_s16_kernel", "dwconv3x3_kernel", "conv_s16_kernel", "dwpw_pair_kernel"], names
    wap = unpack_conv_s16(pack_conv_s16(wa, ba, store), c, c, 1, store)[0].double()
    wbp = unpack_conv_s16(pack_conv_s16(wb, bb, store), c, c, 1, store)[0].double()
    s = lambda t: _nchw(t.cpu()[..., :c])
    _check_stages(f"per-op {store} {nhw}", cs, dt, dict(u1=s(u1), h=s(hd), u2=s(u2), out=s(y)), wap, wbp)
    _check_stages(f"fused {store} {nhw}", cs, dt, dict(u1=_observe(cs, "u1"), h=_observe(cs, "h"), u2=_observe(cs, "u2"), out=s(fused)), cs["wae"], cs["wbe"])
    d = (fused.cpu()[..., :c].double() - y.cpu()[..., :c].double()).abs()
    print(f"fused against per-op {store} {nhw}: {int((d > 0).sum())} of {d.numel()} values differ, by at most {float(d.max()):.3e}")


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_h_is_zero_padded_not_bias_padded(store):
    """dw3_b sees h zero-padded: outside the image h is 0, not relu(ba); and dw3_a sees x zero-padded, not its own bias.  With both biases at
    3 and a small Wa, the restatement of u2 whose ring of h holds relu(ba), and the one of u1 whose ring of x holds the bias, are off at
    the one-pixel border by far more than the bound and nowhere else -- shown on the CPU before the kernel's u1 and u2 are held to the
    zero-padded ones (a kernel that computes h = relu(ba) on its halo ring without masking it fails here)."""
    nhw = (1, 17, 33)
    cs = _case(store, nhw, bias=3.0)
    dt = DT[store]
    got = dict(u1=_observe(cs, "u1"), h=_observe(cs, "h"), u2=_observe(cs, "u2"), out=_nchw(_run_pair(cs)[..., :50]))
    x = _nchw(cs["x"])
    right = dict(_stage_refs(cs, x, got["u1"], got["h"], got["u2"], cs["wae"], cs["wbe"]))
    wrong = dict(_stage_refs(cs, x, got["u1"], got["h"], got["u2"], cs["wae"], cs["wbe"], ring_x=cs["w"][1], ring_h=F.relu(cs["w"][3])))
    border = torch.ones_like(x, dtype=torch.bool)
    border[:, :, 1:-1, 1:-1] = False
    live = torch.zeros_like(border)
    live[:, cs["live"]] = True
    for name in ("u1", "u2"):
        ratio = ((wrong[name] - right[name]).abs() / _tol(right[name], dt))[border & live]
        print(f"border {store}: the bias-padded restatement of {name} is off by {float(ratio.min()):.1f} .. {float(ratio.max()):.1f} x the bound at the border")
        assert float(ratio.max()) > 10.0 and float((wrong[name] - right[name]).abs()[~border].max()) < 1e-9
    _check_stages(f"border {store}", cs, dt, got, cs["wae"], cs["wbe"])


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("joint", [True, False], ids=["one-arena", "split-arenas"])
def test_nothing_outside_the_declared_views_is_read_or_written(store, joint):
    """x at channel offset 8 of a pitch-72 tensor with NaN in the foreign channels and in the guards, the result at offset 16 of a pitch-80
    tensor.  The pad slots 50 .. 55 of x hold a hostile finite pattern (tests/_poison.py): the result is what the clean input gives, bit
    for bit."""
    from ntire2022_esr_amd import ops
    nhw = (2, 20, 36)
    cs = _case(store, nhw)
    dt = DT[store]
    clean = _run_pair(cs)
    wide = torch.full(nhw + (72,), float("nan"), dtype=dt)
    wide[..., 8:58] = cs["x"]
    pad = P.typed_noise(wide[..., 58:64].numel() * 2, 0, store, seed=5).view(dt)
    wide[..., 58:64] = pad.view(nhw + (6,))
    arenas = [G.Arena(DEV, fill="nan", seed=4)] if joint else [G.Arena(DEV, fill="nan", seed=4), G.Arena(DEV, fill="nan", seed=5)]
    a_in, a_out = arenas[0], arenas[-1]
    a_in.add_input("x", wide)
    a_out.add_output("y", nhw + (80,), dt, writable=(-1, 16, 56))
    for a in arenas:
        a.build()
    ops.dwpw_pair(a_in["x"], *cs["w"], slope=SLOPE, in_coff=8, out=a_out["y"], out_coff=16)
    for a in arenas:
        a.check_untouched()
    assert torch.equal(a_out.written("y").cpu(), clean)


def test_an_output_in_xs_tensor_is_refused():
    from ntire2022_esr_amd import ops, _lib as L
    cs = _case("bf16", (1, 16, 16))
    wide = torch.zeros(1, 16, 16, 128, dtype=torch.bfloat16, device=DEV)
    wide[..., :50] = cs["x"].to(DEV)
    with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
        ops.dwpw_pair(wide, *cs["w"], slope=SLOPE, out=wide, out_coff=64)
    torch.cuda.synchronize()
    assert not bool(wide[..., 56:].any())


# ---- ESA's low-resolution branch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nhw", [(1, 14, 14), (1, 15, 14), (1, 20, 27), (2, 45, 70)], ids=lambda s: "x".join(str(v) for v in s))
def test_esa_unshuffle_matches_fp64(store, nhw):
    """odd sizes are floored by the strided unshuffle; a ring of relu(bias) around 1 x 1, 2 x 3 and larger pooled maps; large biases so that
    the ring shows (some negative: relu)"""
    from ntire2022_esr_amd import ops
    n, h, w = nhw
    f = 12
    g = torch.Generator().manual_seed(1000 * h + w + (store == "f16"))
    dt = DT[store]
    c1 = torch.randn(n, h, w, 16, generator=g).to(dt)
    wt, b = torch.randn(f, 4 * f, 1, 1, generator=g) * 0.2, torch.randn(f, generator=g) * 3.0
    with ops.kernel_trace() as names:
        y = ops.esa_unshuffle(c1.to(DEV), wt, b)
    torch.cuda.synchronize()
    assert names == [f"esa_unshuffle_kernel<{ {'f32': 0, 'bf16': 1, 'f16': 2}[store] }>"], names
    x = _nchw(c1[..., :f])[:, :, :h // 2 * 2, :w // 2 * 2]
    ref = F.relu(F.conv2d(F.relu(F.max_pool2d(F.pixel_unshuffle(x, 2), 7, 3)), wt.double(), b.double(), padding=1))
    h3, w3 = (h // 2 - 7) // 3 + 1, (w // 2 - 7) // 3 + 1
    assert tuple(y.shape) == (n, h3 + 2, w3 + 2, 16) and tuple(ref.shape) == (n, f, h3 + 2, w3 + 2)
    got = _nchw(y.cpu()[..., :f])
    err = float((got - ref).abs().max())
    print(f"unshuffle {store} {nhw}: c3 {h3 + 2}x{w3 + 2}, max|got - ref| = {err:.3e}, max|ref| = {float(ref.abs().max()):.3f}")
    assert err <= 2e-5 * float(ref.abs().max())
    assert torch.all(y[..., f:] == 0)
    ring = F.relu(b.double()).view(1, f, 1)
    want = ring.float().double().view(1, f, 1, 1).expand(n, f, h3 + 2, w3 + 2)
    edge = torch.ones(h3 + 2, w3 + 2, dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    assert float(ring.max()) > 1.0 and torch.equal(got[:, :, edge], want[:, :, edge])      # all four sides of the ring: relu(bias), exactly


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
_models = {}


def _dwrfdn(compute, fuse):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import DWRFDN
    if "m" not in _models:
        m = DWRFDN()
        m.load_state_dict(load_file(os.path.join(GOLD, "team35_rfdn.safetensors")), strict=True)
        _models["m"] = m.eval().to(DEV)
    m = _models["m"]
    m.set_compute(compute)
    m.fuse_pair = fuse
    m.use_graphs = True
    return m


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-op form only)


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _n_fused(m, shape):
    return sum(o.kind == "dwpw" for o in m._plans[_key(shape)].plan.ops)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    g = np.load(os.path.join(GOLD, "e2e_team35_rfdn.npz"))
    m = _dwrfdn("f32", False)
    dr = float(g["data_range"])
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"DWRFDN e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * dr, err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_team35_rfdn_{h}x{w}.npz"))
    m = _dwrfdn(compute, fuse)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    assert _n_fused(m, (1, 3, h, w)) == (12 if fuse else 0)
    assert bool(torch.isfinite(y).all())
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"DWRFDN {h}x{w} {compute} fuse_pair={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB "
          f"(d = {psnr - float(g['psnr']):+.4f}), max|dy|/range = {rel:.2e}")
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    if compute == "f32":
        assert rel <= 2e-5, rel


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_batch_equals_per_image(compute, fuse):
    m = _dwrfdn(compute, fuse)
    x = (torch.rand(2, 3, 40, 52, generator=torch.Generator().manual_seed(40)) * 255.0).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    assert _n_fused(m, x.shape) == _n_fused(m, (1, 3, 40, 52)) == (12 if fuse else 0)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", [("f32", False), ("bf16", False), ("bf16", True)])
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _dwrfdn(compute, fuse)
    shape = (1, 3, 40, 52)
    g = torch.Generator().manual_seed(9)
    xs = [(torch.rand(*shape, generator=g) * 255.0).to(DEV) for _ in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]               # forwards 2 .. 4 are graph launches with new x / y each
    torch.cuda.synchronize()
    ent = m._plans[_key(shape)]
    assert _n_fused(m, shape) == (12 if fuse else 0)
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


@pytest.mark.parametrize("shape", [(1, 3, 14, 17), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit"""
    m = _dwrfdn(compute, fuse)
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
