"""-m gpu: RePAFDN (models.team10_repafdn.repafdn.RePAFDN; ntire2022_esr_amd.RePAFDN) on the MI355X.

  * esr_pa_gate (pa_gate_kernel), y = t * sigmoid(W . t + b) + s, in fp32, bf16 and fp16 storage against an fp64 restatement on the blob's
    EFFECTIVE weights (hi + lo in 16-bit storage) that rounds where the kernel rounds -- once, at the store: s none, single and a hi + lo
    pair, y single and a pair (its hi + lo held to the fp32 sum), gate arguments pushed to -60 and +60 through the bias (the checkpoint
    reaches -52), pad channels, views, aliasing;
  * esr_pa_tail (pa_tail_kernel), the same behind a 3x3 in ONE launch, bf16 and fp16: the hidden t handed out exactly and held to the fp64
    restatement of the 3x3, the gated result to the restatement computed from that t, an exact-grid chain bit for bit, zero padding, the
    fused against the per-op form;
  * the network against the reference's goldens (tools/gen_golden_repafdn.py): fp32 e2e vectors, PSNR at 256 x 256 and 339 x 510 in every
    storage and both forms, a batch against its single images, graph replay against esr_run_ops, no dependence on what the workspace held before, thin
    images in a batch; and the unrounded checkpoint against true_team10_repafdn.npz."""
import os

import numpy as np
import pytest
import torch

import _guarded as G
import _poison as P
from conftest import GOLD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
STEM = "team10_repafdn"
# PSNR against the reference's, dB: the project's budgets
BUDGET = {"f32": 0.002, "bf16": 0.01, "f16": 0.005}
# max |dy| / range at 256 x 256 with the UNROUNDED checkpoint, 16-bit storage: the distance that rounding the weights alone causes -- the
# REFERENCE on the CPU with every weight rounded once to the storage type against the reference with the true ones, true_team10_repafdn.npz:
# dw_rel_bf16 = 8.44e-3, dw_rel_f16 = 8.79e-4 -- plus a margin for the storage's own arithmetic.  The project's rule for that margin
# (tests/_true_weights.py) is twice the largest distance measured with exact, bf16-representable weights over both sizes and both forms;
# for this network that is 2 x 8.87e-3 (bf16) and 2 x 1.59e-3 (f16).  The margin held here is the SMALLER one of the
# table's nearest network, DWRFDN (the same frame at nf = 50): 2 x 6.99e-3 and 2 x 1.36e-3 -- the tighter of the two bounds.
DW_REL = {"bf16": 8.44e-3, "f16": 8.79e-4}
MARGIN = {"bf16": 1.40e-2, "f16": 2.72e-3}
MAX_REL = {k: DW_REL[k] + MARGIN[k] for k in DW_REL}
# (n, h, w): one pixel; fewer than 16 pixels; whole groups of 16; a ragged last group; a batch
SIZES = [(1, 1, 1), (1, 3, 5), (1, 16, 16), (1, 17, 33), (2, 20, 36)]
SIZE_IDS = [f"{n}x{h}x{w}" for n, h, w in SIZES]
WIDTHS = [48, 33, 64]                                  # the network's, and both ends of the accepted range
STORES = ["f32", "bf16", "f16"]
# (storage, kind of s): hi + lo pairs are a 16-bit storage format
S_KINDS = [pytest.param(st, k, id=f"{st}-{k}") for st in STORES for k in ("none", "single", "pair") if not (st == "f32" and k == "pair")]
GATE_CASES = [pytest.param(nhw, c, id=f"{i}-{c}") for c in WIDTHS for nhw, i in zip(SIZES, SIZE_IDS)]      # every size at every width


def _tol(ref, dt):
    """the project's bound (tests/test_gpu_dwrfdn.py): one 16-bit store; for fp32 the suite's 2e-5 of the largest value"""
    if dt == torch.float32:
        return torch.full_like(ref, 2e-5 * max(1.0, float(ref.abs().max())))
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    return ref.abs() * eps * 1.01 + 3e-5 * max(1.0, float(ref.abs().max()))


def _gran(store):
    return 4 if store == "f32" else 8


def _up(c, m):
    return (c + m - 1) // m * m


def _padded(x, pitch, value=0.0):
    return torch.nn.functional.pad(x, (0, pitch - x.shape[-1]), value=value).contiguous()


def _sigmoid(v):
    e = torch.exp(-v.abs())
    return torch.where(v < 0, e / (1.0 + e), 1.0 / (1.0 + e))


_cases = {}


def _case(store, nhw, c, bias=None):
    """t and s (single, and as a hi + lo pair of a finer value) in the storage type, W and b, and the blob's effective weights: computed
    once per case and left unchanged.  bias: every gate bias at this value, with a small W"""
    key = (store, nhw, c, bias)
    if key not in _cases:
        from ntire2022_esr_amd.engine import pa_gate_effective, pack_pa_gate
        n, h, w = nhw
        dt = DT[store]
        g = torch.Generator().manual_seed(1000 * c + 100 * h + w + 7 * STORES.index(store) + (0 if bias is None else 31))
        t = (torch.randn(n, h, w, c, generator=g) * 2.0).to(dt)
        s32 = torch.randn(n, h, w, c, generator=g) * 3.0
        s = s32.to(dt)
        s_lo = (s32 - s.float()).to(dt)
        wt, b = torch.randn(c, c, generator=g) * 0.2, torch.randn(c, generator=g)
        if bias is not None:
            wt, b = wt * 0.05, torch.full((c,), float(bias))
        we, be = pa_gate_effective(pack_pa_gate(wt, b, store), c, store)
        _cases[key] = dict(t=t, s=s, s_pair=torch.stack([s, s_lo]), w=wt, b=b, we=we, be=be)
    return _cases[key]


def _ref(cs, s=None):
    """fp64: t * sigmoid(We . t + be) (+ s), unrounded; s: fp64 or None"""
    t = cs["t"].double()
    arg = t @ cs["we"].t() + cs["be"]
    y = t * _sigmoid(arg)
    return y if s is None else y + s, arg


def _s_of(cs, kind):
    """(what ops.pa_gate takes, the value the kernel adds as fp64): none / single / a hi + lo pair summed in fp32"""
    if kind == "none":
        return None, None
    if kind == "single":
        return cs["s"], cs["s"].double()
    return cs["s_pair"], (cs["s_pair"][0].float() + cs["s_pair"][1].float()).double()


def _gate(cs, store, s=None, **kw):
    from ntire2022_esr_amd import ops
    c = cs["t"].shape[-1]
    pitch = _up(c, 8)
    sd = None if s is None else _padded(s, pitch).to(DEV)
    y = ops.pa_gate(_padded(cs["t"], pitch).to(DEV), cs["w"], cs["b"], s=sd, **kw)
    torch.cuda.synchronize()
    return y.cpu()


# ---- esr_pa_gate ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store,skind", S_KINDS)
@pytest.mark.parametrize("nhw,c", GATE_CASES)
def test_pa_gate_matches_fp64_restatement(store, nhw, c, skind):
    """single and pair outputs for every kind of s: the single result within one store of the restatement, the pair's high part equal to
    it bit for bit, the pair's hi + lo within the fp32 bound (2e-5 of the largest value) plus 2^-16 of the value itself"""
    from ntire2022_esr_amd import ops
    cs = _case(store, nhw, c)
    dt = DT[store]
    s, s64 = _s_of(cs, skind)
    ref, arg = _ref(cs, s64)
    with ops.kernel_trace() as names:
        y = _gate(cs, store, s)
    assert names == [f"pa_gate_kernel<{STORES.index(store)}>"], names
    assert y.shape == nhw + (_up(c, _gran(store)),) and y.dtype == dt and torch.all(y[..., c:] == 0)
    err = (y[..., :c].double() - ref).abs()
    print(f"pa_gate {store} C={c} {nhw} s={skind}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound), "
          f"arguments {float(arg.min()):.1f} .. {float(arg.max()):.1f}")
    assert int((err > _tol(ref, dt)).sum()) == 0
    if store == "f32":
        return
    yp = _gate(cs, store, s, pair_out=True)
    assert yp.shape == (2,) + nhw + (_up(c, 8),) and torch.all(yp[..., c:] == 0)
    assert torch.equal(yp[0], y)
    both = yp[0].double() + yp[1].double()
    err = (both[..., :c] - ref).abs()
    bound = _tol(ref, torch.float32) + ref.abs() * 2.0 ** -16
    print(f"pa_gate {store} C={c} {nhw} s={skind} pair: max|hi + lo - ref| = {float(err.max()):.3e} ({float((err / bound).max()):.3f} of the bound)")
    assert int((err > bound).sum()) == 0
    # the split rule of ESR_HILO_OUT: hi = rnd(v), so the low part is at most half a step of hi (2^-8 / 2^-11 of it)
    eps = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    assert bool((yp[1].double().abs() <= yp[0].double().abs() * eps + 2.0 ** -24).all())


@pytest.mark.parametrize("store,skind", [p for p in S_KINDS if p.values[1] != "none"])
@pytest.mark.parametrize("nhw,c", [pytest.param(SIZES[3], c, id=f"{SIZE_IDS[3]}-{c}") for c in WIDTHS])
def test_pa_gate_saturated_gates(store, nhw, c, skind):
    """every bias at -60: the gate is below 1e-24 and y equals s, bit for bit; at +60 the gate is 1.0 in fp32 and y = rnd(t + s)"""
    dt = DT[store]
    for bias in (-60.0, 60.0):
        cs = _case(store, nhw, c, bias=bias)
        s, s64 = _s_of(cs, skind)
        _, arg = _ref(cs, s64)
        assert float(arg.abs().min()) > 50.0 and float(arg.abs().max()) < 70.0
        y = _gate(cs, store, s)[..., :c]
        want = s64.float().to(dt) if bias < 0 else (cs["t"].float() + s64.float()).to(dt)
        nd = int((y != want).sum())
        print(f"pa_gate {store} C={c} s={skind} bias {bias:+.0f}: arguments {float(arg.min()):.1f} .. {float(arg.max()):.1f}, {nd} values differ")
        assert nd == 0


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("joint", [True, False], ids=["one-arena", "split-arenas"])
def test_pa_gate_stays_inside_its_views(store, joint):
    """t at channel offset 8 of a pitch-72 tensor and s at offset 16 of a pitch-80 tensor, NaN in the foreign channels and in the guards,
    the result at offset 16 of a pitch-80 tensor: nothing else is written, and the result is what the dense tensors give, bit for bit"""
    from ntire2022_esr_amd import ops
    nhw, c = (2, 20, 36), 48
    cs = _case(store, nhw, c)
    dt = DT[store]
    clean = _gate(cs, store, cs["s"])
    wide_t = torch.full(nhw + (72,), float("nan"), dtype=dt)
    wide_t[..., 8:8 + c] = cs["t"]
    wide_s = torch.full(nhw + (80,), float("nan"), dtype=dt)
    wide_s[..., 16:16 + c] = cs["s"]
    arenas = [G.Arena(DEV, fill="nan", seed=4)] if joint else [G.Arena(DEV, fill="nan", seed=4), G.Arena(DEV, fill="nan", seed=5)]
    a_in, a_out = arenas[0], arenas[-1]
    a_in.add_input("t", wide_t)
    a_in.add_input("s", wide_s)
    a_out.add_output("y", nhw + (80,), dt, writable=(-1, 16, c))
    for a in arenas:
        a.build()
    ops.pa_gate(a_in["t"], cs["w"], cs["b"], s=a_in["s"], in_coff=8, s_coff=16, out=a_out["y"], out_coff=16)
    for a in arenas:
        a.check_untouched()
    assert torch.equal(a_out.written("y").cpu(), clean)


@pytest.mark.parametrize("store", STORES)
def test_pa_gate_refuses_a_result_in_t_or_s(store):
    """y is another tensor than t and s (the op is not specified in place): ESR_ERR_BAD_ARG before anything is launched; so are a
    caller-provided output of another dtype, pitch or shape"""
    from ntire2022_esr_amd import ops, _lib as L
    cs = _case(store, (1, 16, 16), 48)
    t, s = cs["t"].to(DEV), cs["s"].to(DEV)
    before = (t.clone(), s.clone())
    for out in (t, s):
        with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
            ops.pa_gate(t, cs["w"], cs["b"], s=s, out=out)
    wide = torch.zeros(1, 16, 16, 128, dtype=DT[store], device=DEV)
    wide[..., :48] = t
    with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
        ops.pa_gate(wide, cs["w"], cs["b"], out=wide, out_coff=64)
    for bad in (torch.zeros(1, 16, 16, 48, dtype=torch.float64, device=DEV), torch.zeros(1, 16, 16, 44, dtype=DT[store], device=DEV),
                torch.zeros(1, 16, 17, 48, dtype=DT[store], device=DEV), torch.zeros(1, 16, 16, 48, dtype=DT[store])):
        with pytest.raises(L.EsrError):
            ops.pa_gate(t, cs["w"], cs["b"], s=s, out=bad)
    if store != "f32":
        pair = torch.stack([s, torch.zeros_like(s)])
        with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
            ops.pa_gate(t, cs["w"], cs["b"], s=pair, out=pair, pair_out=True)
    torch.cuda.synchronize()
    assert torch.equal(t, before[0]) and torch.equal(s, before[1]) and not bool(wide[..., 48:].any())


PAD_WIDTHS = [33, 34, 35, 36, 37, 38, 39]              # every remainder of C mod 8 but 0: each rung of the kernels' pad-slot masks


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("c", PAD_WIDTHS)
def test_pad_slots_never_reach_a_result(store, c):
    """`channels of t and s at and beyond C are never used, whatever they hold`: the pad slots C .. 39 of t, s (single and pair) and of the
    fused kernel's x hold NaN -- the results are those of the zero-padded tensors bit for bit, their own pad channels zeros.  pa_gate_kernel
    masks after the load; pa_tail_kernel clears the last 16-byte piece of the staged x (`keep` = C mod 8 = 1 .. 7 here) and masks s."""
    from ntire2022_esr_amd import ops
    nhw = (1, 17, 33)
    nan = float("nan")
    cs = _case(store, nhw, c)
    pitch = _up(c, 8)
    kinds = ["none", "single"] + ([] if store == "f32" else ["pair"])
    for skind in kinds:
        s, _ = _s_of(cs, skind)
        clean = _gate(cs, store, s)
        sd = None if s is None else _padded(s, pitch, nan).to(DEV)
        y = ops.pa_gate(_padded(cs["t"], pitch, nan).to(DEV), cs["w"], cs["b"], s=sd)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(clean).all()) and torch.equal(y.cpu(), clean), (skind, int((y.cpu() != clean).sum()))
        assert torch.all(y.cpu()[..., c:] == 0)
    if store == "f32":
        return
    ct = _tail_case(store, nhw, c)
    for skind in kinds:
        s, _ = _s_of(ct, skind)
        clean = _tail(ct, s)
        sd = None if s is None else _padded(s, pitch, nan).to(DEV)
        y = ops.pa_tail(_padded(ct["x"], pitch, nan).to(DEV), ct["w3"], ct["b3"], ct["w"], ct["b"], s=sd)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(clean).all()) and torch.equal(y.cpu(), clean), (skind, int((y.cpu() != clean).sum()))
        assert torch.all(y.cpu()[..., c:] == 0)


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("c,cout", [(33, 48), (38, 48), (50, 64), (48, 48)])
def test_more_channels_stored_than_the_granule_needs(store, c, cout):
    """cout up to round_up(C, 16) (`out_channels`): a destination that is a whole K chunk wider than C, as the engine stores into whole
    buffers -- channels 0 .. C - 1 are those of the default width, C .. cout - 1 zeros over a destination that held something else"""
    from ntire2022_esr_amd import ops
    nhw = (1, 17, 33)
    cs = _case(store, nhw, c)
    base = _gate(cs, store, cs["s"])
    dirty = torch.full(nhw + (cout,), 7.0, dtype=DT[store], device=DEV)
    wide = _gate(cs, store, cs["s"], out=dirty, out_channels=cout)
    assert wide.shape[-1] == cout and torch.equal(wide[..., :c], base[..., :c]) and torch.all(wide[..., c:] == 0)
    if store == "f32":
        return
    ct = _tail_case(store, nhw, c)
    base = _tail(ct, ct["s"], pair_out=True)
    dirty = torch.full((2,) + nhw + (cout,), 7.0, dtype=DT[store], device=DEV)
    wide = _tail(ct, ct["s"], pair_out=True, out=dirty, out_channels=cout)
    assert wide.shape[-1] == cout and torch.equal(wide[..., :c], base[..., :c]) and torch.all(wide[..., c:] == 0)


# ---- esr_pa_tail ----------------------------------------------------------------------------------------------------------------------------
STORES16 = ["bf16", "f16"]
TAIL_CASES = GATE_CASES


def _conv3_eff(w3, b3, store):
    """the 3x3 as pa_tail_kernel (and conv_s16_kernel) multiplies by it: read back from the esr_pack_conv_s16 blob"""
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    c = w3.shape[0]
    phys = _up(c, 16)
    we, be = unpack_conv_s16(pack_conv_s16(w3, b3, store, cin_phys=phys), c, c, 3, store, cin_phys=phys)
    return we.double(), be.double()


def _tail_case(store, nhw, c, b3=None):
    key = ("tail", store, nhw, c, b3)
    if key not in _cases:
        cs = dict(_case(store, nhw, c))
        n, h, w = nhw
        g = torch.Generator().manual_seed(77 * c + 10 * h + w + STORES16.index(store))
        cs["x"] = torch.randn(n, h, w, c, generator=g).to(DT[store])
        cs["w3"], cs["b3"] = torch.randn(c, c, 3, 3, generator=g) * 0.08, torch.randn(c, generator=g) * 0.5
        if b3 is not None:
            cs["b3"] = torch.full((c,), float(b3))
        cs["w3e"], cs["b3e"] = _conv3_eff(cs["w3"], cs["b3"], store)
        _cases[key] = cs
    return _cases[key]


def _tail(cs, s=None, w=None, b=None, **kw):
    from ntire2022_esr_amd import ops
    c = cs["x"].shape[-1]
    pitch = _up(c, 8)
    sd = None if s is None else _padded(s, pitch).to(DEV)
    y = ops.pa_tail(_padded(cs["x"], pitch).to(DEV), cs["w3"], cs["b3"], cs["w"] if w is None else w, cs["b"] if b is None else b, s=sd, **kw)
    torch.cuda.synchronize()
    return y.cpu()


def _hidden_t(cs):
    """t, which no launch stores, handed out EXACTLY: a zero gate weight and a bias of +60 make the gate 1.0 in fp32, and a pair output
    without s is t to 16 extra bits (hi = rnd(t): the gate's matrix operand).  Returns (hi, lo) in the storage type, [n, h, w, C]"""
    c = cs["x"].shape[-1]
    yp = _tail(cs, w=torch.zeros(c, c), b=torch.full((c,), 60.0), pair_out=True)
    assert torch.all(yp[..., c:] == 0)
    return yp[0][..., :c], yp[1][..., :c]


def _conv_ref(cs, ring=None):
    """fp64 t = conv3x3(x) + b3 on the effective weights, NHWC; ring: a value that stands in the out-of-image ring instead of zeros (the WRONG
    padding of the border test)"""
    x = cs["x"].double().permute(0, 3, 1, 2)
    if ring is None:
        t = torch.nn.functional.conv2d(x, cs["w3e"], cs["b3e"], padding=1)
    else:
        t = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (1, 1, 1, 1), value=float(ring)), cs["w3e"], cs["b3e"])
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("store,skind", [pytest.param(st, k, id=f"{st}-{k}") for st in STORES16 for k in ("none", "single", "pair")])
@pytest.mark.parametrize("nhw,c", TAIL_CASES)
def test_pa_tail_stage_by_stage(store, nhw, c, skind):
    """The hidden t against the fp64 restatement of the 3x3 on the effective weights (an fp32 accumulation: 2e-5 of the largest value, plus
    2^-16 of the value for the pair that hands it out); W = 0 and b = 0: exactly t / 2, both parts of the pair; then the gated result
    against the fp64 restatement computed FROM THAT t, its matrix operand rnd(t) = the pair's high part: one store (_tol)."""
    from ntire2022_esr_amd import ops
    cs = _tail_case(store, nhw, c)
    dt = DT[store]
    hi, lo = _hidden_t(cs)
    t = hi.double() + lo.double()
    ref_t = _conv_ref(cs)
    err = (t - ref_t).abs()
    bound = _tol(ref_t, torch.float32) + ref_t.abs() * 2.0 ** -16
    print(f"pa_tail {store} C={c} {nhw}: hidden t max|got - ref| = {float(err.max()):.3e} ({float((err / bound).max()):.3f} of the bound), max|t| = {float(t.abs().max()):.2f}")
    assert int((err > bound).sum()) == 0 and (float(t.abs().max()) > 1.0 or nhw == (1, 1, 1))
    half = _tail(cs, w=torch.zeros(c, c), b=torch.zeros(c), pair_out=True)[..., :c]
    # (halving is exact unless the halved part falls below the storage type's smallest normal, where it needs a rounding of its own: a part
    # at or below twice that is held to one subnormal step instead)
    tiny = 2.0 ** (-126 if dt == torch.bfloat16 else -14)
    for got, full in ((half[0], hi), (half[1], lo)):
        normal = full.double().abs() > 2 * tiny
        assert torch.equal((got.double() * 2)[normal], full.double()[normal])
        assert float((got.double() * 2 - full.double()).abs().max()) <= 2 * tiny * 2.0 ** (-7 if dt == torch.bfloat16 else -10)
    s, s64 = _s_of(cs, skind)
    arg = hi.double() @ cs["we"].t() + cs["be"]
    ref = t * _sigmoid(arg) + (0.0 if s64 is None else s64)
    with ops.kernel_trace() as names:
        y = _tail(cs, s)
    assert names == [f"pa_tail_kernel<{'true' if store == 'bf16' else 'false'}, {(c + 15) // 16}>"], names
    assert y.shape == nhw + (_up(c, 8),) and torch.all(y[..., c:] == 0)
    err = (y[..., :c].double() - ref).abs()
    print(f"pa_tail {store} C={c} {nhw} s={skind}: max|got - ref| = {float(err.max()):.3e} ({float((err / _tol(ref, dt)).max()):.3f} of the bound)")
    assert int((err > _tol(ref, dt)).sum()) == 0
    yp = _tail(cs, s, pair_out=True)
    assert torch.equal(yp[0], y) and torch.all(yp[..., c:] == 0)
    err = ((yp[0].double() + yp[1].double())[..., :c] - ref).abs()
    bound = _tol(ref, torch.float32) + ref.abs() * 2.0 ** -16
    assert int((err > bound).sum()) == 0, float((err / bound).max())


def _grid(g, shape, step, bound):
    """seeded multiples of `step` in [-bound, bound]"""
    k = int(round(bound / step))
    return torch.randint(-k, k + 1, shape, generator=g).double() * step


@pytest.mark.parametrize("store", STORES16)
@pytest.mark.parametrize("nhw,c", TAIL_CASES)
def test_pa_tail_exact_case_bit_for_bit(store, nhw, c):
    """The whole chain from x alone on a coarse binary grid: x and s in steps of 1/16, the 3x3's weights of 1/16 (values of the storage type,
    which the packer's error diffusion leaves as they are: asserted on the blob), its bias of 1/4.  Every term of t is a multiple of 2^-8
    and the magnitudes sum to less than 2^16: every partial sum in ANY order is an fp32 number, so t is exact; with a zero gate weight
    and a bias of 0 / +60 / -60 the gate is exactly 1/2 / 1 / below 1e-26, and a correct kernel returns rnd(t / 2 + s), rnd(t + s) and s
    bit for bit."""
    n, h, w = nhw
    dt = DT[store]
    g = torch.Generator().manual_seed(77 + 100 * h + w + c)
    x = _grid(g, (n, h, w, c), 1 / 16, 2.0)
    s = _grid(g, (n, h, w, c), 1 / 16, 4.0)
    s = torch.where(s == 0, torch.full_like(s, 1 / 16), s)                      # (at -60 the result is s itself: keep it away from the tiny product)
    w3, b3 = _grid(g, (c, c, 3, 3), 1 / 16, 0.125), _grid(g, (c,), 1 / 4, 0.5)
    assert torch.equal(x, x.to(dt).double()) and torch.equal(s, s.to(dt).double())
    w3e, b3e = _conv3_eff(w3.float(), b3.float(), store)
    assert torch.equal(w3e, w3) and torch.equal(b3e, b3)
    xn = x.permute(0, 3, 1, 2)
    mags = torch.nn.functional.conv2d(xn.abs(), w3.abs(), b3.abs(), padding=1)
    assert float(mags.max()) < 2.0 ** 24 * 2.0 ** -8
    t = torch.nn.functional.conv2d(xn, w3, b3, padding=1).permute(0, 2, 3, 1)
    assert torch.equal(t, t.float().double()) and (float(t.abs().max()) > 4.0 or nhw == (1, 1, 1))
    cs = dict(x=x.to(dt), w3=w3.float(), b3=b3.float())
    zero = torch.zeros(c, c)
    for bias, want in ((0.0, (t.float() * 0.5 + s.float()).to(dt)), (60.0, (t.float() + s.float()).to(dt)), (-60.0, s.to(dt))):
        y = _tail(cs, s.to(dt), w=zero, b=torch.full((c,), bias))
        nd = int((y[..., :c] != want).sum())
        print(f"pa_tail exact {store} C={c} {nhw} gate bias {bias:+.0f}: {nd} of {want.numel()} values differ; max|t| = {float(t.abs().max()):.2f}")
        assert nd == 0 and torch.all(y[..., c:] == 0)


@pytest.mark.parametrize("store", STORES16)
@pytest.mark.parametrize("c", WIDTHS)
def test_pa_tail_zero_pads_x(store, c):
    """t at a border pixel is the zero-padded convolution.  With every bias of the 3x3 at 3: the restatement whose ring of x holds 3 instead
    of zeros is off at the one-pixel border by far more than the bound and nowhere else -- shown on the CPU -- and the kernel's hidden t
    is held to the zero-padded one everywhere"""
    nhw = (1, 17, 33)
    cs = _tail_case(store, nhw, c, b3=3.0)
    hi, lo = _hidden_t(cs)
    t = hi.double() + lo.double()
    right, wrong = _conv_ref(cs), _conv_ref(cs, ring=3.0)
    bound = _tol(right, torch.float32) + right.abs() * 2.0 ** -16
    border = torch.ones(nhw + (c,), dtype=torch.bool)
    border[:, 1:-1, 1:-1] = False
    ratio = ((wrong - right).abs() / bound)[border]
    print(f"pa_tail border {store} C={c}: the 3-padded restatement is off by a median of {float(ratio.median()):.0f} x (max {float(ratio.max()):.0f} x) the bound at the border")
    assert float(ratio.median()) > 100.0 and float((wrong - right).abs()[~border].max()) < 1e-9
    err = (t - right).abs()
    assert int((err > bound).sum()) == 0, float((err / bound).max())


def _ordinal(t):
    """a 16-bit float tensor as integers in value order (+0 = -0 = 0): neighbours in the storage type differ by 1"""
    bits = t.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF
    return torch.where(bits >= 0x8000, -(bits & 0x7FFF), bits & 0x7FFF)


def _ulp(v, dt):
    """the storage step of dt at the magnitude of the fp64 tensor v (the subnormal step below the smallest normal)"""
    mbits, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    return torch.exp2(torch.floor(torch.log2(torch.clamp(v.abs(), min=2.0 ** emin))) - mbits)


@pytest.mark.parametrize("store", STORES16)
@pytest.mark.parametrize("skind", ["none", "single", "pair"])
@pytest.mark.parametrize("nhw,c", [pytest.param(SIZES[4], c, id=f"{SIZE_IDS[4]}-{c}") for c in WIDTHS])
def test_fused_against_per_op_form(store, nhw, c, skind):
    """The per-op form stores t once in the storage type, t16 = rnd(t), and multiplies THAT by the gate g; the fused form multiplies the fp32
    t.  Both feed the same rnd(t) to the gate's 1x1 -- asserted: the 3x3 launch's result equals the high part of the fused kernel's hidden t
    bit for bit (both accumulate from the bias, chunk by chunk, tap pair by tap pair) -- so g is the same and the two fp32 sums differ by
    |t - t16| g <= half a storage step of t times g.
      without s   |t g| 2^-(m+1) < step(t g), so the sums are less than one step of y apart and the stored results are equal or
                  NEIGHBOURS in the storage type: asserted, at most ONE 16-bit step.
      with s      one step of y cannot hold: where t g and s cancel, y is far smaller than t and its own steps far finer than what t's
                  rounding leaves (hundreds of them on this data).  Asserted is the bound that does hold, term by term:
                  |fused - per-op| <= |t - t16| g + step(fused) / 2 + step(per-op) / 2, plus 4 x 2^-24 (|t g| + |s|) for the fp32
                  operations of the two kernels; |t - t16| <= |lo| + step(lo) / 2 of the hidden t's pair.
    The share of outputs that differ at all and the largest distance in 16-bit steps are printed."""
    from ntire2022_esr_amd import ops
    cs = _tail_case(store, nhw, c)
    dt = DT[store]
    s, s64 = _s_of(cs, skind)
    pitch = _up(c, 8)
    xd = _padded(cs["x"], pitch).to(DEV)
    sd = None if s is None else _padded(s, pitch).to(DEV)
    with ops.kernel_trace() as names:
        t16 = ops.conv2d(xd, cs["w3"], cs["b3"], cin=c)
        per_op = ops.pa_gate(t16, cs["w"], cs["b"], s=sd)
        fused = ops.pa_tail(xd, cs["w3"], cs["b3"], cs["w"], cs["b"], s=sd)
    torch.cuda.synchronize()
    assert [k.split("<")[0] for k in names][1:] == ["pa_gate_kernel", "pa_tail_kernel"], names
    hi, lo = _hidden_t(cs)
    t16 = t16.cpu()[..., :c]
    assert torch.equal(t16, hi)                                   # the same matrix operand for the gate in both forms
    a16, b16 = fused.cpu()[..., :c], per_op.cpu()[..., :c]
    a, b = a16.double(), b16.double()
    steps = (_ordinal(a16) - _ordinal(b16)).abs()
    share = 100.0 * float((a != b).double().mean())
    if skind == "none":
        print(f"fused against per-op {store} C={c} s=none: {share:.2f} % of {a.numel()} outputs differ, by at most {int(steps.max())} 16-bit step(s)")
        assert int(steps.max()) <= 1
        return
    t = hi.double() + lo.double()
    g = _sigmoid(hi.double() @ cs["we"].t() + cs["be"])
    # (|t - t16| itself: the hidden t is handed out as hi + lo, so it is known to half a step of lo)
    dt16 = lo.double().abs() + 0.5 * _ulp(lo.double(), dt)
    bound = dt16 * g * (1 + 1e-5) + 0.5 * _ulp(a, dt) + 0.5 * _ulp(b, dt) + 4 * 2.0 ** -24 * ((t * g).abs() + s64.abs())
    ratio = (a - b).abs() / bound
    print(f"fused against per-op {store} C={c} s={skind}: {share:.2f} % of {a.numel()} outputs differ, by at most {int(steps.max())} 16-bit steps of "
          f"their own; |fused - per-op| reaches {float(ratio.max()):.3f} of the derived bound")
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("store", STORES16)
def test_pa_tail_views_and_aliasing(store):
    """x at channel offset 8 of a pitch-72 tensor, s at offset 16 of a pitch-80 tensor, NaN in the foreign channels and the guards, the
    result at offset 16 of a pitch-80 tensor: nothing else is written and the result is the dense tensors', bit for bit; a result in x's
    or s's tensor is refused before anything is launched"""
    from ntire2022_esr_amd import ops, _lib as L
    nhw, c = (2, 20, 36), 48
    cs = _tail_case(store, nhw, c)
    dt = DT[store]
    clean = _tail(cs, cs["s"])
    wide_x = torch.full(nhw + (72,), float("nan"), dtype=dt)
    wide_x[..., 8:8 + c] = cs["x"]
    wide_s = torch.full(nhw + (80,), float("nan"), dtype=dt)
    wide_s[..., 16:16 + c] = cs["s"]
    a = G.Arena(DEV, fill="nan", seed=6)
    a.add_input("x", wide_x)
    a.add_input("s", wide_s)
    a.add_output("y", nhw + (80,), dt, writable=(-1, 16, c))
    a.build()
    ops.pa_tail(a["x"], cs["w3"], cs["b3"], cs["w"], cs["b"], s=a["s"], in_coff=8, s_coff=16, out=a["y"], out_coff=16)
    a.check_untouched()
    assert torch.equal(a.written("y").cpu(), clean)
    x, s = cs["x"].to(DEV), cs["s"].to(DEV)
    for out in (x, s):
        with pytest.raises(L.EsrError, match="ESR_ERR_BAD_ARG"):
            ops.pa_tail(x, cs["w3"], cs["b3"], cs["w"], cs["b"], s=s, out=out)
    with pytest.raises(L.EsrError, match="16-bit storage only"):
        ops.pa_tail(x.float(), cs["w3"], cs["b3"], cs["w"], cs["b"])
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), cs["x"]) and torch.equal(s.cpu(), cs["s"])


# ---- the network ----------------------------------------------------------------------------------------------------------------------------
_models = {}


FORMS = [("f32", False), ("bf16", False), ("bf16", True), ("f16", False), ("f16", True)]      # (an fp32 plan has the per-op form only)


def _repafdn(compute, fuse=False, true_weights=False):
    from safetensors.torch import load_file
    from ntire2022_esr_amd import RePAFDN
    key = "true" if true_weights else "m"
    if key not in _models:
        m = RePAFDN()
        if true_weights:
            sd = {}
            for part in ("_f32.safetensors", "_f32.part2.safetensors"):
                sd.update(load_file(os.path.join(GOLD, STEM + part)))
        else:
            sd = load_file(os.path.join(GOLD, STEM + ".safetensors"))
        m.load_state_dict(sd, strict=True)
        _models[key] = m.eval().to(DEV)
    m = _models[key]
    m.set_compute(compute)
    m.fuse_pa_tail = fuse
    m.use_graphs = True
    return m


def _key(shape):
    return tuple(shape) + (torch.device(DEV),)


def _tail_kinds(m, shape):
    """the kinds of the plan's ops that hold the gate: ["pagate"] per-op, ["patail"] fused"""
    return [o.kind for o in m._plans[_key(shape)].plan.ops if o.kind in ("pagate", "patail")]


def _want_kinds(fuse):
    return ["patail"] if fuse else ["pagate"]


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_fp32_matches_reference_e2e(case):
    """image crops in 0 .. 1 (1 x 48 x 64, 2 x 20 x 36, 1 x 15 x 15: the minimum, a 1 x 1 pooled map): within 2e-5 max(1, |y|max)"""
    g = np.load(os.path.join(GOLD, f"e2e_{STEM}.npz"))
    m = _repafdn("f32")
    x, ref = torch.from_numpy(g["x" + case]).to(DEV), g["y" + case]
    with torch.no_grad():
        y = m(x).cpu().numpy()
    assert y.shape == ref.shape
    err = float(np.abs(y.astype(np.float64) - ref).max())
    print(f"RePAFDN e2e {case}: max|y - ref| = {err:.3e}, max|ref| = {float(np.abs(ref).max()):.3f}")
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max())), err


def _hr(h4, w4):
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB"))
    return np.pad(img, ((0, h4 - img.shape[0]), (0, w4 - img.shape[1]), (0, 0)), mode="symmetric")


@pytest.mark.parametrize("compute,fuse", FORMS)
@pytest.mark.parametrize("h,w", [(256, 256), (339, 510)])
def test_psnr_against_reference_at_stated_size(h, w, compute, fuse):
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"big_{STEM}_{h}x{w}.npz"))
    m = _repafdn(compute, fuse)
    dr = float(g["data_range"])
    with torch.no_grad():
        y = m(util.uint2tensor4(g["lr"], dr).to(DEV))
    assert _tail_kinds(m, (1, 3, h, w)) == _want_kinds(fuse)
    assert bool(torch.isfinite(y).all())
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(4 * h, 4 * w), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"RePAFDN {h}x{w} {compute} fuse_pa_tail={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB (d = {psnr - float(g['psnr']):+.4f}), "
          f"max|dy|/range = {rel:.2e}")
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    if compute == "f32":
        assert rel <= 2e-5 * max(1.0, float(np.abs(g["sr_sample"]).max())), rel


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_unrounded_checkpoint_against_its_goldens(compute, fuse):
    """the checkpoint as the reference ships it, fp32 and unrounded (true_team10_repafdn.npz): fp32 e2e within 2e-5 max(1, |y|max); the PSNR
    at 256 x 256 within the same budgets; max |dy| / range in 16-bit storage within MAX_REL (the constants above)"""
    from ntire2022_esr_amd import image_util as util
    g = np.load(os.path.join(GOLD, f"true_{STEM}.npz"))
    e2e = np.load(os.path.join(GOLD, f"e2e_{STEM}.npz"))
    lr = np.load(os.path.join(GOLD, f"big_{STEM}_256x256.npz"))["lr"]
    assert abs(float(g["dw_rel_bf16"]) - DW_REL["bf16"]) < 1e-4 and abs(float(g["dw_rel_f16"]) - DW_REL["f16"]) < 1e-5
    m = _repafdn(compute, fuse, true_weights=True)
    dr = float(g["data_range"])
    with torch.no_grad():
        if compute == "f32":
            for k in ("b", "c"):
                y = m(torch.from_numpy(e2e["x" + k]).to(DEV)).cpu().numpy()
                err = float(np.abs(y.astype(np.float64) - g["y" + k]).max())
                print(f"RePAFDN true weights e2e {k}: max|y - ref| = {err:.3e}")
                assert err <= 2e-5 * max(1.0, float(np.abs(g["y" + k]).max())), err
        y = m(util.uint2tensor4(lr, dr).to(DEV))
    psnr = util.calculate_psnr(util.tensor2uint(y, dr), _hr(1024, 1024), border=4)
    rel = float(np.abs(y[0, :, ::9, ::9].cpu().numpy().astype(np.float64) - g["sr_sample"]).max()) / dr
    print(f"RePAFDN true weights 256x256 {compute} fuse_pa_tail={int(fuse)}: PSNR {psnr:.4f} vs reference {float(g['psnr']):.4f} dB (d = {psnr - float(g['psnr']):+.4f}), "
          f"max|dy|/range = {rel:.2e}" + ("" if compute == "f32" else f" (bound {MAX_REL[compute]:.2e})"))
    assert abs(psnr - float(g["psnr"])) <= BUDGET[compute]
    assert rel <= (2e-5 * max(1.0, float(np.abs(g["sr_sample"]).max())) if compute == "f32" else MAX_REL[compute]), rel


def _crops(n, h, w, seed):
    """n crops of test.bmp in 0 .. 1, NCHW (the network's data_range is 1.0; uniform noise is not what it was trained on)"""
    from PIL import Image
    img = np.array(Image.open(os.path.join(GOLD, "test.bmp")).convert("RGB")).astype(np.float32) / 255.0
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        y0, x0 = rng.randint(0, img.shape[0] - h + 1), rng.randint(0, img.shape[1] - w + 1)
        out.append(img[y0:y0 + h, x0:x0 + w])
    return torch.from_numpy(np.stack(out)).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_batch_equals_per_image(compute, fuse):
    m = _repafdn(compute, fuse)
    x = _crops(2, 40, 52, 40).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(2)]
    kinds = lambda shape: [(o.kind, getattr(o, "w", None)) for o in m._plans[_key(shape)].plan.ops]
    assert kinds(x.shape) == kinds((1, 3, 40, 52)) and _tail_kinds(m, x.shape) == _want_kinds(fuse)
    for i in range(2):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", FORMS)
def test_thin_images_in_a_batch(compute, fuse):
    """five 15 x 15 images (the minimum: a 1 x 1 pooled map; fewer pixels than a group of 16 holds per row) against each image alone"""
    m = _repafdn(compute, fuse)
    x = _crops(5, 15, 15, 15).to(DEV)
    with torch.no_grad():
        yb = m(x)
        ys = [m(x[i:i + 1]) for i in range(5)]
    assert bool(torch.isfinite(yb).all())
    for i in range(5):
        assert torch.equal(yb[i:i + 1], ys[i]), (i, float((yb[i:i + 1] - ys[i]).abs().max()))


@pytest.mark.parametrize("compute,fuse", [("f32", False), ("bf16", False), ("bf16", True)])
def test_graph_forward_equals_run_ops(compute, fuse):
    from ntire2022_esr_amd import _lib as L
    m = _repafdn(compute, fuse)
    shape = (1, 3, 40, 52)
    xs = [_crops(1, 40, 52, 9 + i).to(DEV) for i in range(4)]
    with torch.no_grad():
        m.use_graphs = False
        ref = [m(x).clone() for x in xs]
        torch.cuda.synchronize()
        m.use_graphs = True
        ys = [m(x) for x in xs]               # forwards 2 .. 4 are graph launches with new x / y each
    torch.cuda.synchronize()
    ent = m._plans[_key(shape)]
    assert _tail_kinds(m, shape) == _want_kinds(fuse)
    assert ent.graph is not None and L.lib().esr_graph_nodes(ent.graph) >= len(ent.arr)
    for y, r in zip(ys, ref):
        assert torch.equal(y, r), float((y - r).abs().max())


@pytest.mark.parametrize("shape", [(1, 3, 15, 15), (2, 3, 20, 36)], ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("compute,fuse", FORMS)
def test_result_does_not_depend_on_stale_workspace_bytes(compute, fuse, shape):
    """tests/test_gpu_stale_workspace.py's first check for this network: the whole workspace overwritten with hostile finite patterns
    (tests/_poison.py) between two forwards of one shape, through esr_run_ops and through graph replay, bit for bit"""
    m = _repafdn(compute, fuse)
    assert not m.rezero_on_switch
    dev = torch.device(DEV)
    x = _crops(shape[0], shape[2], shape[3], 17 * shape[2] + shape[3]).to(DEV)
    try:
        results = []
        for graphs in (False, True):
            m.use_graphs = graphs
            m._drop_plans()                                     # a fresh context: prepare() zero-fills the workspace
            ent = m.prepare(shape, DEV)
            ctx = m._ctxs[(dev, torch.cuda.default_stream(dev).cuda_stream)]
            assert ctx.ws_owner == _key(shape) and not bool(ctx.ws.any())
            assert _tail_kinds(m, shape) == _want_kinds(fuse)
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
