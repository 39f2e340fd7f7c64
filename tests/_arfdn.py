"""What tests/test_arfdn.py (CPU) and tests/test_gpu_arfdn.py share: the fp64 restatement of an ARFDB step (team 14, block.py:233-254) as
esr_asym_step defines it, the widths and sizes the kernel is tested at, the cases' inputs and the stand-in descriptor of the refusal tests."""
import ctypes
from types import SimpleNamespace

import torch
import torch.nn.functional as F

DT = {"bf16": torch.bfloat16, "f16": torch.float16}
MANT = {torch.bfloat16: 7, torch.float16: 10}                  # stored mantissa bits
MIN_NORMAL = {torch.bfloat16: 2.0 ** -126, torch.float16: 2.0 ** -14}

# (1, 1), (1, 19), (19, 1): one-pixel images and one-pixel-wide strips across a tile edge; (15, 15): a lone partial tile; (16, 17), (33, 18): one
# column / row spills into a second tile, and a halo pixel is a real pixel of another tile
SIZES = [(1, 1), (1, 19), (19, 1), (15, 15), (16, 17), (33, 18)]
# (cin, c, `+ in`, number of earlier distilled maps).  ARFDN's own three steps, then both ends of every range esr_asym_step_supported admits
# (c 17..32; cin 17..32 with or without `+ in`, 33..64 without) and every residue of the kernel's pad-slot mask, keep = cin - (round_up(cin, 8) - 8)
# in 1 .. 7, with one, three (cin 33..48) and four chunks of the 1x1's image
ARFDN_WIDTHS = [(50, 25, False, 0), (25, 25, True, 1), (25, 25, True, 2)]
NEW_WIDTHS = [(17, 17, True, 2),        # keep = 1, the lower end of every range
              (27, 27, True, 0),        # keep = 3
              (32, 32, True, 1),        # the upper end of the residual form
              (18, 24, False, 1),       # keep = 2
              (22, 32, False, 2),       # keep = 6
              (31, 17, False, 0),       # keep = 7
              (33, 17, False, 1),       # the lower end of the two-K-pair form: three 1x1 chunks, keep = 1
              (45, 32, False, 2),       # keep = 5
              (52, 20, False, 0),       # four chunks, keep = 4
              (64, 25, False, 1)]       # the upper end of cin
# ARFDN's widths at every size, the others at the two sizes with a ragged second tile in one direction each
STEP_CASES = [(hw,) + wd for wd in ARFDN_WIDTHS for hw in SIZES] + [(hw,) + wd for wd in NEW_WIDTHS for hw in [(16, 17), (33, 18)]]


def case_id(v):
    hw, cin, c, res, np_ = v
    return f"{hw[0]}x{hw[1]}-{cin}-{c}-{'res' if res else 'nores'}-p{np_}"


def r8(c):
    return (c + 7) // 8 * 8


def act(v, slope):
    """the kernels' max(v, slope v), slope <= 1"""
    return torch.maximum(v, v * slope)


def stored(v, dt):
    """v as a tensor of dtype dt holds it (RNE from fp32, as the kernels round), back in fp64"""
    return v.to(torch.float32).to(dt).double()


def ulp(v, dt):
    """the storage step at |v| (the smallest normal number's below it)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(MIN_NORMAL[dt])))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dt])


def step_ref(x, w, slope, res, ps, dt, d_used=None, bias_pad=False):
    """The step in fp64.  x [n, cin, h, w] and ps (the earlier distilled maps [n, c, h, w]) as stored; w: namespace of fp64 weights d, bd
    [c, cin, 1, 1], l1, bl1 [c, cin, 3, 1], m1, bm1 [c, cin, 1, 3], l2 [c, c, 1, 3], m2 [c, c, 3, 1], b2 = b_l2 + b_m2.  d, a_l and a_m are rounded
    to dt once; d_used: the d added in the sum (default: the restated one).  bias_pad: the WRONG reading of the padding -- a_l / a_m computed
    on the zero-padded input, so that the halo of the second convolutions holds act(bias) instead of 0.
    -> namespace(d, a_l, a_m, out: before the last rounding; extra: |W_l2| (*) ulp(a_l) + |W_m2| (*) ulp(a_m), what one storage step of
    every never-stored operand moves `out` by at most)"""
    x = x.double()
    d = act(F.conv2d(x, w.d, w.bd), slope)
    if bias_pad:
        xp = F.pad(x, (1, 1, 1, 1))
        a_l = stored(act(F.conv2d(xp, w.l1, w.bl1, padding=(1, 0)), slope)[:, :, 1:-1, :], dt)       # h rows x (w + 2) columns
        a_m = stored(act(F.conv2d(xp, w.m1, w.bm1, padding=(0, 1)), slope)[:, :, :, 1:-1], dt)       # (h + 2) rows x w columns
        pl, pm = (0, 0), (0, 0)
    else:
        a_l = stored(act(F.conv2d(x, w.l1, w.bl1, padding=(1, 0)), slope), dt)
        a_m = stored(act(F.conv2d(x, w.m1, w.bm1, padding=(0, 1)), slope), dt)
        pl, pm = (0, 1), (1, 0)
    v = F.conv2d(a_l, w.l2, padding=pl) + F.conv2d(a_m, w.m2, padding=pm) + w.b2[None, :, None, None]
    if res:
        v = v + x
    v = v + (stored(d, dt) if d_used is None else d_used.double())
    for p in ps:
        v = v + p.double()
    extra = F.conv2d(ulp(a_l, dt), w.l2.abs(), padding=pl) + F.conv2d(ulp(a_m, dt), w.m2.abs(), padding=pm)
    return SimpleNamespace(d=d, a_l=a_l, a_m=a_m, out=act(v, slope), extra=extra)


def _seed(store, hw, cin, c, res, np_, tag):
    return (1000003 * cin + 10007 * c + 101 * hw[0] + 7 * hw[1] + 3 * np_ + int(res) + (store == "f16") * 50021 + tag * 99991) % (2 ** 31)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def random_case(store, hw, cin, c, res, np_, n=2, b1=None, slope=0.05):
    """inputs rounded to the storage type, fp32 weights as a checkpoint holds them; b1: the value of every b_l1 / b_m1 (the border case)"""
    dt = DT[store]
    g = torch.Generator().manual_seed(_seed(store, hw, cin, c, res, np_, 1 if b1 is None else 2))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rn(n, hw[0], hw[1], cin).to(dt)
    ps = [(rn(n, hw[0], hw[1], c) * 0.5).to(dt) for _ in range(np_)]
    W = dict(w_d=rn(c, cin, 1, 1) * 0.15, b_d=rn(c) * 0.2,
             w_l1=rn(c, cin, 3, 1) * 0.1, b_l1=rn(c) * 0.1, w_l2=rn(c, c, 1, 3) * 0.1, b_l2=rn(c) * 0.1,
             w_m1=rn(c, cin, 1, 3) * 0.1, b_m1=rn(c) * 0.1, w_m2=rn(c, c, 3, 1) * 0.1, b_m2=rn(c) * 0.1)
    if b1 is not None:
        W["b_l1"], W["b_m1"] = torch.full((c,), float(b1)), torch.full((c,), float(b1))
    return SimpleNamespace(store=store, dt=dt, hw=hw, cin=cin, c=c, res=res, x=x, ps=ps, W=W, slope=slope)


def grid_case(store, hw, cin, c, res, np_, n=2):
    """The exact grid: inputs in {-1, 0, 1}, sparse weights in {-1, 0, 1}, integer biases, earlier maps on multiples of 1/4 and slope 1/2, so
    that every d, a_l and a_m is a multiple of 1/2 of a few bits and every partial sum a small multiple of 1/4 (asserted: grid_is_exact)"""
    dt = DT[store]
    g = torch.Generator().manual_seed(_seed(store, hw, cin, c, res, np_, 3))
    tri = lambda shape, density: ((torch.rand(*shape, generator=g) < density).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1))
    x = tri((n, hw[0], hw[1], cin), 0.5).to(dt)
    ps = [(torch.randint(-8, 9, (n, hw[0], hw[1], c), generator=g).float() / 4).to(dt) for _ in range(np_)]
    ib = lambda: torch.randint(-2, 3, (c,), generator=g).float()
    d1, d2 = min(0.25, 8.0 / cin), 6.0 / (3 * c)
    W = dict(w_d=tri((c, cin, 1, 1), d1), b_d=ib(),
             w_l1=tri((c, cin, 3, 1), d1 / 2), b_l1=ib(), w_l2=tri((c, c, 1, 3), d2), b_l2=ib(),
             w_m1=tri((c, cin, 1, 3), d1 / 2), b_m1=ib(), w_m2=tri((c, c, 3, 1), d2), b_m2=ib())
    return SimpleNamespace(store=store, dt=dt, hw=hw, cin=cin, c=c, res=res, x=x, ps=ps, W=W, slope=0.5)


def weights64(W, store=None):
    """the restatement's weights: the checkpoint's (store None) or the EFFECTIVE ones of the blobs esr_asym_step reads for `store`"""
    if store is None:
        l1, m1, l2, m2 = (W[k] for k in ("w_l1", "w_m1", "w_l2", "w_m2"))
        wd, bd, bl1, bm1, b2 = W["w_d"], W["b_d"], W["b_l1"], W["b_m1"], W["b_l2"] + W["b_m2"]
    else:
        from ntire2022_esr_amd.engine import pack_asym_s16, pack_conv_s16, unpack_asym_s16, unpack_conv_s16
        c, cin = W["w_d"].shape[:2]
        cp = (cin + 15) // 16 * 16
        wd, bd = unpack_conv_s16(pack_conv_s16(W["w_d"], W["b_d"], store, cin_phys=cp), cin, c, 1, store, cin_phys=cp)
        blob = pack_asym_s16(W["w_l1"], W["b_l1"], W["w_m1"], W["b_m1"], W["w_l2"], W["b_l2"], W["w_m2"], W["b_m2"], store)
        (l1, m1, l2, m2), (bl1, bm1, b2) = unpack_asym_s16(blob, cin, c, store)
    dd = lambda t: t.double()
    return SimpleNamespace(d=dd(wd), bd=dd(bd), l1=dd(l1), bl1=dd(bl1), m1=dd(m1), bm1=dd(bm1), l2=dd(l2), m2=dd(m2), b2=dd(b2))


def grid_is_exact(case, ref, w):
    """The derivation of the exact-grid test, checked: d, a_l and a_m of the fp64 restatement are representable in the storage type, and the
    sum of the MAGNITUDES of every term of every accumulation, in units of the grid (1/4), stays below 2^24 -- so every partial sum, in
    whatever order, is an integer multiple of 1/4 that fp32 holds exactly."""
    dt = case.dt
    x = nchw(case.x).double()
    for name in ("d", "a_l", "a_m"):
        v = getattr(ref, name)
        assert torch.equal(stored(v, dt), v), name
        assert torch.equal(v * 2, torch.round(v * 2)), name
    assert all(torch.equal(t.double() * 4, torch.round(t.double() * 4)) for t in [case.x] + case.ps)
    mags = [F.conv2d(x.abs(), w.d.abs()) + w.bd.abs()[None, :, None, None],
            F.conv2d(x.abs(), w.l1.abs(), padding=(1, 0)) + w.bl1.abs()[None, :, None, None],
            F.conv2d(x.abs(), w.m1.abs(), padding=(0, 1)) + w.bm1.abs()[None, :, None, None],
            F.conv2d(ref.a_l.abs(), w.l2.abs(), padding=(0, 1)) + F.conv2d(ref.a_m.abs(), w.m2.abs(), padding=(1, 0)) + w.b2.abs()[None, :, None, None]
            + (x.abs() if case.res else 0) + ref.d.abs() + sum(nchw(p).double().abs() for p in case.ps)]
    assert max(float(m.max()) for m in mags) * 4 < 2 ** 24
    return True


# ---- the entry point's validation: a descriptor over stand-in addresses (nothing below reads or writes them) --------------------------------
S = 1 << 20     # bytes between the stand-in tensors: more than one of them holds (1 x 32 x 40 x 128 x 2)


def step_desc(L, a, store="bf16", **kw):
    """ARFDN's third step at 1 x 32 x 40: `in` (r2) and out (r3) in pitch-32 tensors of their own, d3 and the earlier maps d2, d1 as slices of
    one pitch-128 concat tensor"""
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize, d.post_cout = 1, 32, 40, 25, 25, 3, 25
    d.in_layout = d.out_layout = L.NHWC
    d.act = d.post_act = L.ACT_LRELU
    d.slope, d.res_mode = 0.05, L.RES_PRE_ACT
    d.storage = d.compute = L.STORE[store]
    d.inp, d.out0 = L.View(a, 32, 0), L.View(a + S, 32, 0)
    d.post_out, d.res, d.tail_cat = L.View(a + 2 * S, 128, 32), L.View(a + 2 * S, 128, 64), L.View(a + 2 * S, 128, 96)
    d.wpacked = d.post_wpacked = a
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def check_refusals(L, no_gpu):
    """esr_asym_step_supported / esr_asym_step validate before anything is launched: the documented codes for every descriptor outside the range.
    no_gpu: a VALID descriptor passes every check and fails in the launch (ESR_ERR_LAUNCH); on a host with a GPU no valid one is run here --
    the addresses are stand-ins"""
    lib = L.lib()
    buf = (ctypes.c_float * 8192)()
    a = ctypes.addressof(buf)
    sup = lambda **kw: lib.esr_asym_step_supported(ctypes.byref(step_desc(L, a, **kw)))
    run = lambda **kw: lib.esr_asym_step(ctypes.byref(step_desc(L, a, **kw)), None)
    nores = dict(res_mode=L.RES_NONE)
    assert sup() == 1 and sup(store="f16") == 1 and sup(**nores) == 1 and sup(cin=50, inp=L.View(a, 56, 0), **nores) == 1
    assert sup(cin=17, post_cout=17, cout=17) == 1 and sup(cin=32, post_cout=32, cout=32) == 1 and sup(cin=64, inp=L.View(a, 64, 0), **nores) == 1
    assert sup(cout=32) == 1 and sup(act=L.ACT_RELU, post_act=L.ACT_RELU) == 1 and sup(res=L.View(None, 0, 0)) == 1
    refused = [dict(store="f32"), dict(storage=7, compute=7), dict(compute=L.COMPUTE["f16"]), dict(compute=0),
               dict(post_cout=16, cout=16, cin=16), dict(post_cout=33, cout=33, cin=33), dict(post_cout=16, cout=16, **nores), dict(post_cout=33, cout=33, **nores),
               dict(cin=65, **nores), dict(cin=16, **nores), dict(cin=50), dict(cin=26), dict(cin=24),          # `+ in` with cin != c
               dict(cout=24), dict(cout=33), dict(ksize=1), dict(act=L.ACT_GELU, post_act=L.ACT_GELU), dict(post_act=L.ACT_NONE),
               dict(res_mode=L.RES_POST_ACT), dict(res_mode=L.RES_GATE), dict(in_layout=L.NCHW_IN), dict(out_layout=L.NCHW_SHUFFLE4), dict(split=16),
               dict(tail_wpacked=a), dict(tail_cat_c=32), dict(tail_cout=32), dict(post2_wpacked=a), dict(post2_cout=8), dict(out1=L.View(a, 32, 0)),
               dict(border_bias=a), dict(blocked8=1), dict(in_seg_stride=64), dict(in_seg_chunks=2), dict(wino_wpacked=a), dict(hilo=L.HILO_OUT, hilo_stride=4096),
               dict(n=0), dict(h=0), dict(w=-1), dict(h=32768, w=32768)]
    for kw in refused:
        assert sup(**kw) == 0, kw
        assert run(**kw) == -2, kw                                                               # ESR_ERR_UNSUPPORTED
    assert lib.esr_asym_step_supported(None) == 0 and lib.esr_asym_step(None, None) == -1
    cat = lambda coff: L.View(a + 2 * S, 128, coff)
    bad = [dict(inp=L.View(None, 32, 0)), dict(out0=L.View(None, 32, 0)), dict(post_out=L.View(None, 128, 32)), dict(wpacked=None), dict(post_wpacked=None),
           dict(inp=L.View(a, 32, 8)), dict(inp=L.View(a, 28, 0)), dict(inp=L.View(a, 24, 0)), dict(inp=L.View(a, 64, 36)),       # too narrow, misaligned
           dict(out0=L.View(a + S, 24, 0)), dict(out0=L.View(a + S, 64, 20)), dict(out0=L.View(a + S, 32, 8)), dict(cout=32, out0=L.View(a + S, 48, 24)),
           dict(post_out=cat(100)), dict(post_out=L.View(a + 2 * S, 24, 0)), dict(res=cat(104)), dict(tail_cat=cat(100)), dict(res=L.View(a + 3 * S, 24, 0)),
           # each output where something is read, or where the other output goes
           dict(out0=L.View(a, 32, 0)), dict(out0=L.View(a + 16, 32, 0)), dict(out0=L.View(a, 64, 32)), dict(out0=L.View(a + 64, 32, 0)),        # out in `in`'s bytes
           dict(out0=cat(64)), dict(out0=cat(96)), dict(out0=cat(72)), dict(out0=cat(32)), dict(out0=L.View(a + 2 * S + 256, 128, 40)),          # out in p1 / p2 / d
           dict(post_out=cat(64)), dict(post_out=cat(80)), dict(post_out=cat(96)), dict(post_out=L.View(a, 32, 0)), dict(post_out=L.View(a + S, 32, 0)),
           dict(post_out=L.View(a + 2 * S + 16, 128, 0)), dict(inp=L.View(a + 2 * S, 128, 32)), dict(inp=L.View(a + S - 64, 32, 0))]
    for kw in bad:
        assert run(**kw) == -1, kw                                                               # ESR_ERR_BAD_ARG
    # allowed: d, out and `in` as disjoint slices wherever no byte is shared -- d beside p1 and p2 in the concat (the descriptor itself), out there too
    valid = (dict(), dict(store="f16"), dict(out0=cat(0)), dict(res=L.View(None, 0, 0)), dict(res=L.View(None, 0, 0), tail_cat=L.View(None, 0, 0)))
    for kw in valid:
        assert sup(**kw) == 1, kw
        if no_gpu:
            assert run(**kw) == -3, kw                                                           # ESR_ERR_LAUNCH
    op = L.Op()
    op.kind, op.conv = L.OP_ASYM_STEP, step_desc(L, a, store="f32")
    assert L.OP_ASYM_STEP == 19 and lib.esr_run_ops(ctypes.byref(op), 1, None) == -2
    op.conv = step_desc(L, a, out0=L.View(a, 32, 0))
    assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -1
    if no_gpu:
        op.conv = step_desc(L, a)
        assert lib.esr_run_ops(ctypes.byref(op), 1, None) == -3
