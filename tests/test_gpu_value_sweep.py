"""-m gpu: every finite 16-bit value through each kernel's activation and store (helper and CPU proofs: tests/_sweep.py,
tests/test_sweep_helper.py; DESIGN.md "Value sweep").

The weights are only 0 and 1 and every bias and border table is zero, so the pre-activation v of a kernel is the swept value itself:
  * residual route: zero weights, the sweep as the pre-activation residual (v = r); nothing is exempt;
  * identity route: centre-tap identity / 0-1 selection weights, the sweep as the input (v = x).  x is an MFMA operand there, and an x that
    is SUBNORMAL in the storage type may be read as zero: the reference with those inputs zeroed is accepted at those positions (254 of
    65 280 bf16 patterns, 2 046 of 63 488 f16 patterns) and nowhere else.  What the hardware did with them is printed by every case
    ("flushed k") and recorded in DESIGN.md: the MI355X kept every subnormal operand, bf16 and f16 (flushed 0 in every case).
none / ReLU / LeakyReLU and the residual adds are compared EXACTLY with the same fp32 expression on the CPU, rounded once by torch (round to
nearest even): a tie rounded away from zero, a truncating store, an Inf in the wrong place or a flushed subnormal RESULT fails.  The 16-bit
GELU polynomial exists in five copies: every kernel that evaluates it must return conv_s16_kernel's bits for the same v (a table over all
65 536 patterns, built once per storage type), and conv_s16_kernel's own result lies within B(v) + half a storage step x 1.01 of the fp64
GELU, B(v) from the CPU emulation of the polynomial (_sweep.gelu16_bound).  The sigmoid gates are held to half a storage step x 1.01 of
the fp64 result plus the smallest fp32 normal x |r| (expf(-v) overflows below v = -88.7 and the gate is then exactly 0).

SWEPT names the cases of every kernel, EXEMPT the kernels that store nothing through an activation or a 16-bit rounding;
tests/test_sweep_helper.py::test_every_kernel_is_swept_or_exempt holds the two against the __global__ kernels of csrc/."""
import ctypes
import functools
import re

import pytest
import torch

import _sweep as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STORES = ["bf16", "f16"]
SLOPE = 0.05
NONE, LRELU, RELU, GELU = 0, 1, 2, 3
RES_NONE, RES_PRE, RES_POST, RES_GATE = 0, 1, 2, 3
ACT_NAME = {NONE: "none", LRELU: "lrelu", RELU: "relu", GELU: "gelu"}

SWEPT = {
    "conv_s16_kernel": ["test_conv_s16_linear_activations_and_residuals", "test_conv_s16_four_wave_form", "test_tie_pairs_through_the_store",
                        "test_gelu16_anchor_against_fp64", "test_sigmoid_gate_16bit"],
    "conv48r_kernel": ["test_persistent_conv_kernels", "test_gelu16_copies_return_the_anchor_bits"],
    "conv48rq_kernel": ["test_persistent_conv_kernels_with_a_post", "test_gelu16_copies_return_the_anchor_bits"],
    "conv64r_kernel": ["test_persistent_conv_kernels"],
    "conv64m_kernel": ["test_persistent_conv_kernels", "test_persistent_conv_kernels_with_a_post", "test_gelu16_copies_return_the_anchor_bits"],
    "conv48rp_kernel": ["test_conv48rp_post_chain"],
    "bsconv_kernel": ["test_bsconv_16bit", "test_gelu16_copies_return_the_anchor_bits"],
    "dwconv3x3_kernel": ["test_depthwise_kernels"],
    "dwconv7x7_kernel": ["test_depthwise_kernels"],
    "pack_input_kernel": ["test_tie_pairs_through_the_store"],
    "ca_apply_nhwc_kernel": ["test_channel_attention_gate"],
    "ca_apply_nchw_kernel": ["test_fp32_storage"],
    "esa_apply_mfma_kernel": ["test_esa_apply_mfma_gate_and_posts", "test_gelu16_copies_return_the_anchor_bits"],
    "rlfb_chain_kernel": ["test_rlfb_chain"],
    "hfab_kernel": ["test_hfab"],
    "rfdb_tail_kernel": ["test_rfdb_tail", "test_gelu16_copies_return_the_anchor_bits"],
    "refine_cascade_kernel": ["test_refine_cascade"],
    "distill_step_kernel": ["test_distill_step"],
    "resblock_head_kernel": ["test_resblock_head"],
    "cx_block_kernel": ["test_cx_block"],
    "conv_f32_kernel": ["test_fp32_storage"],
    "wino_f32_kernel": ["test_fp32_storage"],
    "esa_apply_kernel": ["test_fp32_storage"],
}
EXEMPT = {
    "ca_reduce_nhwc_kernel": "a reduction: fp64 sums of the input, no activation and no 16-bit store",
    "ca_reduce_nchw_kernel": "a reduction: fp64 sums of the input, no activation and no 16-bit store",
    "esa_pool7_kernel": "max pooling into an fp32 low-resolution map: a selection, nothing is rounded",
    "esa_pool7_branch_kernel": "low-resolution fp32 ESA branch: accumulating 3x3 layers, checked against fp64 by the ESA cases",
    "esa_s2pool_kernel": "low-resolution fp32 ESA: strided conv + max pooling into an fp32 map",
    "esa_s2pool16_kernel": "low-resolution fp32 ESA: strided conv + max pooling into an fp32 map",
    "esa_chain_kernel": "low-resolution fp32 ESA layers: ReLU / none on accumulated fp32 sums, fp32 store",
    "conv3x3s2_kernel": "low-resolution fp32 ESA: the strided conv2, fp32 store, no activation",
    "maxpool7s3_kernel": "max pooling of an fp32 map: a selection, nothing is rounded",
    "ssim_u8_kernel": "a metric on uint8 images: fp64 partial sums",
    "sqerr_u8_kernel": "a metric on uint8 images: an integer sum",
    "tensor2uint_kernel": "the uint8 conversion of the metrics path: no activation, no 16-bit store",
    "tensor2uint_chk_kernel": "the uint8 conversion of the metrics path: no activation, no 16-bit store",
    "bw_probe_kernel": "a bandwidth probe: copies bytes",
    "event_probe_kernel": "a timing probe: copies bytes",
    "imdb_tail_kernel": "fp32 storage, LeakyReLU on accumulated sums only: conv_f32_kernel's epilogue arithmetic, which test_fp32_storage sweeps",
    "wino8_f32_kernel": "fp32 storage and no residual input: no exact route through the Winograd transforms; its activation is wn_act4, swept on wino_f32_kernel",
}


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def _up(v, m):
    return (v + m - 1) // m * m


def _bf(store):
    return "true" if store == "bf16" else "false"


@functools.lru_cache(maxsize=None)
def _sweep(store):
    return S.all_finite(S.DTYPES[store])


@functools.lru_cache(maxsize=None)
def _perm(store):
    return S.permuted(_sweep(store))


def _traced(pattern, fn):
    """fn() under ops.kernel_trace(); the ONE device symbol it launched must match `pattern`"""
    from ntire2022_esr_amd import ops
    with ops.kernel_trace() as names:
        out = fn()
    torch.cuda.synchronize()
    assert len(names) == 1 and re.match(pattern, names[0]), (names, pattern)
    return out, names[0]


def _act32(v, act):
    """the epilogue's activation as the same fp32 expression on the CPU: max(v, slope * v), slope 1 / 0.05 / 0 (fmax: the maxNum of v_max_f32)"""
    slope = {NONE: 1.0, LRELU: SLOPE, RELU: 0.0}[act]
    return torch.fmax(v, torch.tensor(slope, dtype=torch.float32) * v)


def _flush(x):
    """x with its subnormal values (of its own type) read as zero"""
    return torch.where(S.is_subnormal(x), torch.zeros_like(x), x)


def _expr(conv, r, act, res_mode, dt):
    """act(conv + r) / act(conv) + r / act(conv) in fp32, rounded once to dt.  Positions whose fp32 sum overflows are out of scope (the ABI
    requires finite values): they are returned in a mask."""
    pre = conv + r if res_mode == RES_PRE else conv
    y = _act32(pre, act)
    if res_mode == RES_POST:
        y = y + r
    return y.to(dt), ~torch.isfinite(pre) | ~torch.isfinite(y)


def _seen(t32, dt):
    """an fp32 tensor as the 1x1 of a post chain reads it: bf16 -- the 16-bit high part + the 16-bit low part of the remainder (two MFMA k
    slots, summed exactly in fp32); f16 -- the high part alone (11 bits are the storage precision)"""
    hi = t32.to(dt)
    if dt == torch.float16:
        return hi.float()
    lo = torch.where(torch.isfinite(hi.float()), (t32 - hi.float()).to(dt).float(), torch.zeros_like(t32))
    return hi.float() + lo


def _report(what, name, took, n_exempt=None):
    print(f"{what}: {name}" + ("" if n_exempt is None else f"; subnormal inputs flushed {took} of {n_exempt}"))


# ---- the generic conv case ------------------------------------------------------------------------------------------------------------------
def _conv_case(store, shape, cin, cout, k, weights, act, res_mode, kernel, *, res_in=False, border=False, gelu_lut=None, what=""):
    """ops.conv2d on the tiled sweep with zero / identity weights.  x = the sweep, r = the input itself (res_in) or the permuted sweep.
    Returns nothing: compares, prints, raises."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n, h, w = shape
    x = S.tile(_sweep(store), (n, h, w, _up(cin, 16)), cin)
    r = None
    if res_mode != RES_NONE:
        r = x if res_in else S.tile(_perm(store), (n, h, w, _up(cout, 8)), cout)
    wt = S.identity_weight(cout, cin, k) if weights == "identity" else S.zero_weight(cout, cin, k)
    kw = dict(act=act, slope=SLOPE, cin=cin)
    xd = x.to(DEV)
    if r is not None:
        kw.update(res=xd if res_in else r.to(DEV), res_mode=res_mode)
    if border:
        kw.update(border=torch.zeros(16, _up(cout, 16), device=DEV))
    y, name = _traced(kernel, lambda: ops.conv2d(xd, wt, torch.zeros(cout), **kw))
    assert y.dtype == dt and tuple(y.shape) == (n, h, w, _up(cout, 8))
    y = y.cpu()
    assert cout % 8 == 0 or float(y[..., cout:].float().abs().max()) == 0.0
    got = y[..., :cout]
    idx = torch.arange(cout) % cin
    rf = None if r is None else r[..., :cout].float()
    zero = torch.zeros(n, h, w, cout)
    refs = []
    for xin in (x, _flush(x)):
        conv = xin[..., idx].float() if weights == "identity" else zero
        if act == GELU:
            assert res_mode in (RES_NONE, RES_PRE) and not (weights == "identity" and res_mode == RES_PRE), "v must be one 16-bit value"
            v16 = r[..., :cout] if res_mode == RES_PRE else xin[..., idx]
            refs.append((S.from_bits(gelu_lut[S.to_bits(v16).long()], dt), torch.zeros_like(conv, dtype=torch.bool)))
        else:
            refs.append(_expr(conv, rf if rf is not None else zero, act, res_mode, dt))
    (want, skip), (alt, _) = refs
    got = torch.where(skip, want, got)
    vmsg = (x[..., idx] if weights == "identity" else r[..., :cout]).float()
    label = f"{what or 'conv'} {store} {cin}->{cout} k{k} {weights} {ACT_NAME[act]} res{res_mode}{' =in' if res_in else ''} {n}x{h}x{w}"
    took = S.exact(got, want, dt, v=vmsg, flushed=alt if weights == "identity" else None, what=label)
    _report(label, name, took, int(S.is_subnormal(x[..., idx]).sum()) if weights == "identity" else None)


# ---- the anchor of the GELU group: conv_s16_kernel over all patterns -----------------------------------------------------------------------
S16_8W = r"conv_s16_kernel<\d, [13], 8, (true|false), (true|false), \d, \d, false>"
S16_4W = r"conv_s16_kernel<3, 3, 4, (true|false), false, 0, 0, false>"


@functools.lru_cache(maxsize=None)
def _gelu_lut(store):
    """bits of conv_s16_kernel's GELU for every finite pattern of the storage type (-1 elsewhere): zero 1x1 weights, the sweep as the
    pre-activation residual.  1 x 32 x 32 x 64 holds 65 536 values: 256 patterns twice, which must agree."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    v = S.tile(_sweep(store), (1, 32, 32, 64))
    x = S.tile(_perm(store), (1, 32, 32, 64)).to(DEV)
    y, _ = _traced(S16_8W, lambda: ops.conv2d(x, S.zero_weight(64, 64, 1), torch.zeros(64), act=GELU, res=v.to(DEV), res_mode=RES_PRE))
    vb, yb = S.to_bits(v).reshape(-1).long(), S.to_bits(y.cpu()).reshape(-1)
    lut = torch.full((65536,), -1, dtype=torch.int32)
    lut[vb] = yb
    assert bool((lut[vb] == yb).all()), "one v, two results"
    assert int((lut >= 0).sum()) == S.N_FINITE[dt]
    return lut


@pytest.mark.parametrize("store", STORES)
def test_gelu16_anchor_against_fp64(store):
    """conv_s16_kernel's GELU over every finite pattern: within B(v) + half a storage step x 1.01 of fp64 F.gelu, B(v) from the emulation
    (2.13e-4 below -4, where the documents said 1.3e-4; 1.3e-4 on [-4, 4]; 5.3e-5 v above 4).  Measured on the MI355X: bit-identical to the
    CPU emulation gelu16_cpu for every pattern of both types; worst |got - GELU| 7.77e-3 (bf16, 0.998 of the bound) and 1.04e-3 (f16,
    0.998), both at the large values where half a storage step dominates; 2.127e-4 for every v < -4."""
    dt = S.DTYPES[store]
    sw = _sweep(store)
    got = S.from_bits(_gelu_lut(store)[S.to_bits(sw).long()], dt)
    ref = S.gelu_f64(sw)
    worst, share = S.within(got, ref, S.gelu16_bound(sw) + S.store_tol(ref, dt), v=sw, what=f"gelu16 anchor {store}")
    emu = S.gelu16_cpu(sw).to(dt)
    below = (got.double() - ref).abs()[sw.double() < -4]
    print(f"gelu16 anchor {store}: max|got - GELU| = {worst:.3e} ({share:.3f} of the bound); max on v < -4: {float(below.max()):.4e}; "
          f"{int((got.float() != emu.float()).sum())} of {sw.numel()} patterns differ from gelu16_cpu")
    # a second launch at another shape and in another lane order gives the table's bits
    _conv_case(store, (2, 23, 37), 48, 48, 3, "zero", GELU, RES_PRE, S16_8W, gelu_lut=_gelu_lut(store), what="anchor again")


# ---- Part A: conv_s16_kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_conv_s16_linear_activations_and_residuals(store):
    """conv_s16_kernel (8 waves): none / ReLU / LeakyReLU x no / pre- / post-activation residual x zero / identity weights, 3x3 over 48
    channels at 2 x 23 x 37 and the 1x1 (hi + lo weights) over unequal widths; exact against the fp32 expression"""
    for weights in ("zero", "identity"):
        for act in (NONE, RELU, LRELU):
            for res_mode in (RES_NONE, RES_PRE, RES_POST):
                if weights == "zero" and res_mode == RES_NONE:
                    continue
                _conv_case(store, (2, 23, 37), 48, 48, 3, weights, act, res_mode, S16_8W)
    n, h, w = S.shape_for(_sweep(store), 25)
    for act, res_mode in ((LRELU, RES_NONE), (RELU, RES_PRE), (NONE, RES_POST)):
        _conv_case(store, (n, h, w), 25, 50, 1, "identity", act, res_mode, S16_8W)
    _conv_case(store, (n, h, w), 50, 25, 1, "zero", LRELU, RES_PRE, S16_8W)
    _conv_case(store, (2, 23, 37), 48, 48, 3, "identity", LRELU, RES_PRE, S16_8W, res_in=True)         # v = 2 x, the residual from the staged tile


@pytest.mark.parametrize("store", STORES)
def test_conv_s16_four_wave_form(store):
    """conv_s16_kernel on 16 x 16 tiles with two blocks per CU: 32 -> 48 from 512 tiles (48 inputs at that size are conv48r_kernel's), so the
    identity route only -- the form takes no residual from HBM"""
    lut = _gelu_lut(store)
    for act in (NONE, RELU, LRELU, GELU):
        _conv_case(store, (2, 250, 259), 32, 48, 3, "identity", act, RES_NONE, S16_4W, gelu_lut=lut, what="4-wave")


@pytest.mark.parametrize("store", STORES)
def test_tie_pairs_through_the_store(store):
    """x + r exactly on, and a quarter step to either side of, every rounding boundary of the storage type: identity + post-activation
    residual on conv_s16_kernel (the sum is exact in fp32, the store rounds it), and the same sums as fp32 inputs of pack_input_kernel
    (high part = the rounded sum, low part = the rounded remainder).  f16: +-65504 +- 16 must store +-Inf as torch does."""
    from ntire2022_esr_amd import _lib as L, ops
    dt = S.DTYPES[store]
    x, r, info = S.tie_pairs(dt)
    c = 48
    npix = -(-x.numel() // c)
    h = w = int(npix ** 0.5) + 1
    pad = h * w * c - x.numel()
    xt = torch.cat([x, torch.zeros(pad, dtype=dt)]).reshape(1, h, w, c)
    rt = torch.cat([r, torch.zeros(pad, dtype=dt)]).reshape(1, h, w, c)
    want = (xt.float() + rt.float()).to(dt)
    y, name = _traced(S16_8W, lambda: ops.conv2d(xt.to(DEV), S.identity_weight(c, c, 3), torch.zeros(c), act=NONE, res=rt.to(DEV), res_mode=RES_POST))
    S.exact(y.cpu(), want, dt, v=xt.float() + rt.float(), what=f"tie pairs {store} conv_s16")
    _report(f"tie pairs {store} 1x{h}x{w}x{c}: {info}", name, 0)
    # pack_input_kernel: three planes of fp32 sums
    s = x.float() + r.float()
    hw = -(-s.numel() // 3)
    ph = int(hw ** 0.5) + 1
    pw = -(-hw // ph)
    planes = torch.cat([s, torch.zeros(3 * ph * pw - s.numel())]).reshape(1, 3, ph, pw).contiguous()
    xin = planes.to(DEV)
    slots = torch.full((1, ph, pw, 16), 7.0, dtype=dt, device=DEV)
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.storage = 1, ph, pw, 3, L.STORE[store]
    d.inp = L.View(ctypes.c_void_p(xin.data_ptr()), 0, 0)
    d.out0 = L.View(ctypes.c_void_p(slots.data_ptr()), 16, 0)
    _, name = _traced(rf"pack_input_kernel<{_bf(store)}>", lambda: ops._launch(L.OP_PACK_INPUT, d, torch.cuda.current_stream().cuda_stream))
    got = slots.cpu()
    f = planes.permute(0, 2, 3, 1)
    hi = f.to(dt)
    lo = (f - hi.float()).to(dt)
    fin = torch.isfinite(hi.float())                       # (f16: the remainder of an Inf high part is -Inf - Inf arithmetic, not a store)
    S.exact(got[..., 0:3], hi, dt, v=f, what=f"pack_input {store} high parts")
    S.exact(torch.where(fin, got[..., 3:6], lo), lo, dt, v=f, what=f"pack_input {store} low parts")
    S.exact(got[..., 6:9], hi, dt, v=f, what=f"pack_input {store} high parts again")
    assert float(got[..., 9:].float().abs().max()) == 0.0
    _report(f"pack_input {store} 1x3x{ph}x{pw}", name, 0)


@pytest.mark.parametrize("store", STORES)
def test_sigmoid_gate_16bit(store):
    """ESR_RES_GATE on conv_s16_kernel: sigmoid(v) * r with v = the sweep through identity weights, r = 1 and r = the permuted sweep"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n, h, w = 2, 23, 37
    x = S.tile(_sweep(store), (n, h, w, 48))
    for rname, r in (("1", torch.ones(n, h, w, 48, dtype=dt)), ("sweep", S.tile(_perm(store), (n, h, w, 48)))):
        y, name = _traced(S16_8W, lambda: ops.conv2d(x.to(DEV), S.identity_weight(48, 48, 3), torch.zeros(48), res=r.to(DEV), res_mode=RES_GATE))
        ref = S.sigmoid_f64(x) * r.double()
        worst, share = S.within(y.cpu(), ref, S.store_tol(ref, dt) + S.F32_MIN_NORMAL * r.double().abs(), v=x.float(), what=f"gate {store} r={rname}")
        print(f"gate {store} r={rname}: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")


# ---- Part A: the persistent register-resident kernels ----------------------------------------------------------------------------------------
BIG32 = (1, 250, 520)          # 33 x 8 = 264 tiles of 16 x 32, ragged in both directions (conv48r_kernel's threshold is 256)
BIG16 = (1, 250, 259)          # 17 x 16 = 272 tiles of 16 x 16 (conv48rq / conv64r / conv64m: 256)


@pytest.mark.parametrize("store", STORES)
def test_persistent_conv_kernels(store):
    """conv48r_kernel (plain and with the residual = input), conv64r_kernel (two output tiles) and conv64m_kernel (four): they take no
    residual from HBM, so the residual route runs with res = the input and zero weights, the identity route without a residual"""
    bf = _bf(store)
    for act in (NONE, RELU, LRELU):
        _conv_case(store, BIG32, 48, 48, 3, "identity", act, RES_NONE, rf"conv48r_kernel<{bf}, 3, false, 4,", what="conv48r")
        _conv_case(store, BIG32, 48, 48, 3, "zero", act, RES_PRE, rf"conv48r_kernel<{bf}, 3, true, 4,", res_in=True, what="conv48r")
    for act in (NONE, LRELU):
        _conv_case(store, BIG16, 64, 32, 3, "identity", act, RES_NONE, rf"conv64r_kernel<{bf}, 2,", what="conv64r")
        _conv_case(store, BIG16, 64, 64, 3, "identity", act, RES_NONE, rf"conv64m_kernel<{bf}, false, false, 4, false>", what="conv64m")
        _conv_case(store, BIG16, 64, 64, 3, "zero", act, RES_PRE, rf"conv64m_kernel<{bf}, false, false, 4, false>", res_in=True, what="conv64m")
    _conv_case(store, BIG16, 64, 64, 3, "identity", RELU, RES_PRE, rf"conv64m_kernel<{bf}, false, false, 4, false>", res_in=True, what="conv64m")


def _post_case(store, shape, cin, cout, pc, act, post_act, kernel, *, weights="zero", res="in", border=False, pc2=0, store_main=True, gelu_lut=None,
               what=""):
    """a conv with a post 1x1 (and a second one) in its epilogue: main result u = act(conv(x) + x) (res "in", pre-activation), act(conv(x))
    (res "none") or act(conv(x)) + r (res "hbm", post-activation, r = the permuted sweep) -- stored unless store_main is off --, post = post_act(S . u) with
    S a 0 / 1 selection, post2 = S2 . post.  A post reads its fp32 input as _seen() emulates it (bf16: hi + lo parts, f16: the high part), so
    every output is compared exactly -- but for a bf16 post behind the GELU, whose fp32 input is known from the emulation only: half a
    storage step x 1.01 + 2^-15 |ref| there."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n, h, w = shape
    x = S.tile(_sweep(store), (n, h, w, _up(cin, 16)), cin)
    wt = S.identity_weight(cout, cin, 3) if weights == "identity" else S.zero_weight(cout, cin, 3)
    sel, sel2 = S.selection(pc, cout), (S.selection(pc2, pc) if pc2 else None)
    xd = x.to(DEV)
    kw = dict(act=act, slope=SLOPE, cin=cin, post_weight=sel, post_bias=torch.zeros(pc), post_act=post_act, store_main=store_main)
    r = None
    if res == "in":
        kw.update(res=xd, res_mode=RES_PRE)
    elif res == "hbm":
        # (identity weights: a zero residual -- a second operand would carry u past the largest finite value, and the 1x1 multiplies EVERY
        # channel of the pixel by its 0 / 1 weights: 0 x Inf)
        r = S.tile(_perm(store), (n, h, w, _up(cout, 8)), cout) if weights == "zero" else torch.zeros(n, h, w, _up(cout, 8), dtype=dt)
        kw.update(res=r.to(DEV), res_mode=RES_POST)
    if border:
        kw.update(border=torch.zeros(16, _up(cout, 16), device=DEV))
    if pc2:
        kw.update(post2_weight=sel2, post2_bias=torch.zeros(pc2))
    outs, name = _traced(kernel, lambda: ops.conv2d(xd, wt, torch.zeros(cout), **kw))
    y, p = outs[0], outs[1].cpu()
    idx, pidx = torch.arange(cout) % cin, torch.arange(pc) % cout
    label = f"{what} {store} {cin}->{cout}+{pc}{'+' + str(pc2) if pc2 else ''} {weights} {ACT_NAME[act]}/{ACT_NAME[post_act]} res={res} {n}x{h}x{w}"
    took = n_ex = 0
    refs = []
    for xin in (x, _flush(x)):
        conv = xin[..., idx].float() if weights == "identity" else torch.zeros(n, h, w, cout)
        if act == GELU:
            assert weights == "zero" and res == "in"
            u16 = S.from_bits(gelu_lut[S.to_bits(xin[..., idx]).long()], dt)
            u32, skip = S.gelu16_cpu(xin[..., idx]), torch.zeros(n, h, w, cout, dtype=torch.bool)
        elif res == "in":
            u16, skip = _expr(conv, xin[..., idx].float(), act, RES_PRE, dt)
            u32 = _act32(conv + xin[..., idx].float(), act)
        elif res == "none":
            u16, skip = _expr(conv, None, act, RES_NONE, dt)
            u32 = _act32(conv, act)
        else:
            u16, skip = _expr(conv, r[..., :cout].float(), act, RES_POST, dt)
            u32 = _act32(conv, act) + r[..., :cout].float()
        refs.append((u16, u32, skip))
    (u16, u32, skip), (u16f, u32f, _) = refs
    vmsg = x[..., idx].float()
    if store_main:
        yc = y.cpu()[..., :cout]
        took = S.exact(torch.where(skip, u16, yc), u16, dt, v=vmsg, flushed=u16f if weights == "identity" else None, what=label + " main")
        n_ex = int(S.is_subnormal(x[..., idx]).sum())
    if act == GELU and dt == torch.float16:
        u32, u32f = u16.float(), u16f.float()                # (the emulation is not the reference of a bit-exact check: f16 posts read the stored bits)
    s32, s32f = _seen(u32, dt), _seen(u32f, dt)
    pgot = p[..., :pc]
    assert pc % 8 == 0 or float(p[..., pc:].float().abs().max()) == 0.0
    pskip = skip[..., pidx]
    if post_act == GELU:
        # GELU of the post: its argument must be ONE 16-bit value for the table (u itself when it is a 16-bit value; f16: its stored rounding)
        assert bool((s32.to(dt).float() == s32)[~skip].all()), "a GELU post needs a 16-bit argument"
        pwant = S.from_bits(gelu_lut[S.to_bits(s32.to(dt)[..., pidx]).long()], dt)
        pflush = S.from_bits(gelu_lut[S.to_bits(s32f.to(dt)[..., pidx]).long()], dt)
        p32 = pwant.float()
    else:
        p32 = _act32(s32[..., pidx], post_act)
        pwant, pflush = p32.to(dt), _act32(s32f[..., pidx], post_act).to(dt)
    if act == GELU and dt == torch.bfloat16 and post_act != GELU:
        # bf16: the post reads the polynomial's fp32 result as hi + lo; the emulation of that result carries the tolerance, not the bits
        ref = p32.double()
        worst, share = S.within(pgot, ref, S.store_tol(ref, dt) + ref.abs() * 2.0 ** -15, v=vmsg[..., pidx], what=label + " post")
        print(f"{label} post (hi + lo of an emulated fp32 value): max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    else:
        S.exact(torch.where(pskip, pwant, pgot), pwant, dt, v=vmsg[..., pidx], flushed=pflush if weights == "identity" else None, what=label + " post")
    if pc2:
        p2 = outs[2].cpu()
        p2idx = torch.arange(pc2) % pc
        want2 = _seen(p32, dt)[..., p2idx].to(dt)
        S.exact(torch.where(pskip[..., p2idx], want2, p2[..., :pc2]), want2, dt, v=vmsg[..., pidx][..., p2idx], what=label + " post2")
    _report(label, name, took, n_ex if weights == "identity" and store_main else None)


@pytest.mark.parametrize("store", STORES)
def test_persistent_conv_kernels_with_a_post(store):
    """conv64m_kernel with the next distillation 1x1 in its epilogue (both types) and conv48rq_kernel (f16 only)"""
    bf = _bf(store)
    k64 = rf"conv64m_kernel<{bf}, true, false, 4, false>"
    for act, pact in ((NONE, NONE), (NONE, LRELU), (NONE, RELU), (LRELU, NONE), (LRELU, LRELU)):
        _post_case(store, BIG16, 64, 64, 32, act, pact, k64, what="conv64m post")
    _post_case(store, BIG16, 64, 64, 25, LRELU, LRELU, k64, weights="identity", res="none", what="conv64m post")
    if store == "f16":
        for act, pact in ((NONE, NONE), (NONE, LRELU), (LRELU, NONE), (RELU, RELU)):
            _post_case(store, BIG16, 48, 48, 24, act, pact, r"conv48rq_kernel<false,", what="conv48rq")


@pytest.mark.parametrize("store", STORES)
def test_conv48rp_post_chain(store):
    """conv48rp_kernel (RLFB c3_r: 48 -> 48 + a post-activation residual from HBM, not stored, then c5 and esa.conv1 as 0 / 1 selections):
    zero weights make u = r, the sweep, and v = post_act(u) exact; identity weights with LeakyReLU make u an fp32 value that the post reads
    as hi + lo parts"""
    k = rf"conv48rp_kernel<{_bf(store)}, false>"
    for act, pact in ((NONE, NONE), (LRELU, NONE), (RELU, NONE)):
        _post_case(store, BIG16, 48, 46, 46, act, pact, k, res="hbm", pc2=16, store_main=False, what="conv48rp")
    _post_case(store, BIG16, 48, 46, 46, LRELU, NONE, k, weights="identity", res="hbm", pc2=16, store_main=False, what="conv48rp")


@pytest.mark.parametrize("store", STORES)
def test_gelu16_copies_return_the_anchor_bits(store):
    """every kernel that evaluates the 16-bit GELU polynomial -- gelu16x4 in conv48r / conv48rq / conv64m (both forms), the scalar gelu16 of
    esr_bsconv.hip, esr_gelu16 in esa_apply_mfma_kernel's post chain, rfdb_tail_kernel's -- against conv_s16_kernel's bits for the same v
    (bsconv, the ESA post and the tail: in their own cases, with the same table)"""
    lut = _gelu_lut(store)
    bf = _bf(store)
    _conv_case(store, BIG32, 48, 32, 3, "identity", GELU, RES_NONE, rf"conv48r_kernel<{bf}, 2, true, 4,", border=True, gelu_lut=lut, what="conv48r gelu")
    _conv_case(store, BIG16, 48, 48, 3, "zero", GELU, RES_PRE, rf"conv64m_kernel<{bf}, false, false, 3, true>", res_in=True, border=True, gelu_lut=lut,
               what="conv64m 3-chunk gelu")
    if store == "f16":
        _post_case(store, BIG16, 48, 48, 24, GELU, LRELU, r"conv48rq_kernel<false,", border=True, gelu_lut=lut, what="conv48rq gelu")
        _post_case(store, BIG16, 48, 48, 24, NONE, GELU, r"conv48rq_kernel<false,", gelu_lut=lut, what="conv48rq post gelu")
        _post_case(store, BIG16, 48, 48, 24, GELU, GELU, r"conv64m_kernel<false, true, false, 3, true>", border=True, gelu_lut=lut, what="conv64m 3-chunk gelu post")


# ---- Part A: BSConvU, the depthwise kernels, channel attention, the ESA tail ------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES)
def test_bsconv_16bit(store):
    """bsconv_kernel in 16-bit storage: pointwise identity (or zero), depthwise centre tap 1; every activation x no / pre / post residual
    on the main output and the distillation 1x1 (a selection of the input) with every activation.  GELU: the scalar gelu16 of
    esr_bsconv.hip against conv_s16_kernel's bits."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    lut = _gelu_lut(store)
    n, h, w, c, dc = 2, 23, 37, 48, 24
    x = S.tile(_sweep(store), (n, h, w, c))
    r = S.tile(_perm(store), (n, h, w, c))
    dw = S.dw_identity(c, 3)
    didx = torch.arange(dc) % c
    for pw_kind in ("identity", "zero"):
        pw = S.selection(c, c) if pw_kind == "identity" else torch.zeros(c, c)
        for act in (NONE, RELU, LRELU, GELU):
            for res_mode in (RES_NONE, RES_PRE, RES_POST):
                if (pw_kind == "zero" and res_mode != RES_PRE) or (act == GELU and (res_mode == RES_POST or (pw_kind == "identity" and res_mode == RES_PRE))):
                    continue
                (y, yd), name = _traced(rf"bsconv_kernel<3, 2, {ops.L.STORE[store]}>", lambda: ops.bsconv(
                    x.to(DEV), pw, torch.zeros(c), dw, torch.zeros(c), act=act, slope=SLOPE, res=None if res_mode == RES_NONE else r.to(DEV), res_mode=res_mode,
                    d_weight=S.selection(dc, c), d_bias=torch.zeros(dc), d_act=act))
                refs = []
                for xin in (x, _flush(x)):
                    conv = xin.float() if pw_kind == "identity" else torch.zeros(n, h, w, c)
                    if act == GELU:
                        v16 = r if res_mode == RES_PRE else xin
                        main, skip = S.from_bits(lut[S.to_bits(v16).long()], dt), torch.zeros(n, h, w, c, dtype=torch.bool)
                        dist = S.from_bits(lut[S.to_bits(xin[..., didx]).long()], dt)
                    else:
                        main, skip = _expr(conv, r.float(), act, res_mode, dt)
                        dist = _act32(xin[..., didx].float(), act).to(dt)
                    refs.append((main, dist, skip))
                (main, dist, skip), (mainf, distf, _) = refs
                label = f"bsconv {store} pw={pw_kind} {ACT_NAME[act]} res{res_mode}"
                took = S.exact(torch.where(skip, main, y.cpu()[..., :c]), main, dt, v=(x if pw_kind == "identity" else r).float(),
                               flushed=mainf if pw_kind == "identity" else None, what=label)
                took_d = S.exact(yd.cpu()[..., :dc], dist, dt, v=x[..., didx].float(), flushed=distf, what=label + " distilled")
                _report(label, name, took + took_d, int(S.is_subnormal(x).sum()) * (1 if pw_kind == "zero" else 2))


@pytest.mark.parametrize("store", STORES)
def test_depthwise_kernels(store):
    """dwconv3x3_kernel (centre tap 1: v = x, VALU arithmetic, so nothing is exempt; none / ReLU / LeakyReLU x no / pre / post residual exact,
    its GELU -- erff in every storage type -- against fp64) and dwconv7x7_kernel (no activation: the store alone)"""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_dw
    dt = S.DTYPES[store]
    n, h, w, c = 2, 23, 37, 48
    x, r = S.tile(_sweep(store), (n, h, w, c)), S.tile(_perm(store), (n, h, w, c))
    xd, rd = x.to(DEV), r.to(DEV)
    for wkind in ("identity", "zero"):
        pk = pack_dw(S.dw_identity(c, 3) if wkind == "identity" else torch.zeros(c, 1, 3, 3), torch.zeros(c)).to(DEV)
        for act in (NONE, RELU, LRELU, GELU):
            for res_mode in (RES_NONE, RES_PRE, RES_POST):
                if (wkind == "zero" and res_mode != RES_PRE) or (act == GELU and (res_mode == RES_POST or (wkind == "identity" and res_mode == RES_PRE))):
                    continue
                y = torch.full((n, h, w, c), 7.0, dtype=dt, device=DEV)
                d = L.ConvDesc()
                d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, c, c, 3
                d.act, d.slope, d.res_mode, d.storage = act, SLOPE, res_mode, L.STORE[store]
                d.inp = L.View(ctypes.c_void_p(xd.data_ptr()), c, 0)
                d.out0 = L.View(ctypes.c_void_p(y.data_ptr()), c, 0)
                d.res = L.View(ctypes.c_void_p(rd.data_ptr()), c, 0)
                d.wpacked = pk.data_ptr()
                stream = torch.cuda.current_stream().cuda_stream
                _, name = _traced(rf"dwconv3x3_kernel<{L.STORE[store]}>", lambda: ops._launch(L.OP_DWCONV, d, stream))
                label = f"dwconv3x3 {store} {wkind} {ACT_NAME[act]} res{res_mode}"
                conv = x.float() if wkind == "identity" else torch.zeros(n, h, w, c)
                if act == GELU:
                    v = r if res_mode == RES_PRE else x
                    ref = S.gelu_f64(v)
                    worst, share = S.within(y.cpu(), ref, S.store_tol(ref, dt) + S.f32_tol(ref) + v.double().abs() * 2.0 ** -21, v=v.float(), what=label)
                    print(f"{label}: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
                else:
                    want, skip = _expr(conv, r.float(), act, res_mode, dt)
                    S.exact(torch.where(skip, want, y.cpu()), want, dt, v=(x if wkind == "identity" else r).float(), what=label)
                    _report(label, name, 0)
    y, name = _traced(rf"dwconv7x7_kernel<{L.STORE[store]}>", lambda: ops.dwconv7x7(xd, S.dw_identity(c, 7), torch.zeros(c)))
    S.exact(y.cpu()[..., :c], x, dt, v=x.float(), what=f"dwconv7x7 {store}")
    _report(f"dwconv7x7 {store}", name, 0)


GATE_BIASES = [-3.0e38, -65504.0, -104.0, -89.0, -88.75, -88.7, -88.5, -87.5, -87.0, -40.0, -17.0, -16.5, -10.0, -4.0, -1.0, -0.5, -2.0 ** -20, -0.0, 0.0,
               2.0 ** -126, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 17.0, 40.0, 88.0, 89.0, 65504.0]


@pytest.mark.parametrize("store", STORES)
def test_channel_attention_gate(store):
    """ca_apply_nhwc_kernel: w2 = 0 makes the gate sigmoid(b2[ch]); the sweep goes through x, so every value meets 32 gates from both ends of
    expf's range, and the product is rounded once.  (esr_channel_attention_f32 has no op kind, so ops.kernel_trace() cannot name its
    kernels; NHWC + the storage type select ca_reduce_nhwc_kernel + ca_apply_nhwc_kernel<storage> in its one switch.)"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    c, cr = 64, 4
    n, h, w = 2, 23, 37
    b2 = torch.tensor(GATE_BIASES * 2, dtype=torch.float32)
    assert b2.numel() == c
    x = S.tile(_sweep(store), (n, h, w, c))
    y = ops.channel_attention(x.to(DEV), torch.zeros(cr, c), torch.zeros(cr), torch.zeros(c, cr), b2)
    torch.cuda.synchronize()
    gate = S.sigmoid_f64(b2)[None, None, None, :]
    ref = gate * x.double()
    worst, share = S.within(y.cpu(), ref, S.store_tol(ref, dt) + S.F32_MIN_NORMAL * x.double().abs(), v=x.float(), what=f"channel attention {store}")
    print(f"channel attention {store} NHWC: max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")


@pytest.mark.parametrize("store", STORES)
def test_esa_apply_mfma_gate_and_posts(store):
    """esa_apply_mfma_kernel: c3 = 0, conv_f = identity, w4[ch, ch mod 16] = 1 make m[ch] = c1[ch mod 16], the sweep, exactly; y = x *
    sigmoid(m) with x = 1 and x = the permuted sweep, the gate's tolerance (v_rcp(1 + v_exp(..)) here).  Post chain: zero weights and the
    sweep as the pre-activation residual make post 0 = act(r) exactly -- none / ReLU / LeakyReLU exact, GELU (esr_gelu16) against
    conv_s16_kernel's bits --, post 1 a selection of post 0's fp32 result read as hi + lo parts (f16: as its stored rounding)."""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    lut = _gelu_lut(store)
    c, f = 64, 16
    n, h, w = S.shape_for(_sweep(store), f)
    c1 = S.tile(_sweep(store), (n, h, w, f))
    c3 = torch.zeros(n, 2, 2, 16, device=DEV)
    wf, w4 = torch.eye(f), S.selection(c, f)
    m = c1[..., torch.arange(c) % f]
    st = ops.L.STORE[store]
    for xname, x in (("1", torch.ones(n, h, w, c, dtype=dt)), ("sweep", S.tile(_perm(store), (n, h, w, c)))):
        y, name = _traced(rf"esa_apply_mfma_kernel<{st}, 2, 0, 0>", lambda: ops.esa_apply(x.to(DEV), c1.to(DEV), c3, wf, torch.zeros(f), w4, torch.zeros(c)))
        ref = S.sigmoid_f64(m) * x.double()
        worst, share = S.within(y.cpu(), ref, S.store_tol(ref, dt) + S.F32_MIN_NORMAL * x.double().abs(), v=m.float(), what=f"esa apply {store} x={xname}")
        print(f"esa apply {store} x={xname} {n}x{h}x{w}: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    # post chain on the residual route
    x = torch.ones(n, h, w, c, dtype=dt)
    r = S.tile(_sweep(store), (n, h, w, 48))
    p2idx = torch.arange(24) % 48
    for act in (NONE, RELU, LRELU, GELU):
        post = [dict(weight=torch.zeros(48, c), bias=torch.zeros(48), act=act, slope=SLOPE, res=r.to(DEV)),
                dict(weight=S.selection(24, 48), bias=torch.zeros(24), act=NONE)]
        (y, (p0, p1)), name = _traced(rf"esa_apply_mfma_kernel<{st}, 2, 2, 1>", lambda: ops.esa_apply(x.to(DEV), c1.to(DEV), c3, wf, torch.zeros(f), w4, torch.zeros(c),
                                                                                                    post=post))
        label = f"esa apply post {store} {ACT_NAME[act]}"
        if act == GELU:
            want = S.from_bits(lut[S.to_bits(r).long()], dt)
            p32 = S.gelu16_cpu(r)
        else:
            p32 = _act32(r.float(), act)
            want = p32.to(dt)
        S.exact(p0.cpu()[..., :48], want, dt, v=r.float(), what=label + " post 0")
        if act == GELU and dt == torch.bfloat16:
            ref = p32[..., p2idx].double()
            worst, share = S.within(p1.cpu()[..., :24], ref, S.store_tol(ref, dt) + ref.abs() * 2.0 ** -15, v=r[..., p2idx].float(), what=label + " post 1")
            print(f"{label}: {name}; post 0 exact, post 1 (hi + lo of an emulated fp32 value) max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
        else:
            seen = _seen(want.float() if act == GELU else p32, dt)
            S.exact(p1.cpu()[..., :24], seen[..., p2idx].to(dt), dt, v=r[..., p2idx].float(), what=label + " post 1")
            print(f"{label}: {name}; post 0 and post 1 exact")


# ---- Part B: the fused multi-layer kernels ---------------------------------------------------------------------------------------------------
# Every layer carries 0 / 1 weights, so every stage is exact: a 16-bit value scaled by 0.05 once per LeakyReLU stage it passes (negative
# values; the products are rounded to the storage type where the launches store them, subnormal results included).  References take a
# `flush` switch -- every MFMA operand that is subnormal in the storage type read as zero -- and the result with it on is the accepted
# alternative of the identity route (exact(.., flushed=)).  The fused result must also equal the per-op launches bit for bit where the
# kernel's header promises that.
def _stage(t16, act, flush, idx=None, add=None):
    """one 0 / 1 layer on a 16-bit tensor: select channels `idx` (the MFMA operand: flushed if asked), + `add` (fp32, the residual),
    activation, one rounding -> (16-bit result, the fp32 result)"""
    a = (_flush(t16) if flush else t16).float()
    a = a if idx is None else a[..., idx]
    if add is not None:
        a = a + add
    y = _act32(a, act)
    return y.to(t16.dtype), y


def _bits_equal(a, b, what):
    a, b = a.cpu(), b.cpu()
    nd = int((a.contiguous().view(torch.int16) != b.contiguous().view(torch.int16)).sum())
    print(f"{what}: {nd} of {a.numel()} values differ between the fused kernel and the launches it replaces")
    assert nd == 0, what


@pytest.fixture(params=["2", "3"])
def strip_groups(request):
    """both strip widths of rlfb_chain_kernel (G = 2: 28 columns, G = 3: 44), through the research switch ESR_CHAIN_G"""
    import os
    old = os.environ.get("ESR_CHAIN_G")
    os.environ["ESR_CHAIN_G"] = request.param
    yield request.param
    if old is None:
        del os.environ["ESR_CHAIN_G"]
    else:
        os.environ["ESR_CHAIN_G"] = old


@pytest.mark.parametrize("store", STORES)
def test_rlfb_chain(store, strip_groups):
    """rlfb_chain_kernel: t1 = lrelu(x), t2 = lrelu(t1), u = lrelu(t2) + x, v = S . u, c1 = S' . v with identity 3x3s; and with a zero third
    3x3 (u = x, the residual alone)"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n, h, w, c, f = 2, 23, 37, 48, 16
    x = S.tile(_sweep(store), (n, h, w, c))
    xd = x.to(DEV)
    w5, w1 = S.selection(c, c), S.selection(f, c)
    zb = [torch.zeros(c)] * 3
    for last in ("identity", "zero"):
        ws = [S.identity_weight(c, c, 3), S.identity_weight(c, c, 3), S.identity_weight(c, c, 3) if last == "identity" else S.zero_weight(c, c, 3)]
        (v, c1), name = _traced(rf"rlfb_chain_kernel<{_bf(store)}, {strip_groups}>", lambda: ops.conv_chain(xd, ws, zb, w5, torch.zeros(c), w1, torch.zeros(f), cin=c))
        t1 = ops.conv2d(xd, ws[0], zb[0], act=LRELU, slope=SLOPE)
        t2 = ops.conv2d(t1, ws[1], zb[1], act=LRELU, slope=SLOPE)
        _, pv, pc1 = ops.conv2d(t2, ws[2], zb[2], act=LRELU, slope=SLOPE, res=xd, res_mode=RES_POST, post_weight=w5, post_bias=torch.zeros(c),
                                post2_weight=w1, post2_bias=torch.zeros(f), store_main=False)
        torch.cuda.synchronize()
        label = f"rlfb chain {store} G={strip_groups} third 3x3 {last}"
        refs = []
        for flush in (False, True):
            a1, _ = _stage(x, LRELU, flush)
            a2, _ = _stage(a1, LRELU, flush)
            conv3 = (_flush(a2) if flush else a2).float() if last == "identity" else torch.zeros(n, h, w, c)
            u32 = _act32(conv3, LRELU) + x.float()
            v32 = _seen(u32, dt)
            refs.append((v32.to(dt), _seen(v32, dt)[..., :f].to(dt)))
        (wv, wc1), (fv, fc1) = refs
        # u = lrelu(t2) + x is 2 x for a positive x: where that leaves the storage type's range in ANY channel of a pixel, the 1x1 multiplies the
        # Inf by the zero weights of every other output channel -- a non-finite intermediate, which the ABI excludes.  Those pixels are left out.
        live = torch.isfinite(wv.float()).all(dim=-1, keepdim=True)
        assert float(live.float().mean()) > 0.97
        for form, gv, gc in (("fused", v, c1), ("per-op", pv, pc1)):
            took = S.exact(torch.where(live, gv.cpu()[..., :c], wv), wv, dt, v=x.float(), flushed=fv, what=f"{label} {form} v")
            took += S.exact(torch.where(live, gc.cpu()[..., :f], wc1), wc1, dt, v=x[..., :f].float(), flushed=fc1, what=f"{label} {form} c1")
            _report(f"{label} {form}", name if form == "fused" else "three launches", took, int(S.is_subnormal(x).sum()))
        v, pv, c1, pc1 = (torch.where(live, t.cpu()[..., :k], torch.zeros((), dtype=dt)) for t, k in ((v, c), (pv, c), (c1, f), (pc1, f)))
        _bits_equal(v, pv, label + " v")
        _bits_equal(c1, pc1, label + " c1")


@pytest.mark.parametrize("store", STORES)
def test_hfab(store):
    """hfab_kernel: three LeakyReLU 3x3s over 16 channels (0 / 1 selections), then y = sigmoid(t3) * x; the gate's tolerance against fp64 on
    the exact t3, and the per-layer launches bit for bit"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    cin, cmid, pitch = 50, 16, 56
    n, h, w = S.shape_for(_sweep(store), cmid)
    x = S.tile(_perm(store), (n, h, w, pitch), cin)
    x[..., :cmid] = S.tile(_sweep(store), (n, h, w, cmid))
    xd = x.to(DEV)
    ws = [S.identity_weight(cmid, cin, 3), S.identity_weight(cmid, cmid, 3), S.identity_weight(cmid, cmid, 3), S.identity_weight(cin, cmid, 3)]
    bs = [torch.zeros(cmid)] * 3 + [torch.zeros(cin)]
    y, name = _traced(rf"hfab_kernel<{_bf(store)}, 4>", lambda: ops.conv_chain(xd, ws, bs, slope=SLOPE, res_mode=RES_GATE, cin=cin))
    t = xd
    for i in range(3):
        t = ops.conv2d(t, ws[i], bs[i], act=LRELU, slope=SLOPE, cin=cin if i == 0 else None)
    py = ops.conv2d(t, ws[3], bs[3], res=xd, res_mode=RES_GATE, out=torch.zeros(n, h, w, pitch, dtype=dt, device=DEV))
    torch.cuda.synchronize()
    a = x[..., :cmid]
    for _ in range(3):
        a, _ = _stage(a, LRELU, False)
    m = a[..., torch.arange(cin) % cmid]
    ref = S.sigmoid_f64(m) * x[..., :cin].double()
    tol = S.store_tol(ref, dt) + S.F32_MIN_NORMAL * x[..., :cin].double().abs()
    for form, g in (("fused", y), ("per-layer", py)):
        worst, share = S.within(g.cpu()[..., :cin], ref, tol, v=m.float(), what=f"hfab {store} {form}")
        print(f"hfab {store} {form} {n}x{h}x{w}: {name if form == 'fused' else 'four launches'}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    _bits_equal(y, py, f"hfab {store}")


def _tail_desc(L, store, shape, cin_phys, nf, dc, f, mid_act, r3, ds, v, c1, blobs, table):
    n, h, w = shape
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, nf, dc, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = d.compute = L.STORE[store]
    d.act, d.slope = L.ACT_NONE, SLOPE
    d.inp = L.View(ctypes.c_void_p(r3.data_ptr()), cin_phys, 0)
    d.out0 = L.View(ctypes.c_void_p(v.data_ptr()), v.shape[-1], 0)
    d.wpacked, d.tail_wpacked = blobs[0].data_ptr(), blobs[1].data_ptr()
    d.tail_cat = L.View(ctypes.c_void_p(ds.data_ptr()), 32, 0)
    d.tail_cat_c, d.tail_cout, d.tail_mid_act = 96, nf, mid_act
    d.tail_seg_stride16 = ds[0].numel() * 2 // 16
    d.post_wpacked, d.post_out = blobs[2].data_ptr(), L.View(ctypes.c_void_p(c1.data_ptr()), 16, 0)
    d.post_cout, d.post_act = f, L.ACT_NONE
    if table is not None:
        d.border_bias = table.data_ptr()
    assert L.lib().esr_conv_tail_supported(ctypes.byref(d)) == 1
    return d


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("form", ["rfdb", "esdb"])
def test_rfdb_tail(store, form):
    """rfdb_tail_kernel: r4 = act(c4(r3)) rounded, v = c5 . [d1 d2 d3 r4], c1 = conv1 . v.  RFDB form: 64 -> 32, LeakyReLU; ESDB form: 48 ->
    32 with a zero border table and the 16-bit GELU (against conv_s16_kernel's bits).  c4 is a selection of r3 (the sweep), c5 sends r4 to
    v's first 32 channels and d1 (the permuted sweep) to the others, conv1 selects v's first 16."""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, pack_post_s16, pack_tail_s16
    dt = S.DTYPES[store]
    esdb = form == "esdb"
    n, h, w = BIG16
    nf, cp, dc, f = (48, 48, 32, 16) if esdb else (64, 64, 32, 16)
    act = GELU if esdb else LRELU
    lut = _gelu_lut(store) if esdb else None
    r3 = S.tile(_sweep(store), (n, h, w, cp))
    ds = torch.stack([S.tile(_perm(store), (n, h, w, 32)), torch.ones(n, h, w, 32, dtype=dt), S.tile(_sweep(store), (n, h, w, 32))]).contiguous()
    w4 = S.identity_weight(dc, nf, 3)
    w5 = torch.zeros(nf, 4 * dc)
    o = torch.arange(nf)
    w5[o, torch.where(o < dc, 3 * dc + o, o - dc)] = 1.0
    wc = S.selection(f, nf)
    blobs = [pack_conv_s16(w4, torch.zeros(dc), store, cin_phys=cp).to(DEV), pack_tail_s16(w5, torch.zeros(nf), 3, dc, dc, store).to(DEV),
             pack_post_s16(wc, torch.zeros(f), store).to(DEV)]
    table = torch.zeros(16, 32, device=DEV) if esdb else None
    r3d, dsd = r3.to(DEV), ds.to(DEV)
    v = torch.full((n, h, w, nf), 7.0, dtype=dt, device=DEV)
    c1 = torch.full((n, h, w, 16), 7.0, dtype=dt, device=DEV)
    d = _tail_desc(L, store, (n, h, w), cp, nf, dc, f, act, r3d, dsd, v, c1, blobs, table)
    _, name = _traced(rf"rfdb_tail_kernel<{_bf(store)}, {'3, true' if esdb else '4, false'}>",
                      lambda: ops._launch(L.OP_CONV, d, torch.cuda.current_stream().cuda_stream, "tail"))
    refs = []
    for flush in (False, True):
        op = _flush if flush else (lambda t: t)                   # every MFMA operand: r3 for c4, r4 and d1 for c5 (v is summed from them in fp32)
        xin = op(r3)[..., :dc]
        r4 = S.from_bits(lut[S.to_bits(xin).long()], dt) if esdb else _stage(xin, LRELU, False)[0]
        want_v = torch.cat([op(r4), op(ds[0])[..., :nf - dc]], dim=-1)
        refs.append((want_v, want_v[..., :f]))
    (wv, wc1), (fv, fc1) = refs
    label = f"{form} tail {store} {n}x{h}x{w}"
    took = S.exact(v.cpu(), wv, dt, v=torch.cat([r3[..., :dc], ds[0][..., :nf - dc]], dim=-1).float(), flushed=fv, what=label + " v")
    took += S.exact(c1.cpu(), wc1, dt, v=r3[..., :f].float(), flushed=fc1, what=label + " c1")
    _report(label, name, took, int(S.is_subnormal(r3[..., :dc]).sum()) + int(S.is_subnormal(r3[..., :f]).sum()))
    # the launches it replaces: c4, then the 1x1 over the planar concat with conv1 in its epilogue
    kw = dict(border=table) if esdb else {}
    r4p = ops.conv2d(r3d, w4, torch.zeros(dc), act=act, slope=SLOPE, cin=nf, packed=blobs[0], **kw)
    cat = torch.cat([dsd, r4p[None]], dim=0).contiguous()
    pv = ops.conv2d(cat, w5, torch.zeros(nf))
    pc1 = ops.conv2d(pv, wc, torch.zeros(f))
    torch.cuda.synchronize()
    S.exact(pv.cpu()[..., :nf], wv, dt, flushed=fv, what=label + " per-op v")
    S.exact(pc1.cpu()[..., :f], wc1, dt, flushed=fc1, what=label + " per-op c1")
    _bits_equal(v, pv[..., :nf], label + " v")
    _bits_equal(c1[..., :f], pc1[..., :f], label + " c1")


@pytest.mark.parametrize("store", STORES)
def test_refine_cascade(store):
    """refine_cascade_kernel: r2 = lrelu(conv(d2) + d2), d3 = lrelu(S . r2), r3 = lrelu(conv(d3) + d3), r4 = lrelu(conv(r3) + r3) with zero
    3x3s -- every stage is its residual through LeakyReLU, a negative sweep value scaled by 0.05 four times -- and a 0 / 1 selection for
    the 1x1 (identity 3x3s would double the value at every stage: Inf in f16 after the first, and 0 x Inf in its neighbours' taps)"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    n, h, w = S.shape_for(_sweep(store), 16)
    d2 = S.tile(_perm(store), (n, h, w, 32))
    d2[..., :16] = S.tile(_sweep(store), (n, h, w, 16))
    xd = d2.to(DEV)
    z32, z16, sel = S.zero_weight(32, 32, 3), S.zero_weight(16, 16, 3), S.identity_weight(16, 32, 1)
    wts = (z32, torch.zeros(32), sel, torch.zeros(16), z16, torch.zeros(16), z16, torch.zeros(16))
    (d3, r4), name = _traced(rf"refine_cascade_kernel<{_bf(store)}>", lambda: ops.refine_cascade(xd, *wts, slope=SLOPE))
    kw = dict(act=LRELU, slope=SLOPE)
    pr2 = ops.conv2d(xd, wts[0], wts[1], res=xd, res_mode=RES_PRE, **kw)
    pd3 = ops.conv2d(pr2, wts[2], wts[3], **kw)
    pr3 = ops.conv2d(pd3, wts[4], wts[5], res=pd3, res_mode=RES_PRE, **kw)
    pr4 = ops.conv2d(pr3, wts[6], wts[7], res=pr3, res_mode=RES_PRE, **kw)
    torch.cuda.synchronize()
    refs = []
    for flush in (False, True):
        r2, _ = _stage(d2, LRELU, False)
        a3, _ = _stage(r2, LRELU, flush, idx=torch.arange(16))
        b3, _ = _stage(a3, LRELU, False)
        b4, _ = _stage(b3, LRELU, False)
        refs.append((a3, b4))
    (wd3, wr4), (fd3, fr4) = refs
    label = f"refine cascade {store} {n}x{h}x{w}"
    for form, g3, g4 in (("fused", d3, r4), ("per-op", pd3, pr4)):
        took = S.exact(g3.cpu()[..., :16], wd3, dt, v=d2[..., :16].float(), flushed=fd3, what=f"{label} {form} d3")
        took += S.exact(g4.cpu()[..., :16], wr4, dt, v=d2[..., :16].float(), flushed=fr4, what=f"{label} {form} r4")
        _report(f"{label} {form}", name if form == "fused" else "four launches", took, int(S.is_subnormal(d2[..., :16]).sum()))
    _bits_equal(d3, pd3, label + " d3")
    _bits_equal(r4, pr4, label + " r4")


@pytest.mark.parametrize("store", STORES)
def test_distill_step(store):
    """distill_step_kernel: d = relu(S . x), y = relu(c_r(x) + c_b(d) (+ x)) with ONE non-zero term in the sum (the per-op form rounds
    c_b(d) (+ x) to the storage type, the fused one does not: with one term both are exact)"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    c = 32
    n, h, w = S.shape_for(_sweep(store), c)
    x = S.tile(_sweep(store), (n, h, w, c))
    xd = x.to(DEV)
    ident, zero, zb = S.identity_weight(c, c, 3), S.zero_weight(c, c, 3), torch.zeros(c)
    for term, (wr, wb, res) in {"c_r": (ident, zero, False), "c_b": (zero, ident, False), "x": (zero, zero, True)}.items():
        (dd, y), name = _traced(rf"distill_step_kernel<{_bf(store)}, 2, {'true' if res else 'false'}>",
                                lambda: ops.distill_step(xd, S.identity_weight(c, c, 1), zb, wr, zb, wb, zb, res=res))
        pd = ops.conv2d(xd, S.identity_weight(c, c, 1), zb, act=RELU)
        pt = ops.conv2d(pd, wb, zb, res=xd if res else None, res_mode=RES_PRE if res else RES_NONE)
        py = ops.conv2d(xd, wr, zb, act=RELU, res=pt, res_mode=RES_PRE)
        torch.cuda.synchronize()
        refs = []
        for flush in (False, True):
            d16, _ = _stage(x, RELU, flush)
            y16 = {"c_r": _stage(x, RELU, flush)[0], "c_b": _stage(d16, RELU, flush)[0], "x": _stage(x, RELU, False)[0]}[term]
            refs.append((d16, y16))
        (wd, wy), (fd, fy) = refs
        label = f"distill step {store} term {term} {n}x{h}x{w}"
        for form, gd, gy in (("fused", dd, y), ("per-op", pd, py)):
            took = S.exact(gd.cpu()[..., :c], wd, dt, v=x.float(), flushed=fd, what=f"{label} {form} d")
            took += S.exact(gy.cpu()[..., :c], wy, dt, v=x.float(), flushed=fy, what=f"{label} {form} y")
            _report(f"{label} {form}", name if form == "fused" else "three launches", took, 2 * int(S.is_subnormal(x).sum()))
        _bits_equal(dd, pd, label + " d")
        _bits_equal(y, py, label + " y")


@pytest.mark.parametrize("store", STORES)
def test_resblock_head(store):
    """resblock_head_kernel: xs = x + g (g = 0: a second operand would overflow f16 into the next 3x3's taps), t = relu(conv1(xs)), u =
    conv2(t), c1 = S . u with identity 3x3s; with and without g"""
    from ntire2022_esr_amd import ops
    dt = S.DTYPES[store]
    c, f = 32, 16
    n, h, w = S.shape_for(_sweep(store), c)
    x = S.tile(_sweep(store), (n, h, w, c))
    xd = x.to(DEV)
    ident, zb, wc = S.identity_weight(c, c, 3), torch.zeros(c), S.identity_weight(f, c, 1)
    for with_g in (False, True):
        g = torch.zeros(n, h, w, c, dtype=dt, device=DEV) if with_g else None
        (xs, u, c1), name = _traced(rf"resblock_head_kernel<{_bf(store)}, {'true' if with_g else 'false'}>",
                                    lambda: ops.resblock_head(xd, ident, zb, ident, zb, wc, torch.zeros(f), g=g))
        px = xd
        if with_g:
            px = ops.conv2d(g, torch.eye(c)[:, :, None, None], zb, res=xd, res_mode=RES_PRE)
        pt = ops.conv2d(px, ident, zb, act=RELU)
        pu = ops.conv2d(pt, ident, zb)
        pc = ops.conv2d(pu, wc, torch.zeros(f), out=torch.zeros_like(c1))
        torch.cuda.synchronize()
        refs = []
        for flush in (False, True):
            t16, _ = _stage(x, RELU, flush)
            u16, _ = _stage(t16, NONE, flush)
            refs.append((u16, _stage(u16, NONE, flush, idx=torch.arange(f))[0]))
        (wu, wc1), (fu, fc1) = refs
        label = f"resblock head {store} g={with_g} {n}x{h}x{w}"
        if with_g:
            S.exact(xs.cpu()[..., :c], x, dt, v=x.float(), what=label + " xs")
            _bits_equal(xs, px, label + " xs")
        for form, gu, gc in (("fused", u, c1), ("per-op", pu, pc)):
            took = S.exact(gu.cpu()[..., :c], wu, dt, v=x.float(), flushed=fu, what=f"{label} {form} u")
            took += S.exact(gc.cpu()[..., :f], wc1, dt, v=x[..., :f].float(), flushed=fc1, what=f"{label} {form} c1")
            _report(f"{label} {form}", name if form == "fused" else "the launches", took, int(S.is_subnormal(x).sum()))
        _bits_equal(u, pu, label + " u")
        _bits_equal(c1, pc, label + " c1")


@pytest.mark.parametrize("store", STORES)
def test_cx_block(store):
    """cx_block_kernel: t = dw7(v) (centre tap 1), hidden = lrelu(S . t), out = S' . hidden + v; with S' a selection (out = lrelu(v) + v, one
    fp32 add, one rounding) and S' = 0 (out = v).  The fused and the per-op form are each compared with the CPU expression: with 0 / 1
    weights the fused kernel's single weight rounding changes nothing."""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.rfdnext import _hidden_slices
    dt = S.DTYPES[store]
    c, m = 48, 144
    n, h, w = 2, 23, 37
    v = S.tile(_sweep(store), (n, h, w, c))
    vd = v.to(DEV)
    w0, w1 = S.dw_identity(c, 7), S.selection(m, c)
    for second in ("selection", "zero"):
        w2 = S.selection(c, m) if second == "selection" else torch.zeros(c, m)
        args = (w0, torch.zeros(c), w1, torch.zeros(m), w2, torch.zeros(c))
        y, name = _traced(rf"cx_block_kernel<{_bf(store)}>", lambda: ops.cx_block(vd, *args, slope=SLOPE))
        t = ops.dwconv7x7(vd, w0, torch.zeros(c))
        hid = torch.zeros(n, h, w, _up(m, 16), dtype=dt, device=DEV)
        for a, wd in _hidden_slices(m, store):
            ops.conv2d(t, w1[a:a + wd], torch.zeros(wd), act=LRELU, slope=SLOPE, cin=c, out=hid, out_coff=a)
        py = ops.conv2d(hid, w2, torch.zeros(c), res=vd, res_mode=RES_PRE, cin=m)
        torch.cuda.synchronize()
        refs = []
        for flush in (False, True):
            hid16, _ = _stage(v, LRELU, flush)
            conv = (_flush(hid16) if flush else hid16).float() if second == "selection" else torch.zeros(n, h, w, c)
            refs.append(_expr(conv, v.float(), NONE, RES_PRE, dt)[0])
        want, alt = refs
        label = f"cx block {store} second 1x1 {second} {n}x{h}x{w}"
        for form, g in (("fused", y), ("per-op", py)):
            took = S.exact(g.cpu()[..., :c], want, dt, v=v.float(), flushed=alt, what=f"{label} {form}")
            _report(f"{label} {form}", name if form == "fused" else "dwconv7x7 + the 1x1 launches", took, int(S.is_subnormal(v).sum()))


# ---- Part C: fp32 storage ------------------------------------------------------------------------------------------------------------------------
def test_fp32_storage():
    """every finite bf16 pattern widened to fp32 through conv_f32_kernel (GELU by erff on the residual route; the sigmoid gate on the identity
    route), wino_f32_kernel (GELU), esa_apply_kernel (its inline sigmoid) and ca_apply_nchw_kernel (ca_gate's sigmoid) against fp64:
    4 * 2^-24 |ref|, + 2^-21 |v| for GELU (1 + erff(v / sqrt 2) cancels for v < 0 and erff is good to a few ulp of 1), + the smallest fp32
    normal x |r| for the gates"""
    from ntire2022_esr_amd import ops
    sw = _sweep("bf16").float()
    pm = _perm("bf16").float()
    n, h, w, c = 2, 23, 37, 64
    x, r = S.tile(sw, (n, h, w, c)), S.tile(pm, (n, h, w, c))
    xd, rd = x.to(DEV), r.to(DEV)
    gref = S.gelu_f64(x)
    gtol = S.f32_tol(gref) + x.double().abs() * 2.0 ** -21
    y, name = _traced(r"conv_f32_kernel<", lambda: ops.conv2d(rd, S.zero_weight(c, c, 3), torch.zeros(c), act=GELU, res=xd, res_mode=RES_PRE))
    worst, share = S.within(y.cpu(), gref, gtol, v=x, what="conv_f32 gelu")
    print(f"fp32 conv_f32_kernel GELU: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    y, name = _traced(r"wino_f32_kernel<", lambda: ops.conv2d(torch.zeros_like(xd), S.zero_weight(c, c, 3), torch.zeros(c), act=GELU, res=xd, res_mode=RES_PRE,
                                                              wino=True))
    worst, share = S.within(y.cpu(), gref, gtol, v=x, what="wino_f32 gelu")
    print(f"fp32 wino_f32_kernel GELU: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    for rname, rr in (("1", torch.ones_like(x)), ("sweep", r)):
        ref = S.sigmoid_f64(x) * rr.double()
        tol = S.f32_tol(ref) + S.F32_MIN_NORMAL * rr.double().abs()
        y, name = _traced(r"conv_f32_kernel<", lambda: ops.conv2d(xd, S.identity_weight(c, c, 3), torch.zeros(c), res=rr.to(DEV), res_mode=RES_GATE))
        worst, share = S.within(y.cpu(), ref, tol, v=x, what=f"conv_f32 gate r={rname}")
        print(f"fp32 conv_f32_kernel gate r={rname}: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    # esa_apply_kernel: m[ch] = c1[ch mod 16]
    f = 16
    n2, h2, w2 = S.shape_for(sw, f)
    c1 = S.tile(sw, (n2, h2, w2, f))
    m = c1[..., torch.arange(c) % f]
    for xname, xx in (("1", torch.ones(n2, h2, w2, c)), ("sweep", S.tile(pm, (n2, h2, w2, c)))):
        y, name = _traced(r"esa_apply_kernel<0>", lambda: ops.esa_apply(xx.to(DEV), c1.to(DEV), torch.zeros(n2, 2, 2, 16, device=DEV), torch.eye(f), torch.zeros(f),
                                                                       S.selection(c, f), torch.zeros(c)))
        ref = S.sigmoid_f64(m) * xx.double()
        worst, share = S.within(y.cpu(), ref, S.f32_tol(ref) + S.F32_MIN_NORMAL * xx.double().abs(), v=m, what=f"esa_apply f32 x={xname}")
        print(f"fp32 esa_apply_kernel x={xname}: {name}; max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
    # ca_apply_nchw_kernel (and ca_apply_nhwc_kernel<0>): the gate is sigmoid(b2[ch]); no op kind, so no symbol to assert
    b2 = torch.tensor(GATE_BIASES * 2, dtype=torch.float32)
    xn = x.permute(0, 3, 1, 2).contiguous()
    for nchw, xin in ((True, xn), (False, x)):
        y = ops.channel_attention(xin.to(DEV), torch.zeros(4, c), torch.zeros(4), torch.zeros(c, 4), b2, nchw=nchw).cpu()
        torch.cuda.synchronize()
        gate = S.sigmoid_f64(b2)
        ref = xin.double() * (gate[None, :, None, None] if nchw else gate[None, None, None, :])
        worst, share = S.within(y, ref, S.f32_tol(ref) + S.F32_MIN_NORMAL * xin.double().abs(), v=xin, what=f"channel attention f32 nchw={nchw}")
        print(f"fp32 channel attention nchw={nchw}: max|got - ref| = {worst:.3e} ({share:.3f} of the bound)")
