"""-m gpu: every kernel stays inside its declared tensor views (DESIGN.md "Bounds"; the arena: tests/_guarded.py).

The property, the same for every launcher: the case runs twice on the same guarded arena layout -- once with NaN, once with seeded finite
noise in the guards of its inputs, and with two different finite fills in the foreign channels of its input buffers -- and
  (a) no byte outside the declared output views changes (guards, inputs, unused channel slices, outputs declared as not stored);
  (b) both results are finite and bit-identical: the result is a function of the declared views only (two fills because fmaxf(NaN, 0) = 0:
      a ReLU would swallow a NaN that leaked in);
  (c) the result on ordinary freshly allocated tensors is bit-identical too: the arena changes nothing.
Values against fp64 stay with the other test files.  esr_channel_attention_f32 accumulates with fp64 atomics, so (b) / (c) are replaced by
the fp64 restatement and the tolerances of tests/test_gpu_ca.py there.

Fills.  NaN only OUTSIDE a tensor.  Inside an input buffer the channels that are not part of the read slice hold finite values: by the
tight-pitch contract (include/esr_hip.h, esr_storage) the 16-bit K loop reads the 16-channel chunk that holds the slice's end -- up to 8
channels of the next pixel or of a neighbouring slice -- against zero weight rows.  The pad channels inside the read slice are zero, as
every producer leaves them.  In every batch the last image is the one that abuts the guard."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

from _guarded import SENTINEL, Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FILLS = ("nan", "noise")


def _up(v, m):
    return (v + m - 1) // m * m


def _gen(*seed):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(s) for i, s in enumerate(seed)) % (2 ** 31))


def _widen(core, pitch, coff, variant, seed=0):
    """core [..., c] (its pad channels zero) as channels [coff, coff + c) of a [..., pitch] buffer whose other channels hold finite noise
    that differs between the two variants"""
    c = core.shape[-1]
    if pitch == c and coff == 0:
        return core.contiguous()
    t = (torch.randn(*core.shape[:-1], pitch, generator=_gen(seed, variant, 11)) * 2).to(core.dtype)
    t[..., coff:coff + c] = core
    return t.contiguous()


def _core(n, h, w, c, cpad, dt, g, scale=1.0):
    return F.pad(torch.randn(n, h, w, c, generator=g) * scale, (0, cpad - c)).to(dt)


class Case:
    """inputs: name -> CPU tensor (the whole buffer); outputs: name -> (shape, dtype, writable); launch(t): runs the op on the tensors t[name];
    kernel: regex the device symbol of the launch must match (None: the entry point has one kernel); a tuple: one regex per launch, in order;
    rows: name -> elements of one image row, for tensors whose last two dims are not (w, pitch) (Arena.add_input)"""

    def __init__(self, inputs, outputs, launch, kernel=None, rows=None):
        self.inputs, self.outputs, self.launch, self.kernel, self.rows = inputs, outputs, launch, kernel, rows or {}


def _run_guarded(make):
    from ntire2022_esr_amd import ops
    results = []
    for variant, fill in enumerate(FILLS):
        case = make(variant)
        a = Arena(DEV, fill=fill, seed=variant)
        for name, data in case.inputs.items():
            a.add_input(name, data, case.rows.get(name))
        for name, (shape, dtype, writable) in case.outputs.items():
            a.add_output(name, shape, dtype, writable, case.rows.get(name))
        a.build()
        with ops.kernel_trace() as names:
            case.launch(a.tensors)
        torch.cuda.synchronize()
        if case.kernel is not None:
            want = case.kernel if isinstance(case.kernel, tuple) else (case.kernel,) * max(len(names), 1)
            assert len(names) == len(want) and all(re.match(p, k) for p, k in zip(want, names)), (names, case.kernel)
        a.check_untouched()                                                                        # (a)
        res = {name: a.written(name) for name, (_, _, wr) in case.outputs.items() if wr is not None}
        for name, r in res.items():
            assert r.dtype == torch.uint8 or r.dtype == torch.int64 or bool(torch.isfinite(r.double()).all()), (name, fill)
        results.append(res)
    return results, names


def _run_fresh(make):
    case = make(0)
    t = {name: data.to(DEV) for name, data in case.inputs.items()}
    for name, (shape, dtype, _) in case.outputs.items():
        t[name] = torch.full(shape, SENTINEL, dtype=torch.uint8, device=DEV).repeat_interleave(torch.empty(0, dtype=dtype).element_size(), -1) \
            .view(dtype).view(shape)          # the arena's bit pattern, so that elements of a view a kernel legitimately leaves alone compare equal
    case.launch(t)
    torch.cuda.synchronize()
    return {name: (t[name] if wr == "all" else t[name].narrow(*wr)) for name, (_, _, wr) in case.outputs.items() if wr is not None}


def _property(make):
    (r0, r1), names = _run_guarded(make)
    for name in r0:
        assert torch.equal(r0[name], r1[name]), (name, "differs between the NaN and the noise arena", int((r0[name] != r1[name]).sum()))     # (b)
    fresh = _run_fresh(make)
    for name in r0:
        assert torch.equal(r0[name], fresh[name]), (name, "differs from the freshly allocated run")                                          # (c)
    return names


# shape groups: partial tiles in both directions (n = 2), one less / one more than a tile multiple, degenerate strips
SMALL = [(2, 23, 37), (1, 31, 33), (1, 90, 1), (2, 5, 3)]
# the persistent 16-bit kernels start at 256 tiles of 16 x 16: the same groups at a batch that reaches them
PERSIST = [(2, 175, 209), (48, 1, 90), (9, 150, 97)]


# ---- esr_conv2d_f32: one builder for the direct fp32 kernel, the Winograd kernels and the 16-bit family ------------------------------
def _conv(store, n, h, w, cin, cout, k, *, in_pitch=None, in_coff=0, out_pitch=None, out_coff=0, act=1, res=None, res_mode=0, split=0,
          out1_pitch=None, out1_coff=0, blocked_out1=False, post=0, post_act=1, post2=0, store_main=True, border=False, wino=False,
          shuffle=False, nchw=False, nchw_store=None, cin_map=None, kernel=None, cin_phys=None):
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv, pack_conv_s16
    st = nchw_store or store
    dt, gran = DT[st], (4 if st == "f32" else 8)
    g = _gen(n, h, w, cin, cout, k)
    wt = torch.randn(cout, cin if cin_map is None else max(cin_map) + 1, k, k, generator=g) * (0.1 if k == 3 else 0.2)
    b = torch.randn(cout, generator=g)
    table = None
    if border:
        table = torch.randn(16, _up(cout, 16), generator=g) * 0.2
        table[0] = 0
    pw = (torch.randn(post, cout, generator=g) * 0.2, torch.randn(post, generator=g)) if post else None
    pw2 = (torch.randn(post2, post, generator=g) * 0.2, torch.randn(post2, generator=g)) if post2 else None
    cin_r = _up(cin, gran)
    in_pitch = in_pitch or cin_r
    xcore = torch.rand(n, cin, h, w, generator=g) * 255 if nchw else _core(n, h, w, cin, cin_r, DT[store], g)
    cs = min(split, cout) if split else cout
    cs_r = _up(cs, gran)
    rcore = _core(n, h, w, cout, _up(cout, gran), dt, g) if res == "hbm" else None
    packed = None
    if cin_phys is not None and cin_map is None:
        packed = pack_conv_s16(wt, b, store, cin_phys=cin_phys)

    def make(variant):
        ins = {"x": xcore if nchw else _widen(xcore, in_pitch, in_coff, variant, 1)}
        if rcore is not None:
            ins["r"] = _widen(rcore, rcore.shape[-1] + gran, gran, variant, 2)
        outs = {}
        if shuffle:
            outs["y"] = ((n, cout // 16, 4 * h, 4 * w), torch.float32, "all")
        elif store_main:
            outs["y"] = ((n, h, w, out_pitch or cs_r), dt, (-1, out_coff, cs_r))
        if split and split < cout:
            c1r = _up(cout - split, gran)
            if blocked_out1:
                outs["y1"] = ((n, (out1_pitch or c1r) // 8, h, w, 8), dt, (1, out1_coff // 8, c1r // 8))
            else:
                outs["y1"] = ((n, h, w, out1_pitch or c1r), dt, (-1, out1_coff, c1r))
        if post:
            outs["p"] = ((n, h, w, _up(post, gran) + gran), dt, (-1, 0, _up(post, gran)))
        if post2:
            outs["p2"] = ((n, h, w, _up(post2, 8) + 8), dt, (-1, 0, _up(post2, 8)))

        def launch(t):
            kw = dict(act=act, cin=None if nchw else cin, in_coff=in_coff, out=t.get("y"), out_coff=out_coff, split=split, out1=t.get("y1"),
                      out1_coff=out1_coff, blocked_out1=blocked_out1, store_main=store_main, wino=wino, shuffle_out=shuffle, in_nchw=nchw,
                      store=nchw_store, cin_map=cin_map, border=None if table is None else table.to(DEV),
                      packed=None if packed is None else packed.to(DEV))
            if res == "in":
                kw.update(res=t["x"], res_coff=in_coff, res_mode=res_mode)
            elif res == "hbm":
                kw.update(res=t["r"], res_coff=gran, res_mode=res_mode)
            if post:
                kw.update(post_weight=pw[0], post_bias=pw[1], post_act=post_act, post_out=t["p"])
            if post2:
                kw.update(post2_weight=pw2[0], post2_bias=pw2[1], post2_out=t["p2"])
            ops.conv2d(t["x"], wt, b, **kw)
        return Case(ins, outs, launch, kernel, {"y1": w * (out1_pitch or _up(cout - split, gran))} if blocked_out1 else None)
    return make


F32_4W, F32_8W = r"conv_f32_kernel<\d, [13], false, 4,", r"conv_f32_kernel<\d, 3, false, 8,"


@pytest.mark.parametrize("n,h,w", SMALL)
@pytest.mark.parametrize("k,cin,cout", [(3, 48, 64), (1, 64, 48), (3, 64, 16)])
def test_f32_direct_conv_slices(n, h, w, k, cin, cout):
    """conv_f32_kernel, 4-wave tiles: reads a slice of a wider buffer, stores into a slice of a wider buffer, residual from HBM"""
    _property(_conv("f32", n, h, w, cin, cout, k, in_pitch=cin + 16, in_coff=8, out_pitch=cout + 16, out_coff=8, res="hbm", res_mode=1, kernel=F32_4W))


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 5, 3), (9, 97, 130)])
def test_f32_direct_conv_split_store(n, h, w):
    """the split store to out / out1 (IMDBlock: 16 -> concat slice, 48 -> next conv), NHWC and channel-blocked out1; n = 9 at 97 x 130 is the
    8-wave shape (16 x 32 tiles)"""
    kern = F32_8W if n == 9 else F32_4W
    _property(_conv("f32", n, h, w, 48, 64, 3, in_pitch=64, in_coff=16, split=16, out_pitch=64, out_coff=32, out1_pitch=56, out1_coff=4, kernel=kern))
    _property(_conv("f32", n, h, w, 48, 64, 3, split=16, out_pitch=48, out_coff=32, out1_pitch=56, out1_coff=8, blocked_out1=True, kernel=kern))


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 33, 31), (1, 1, 90), (9, 150, 97)])
def test_f32_direct_conv_8wave_head_tail_and_cin_map(n, h, w):
    """8-wave tiles from 256 tiles of 16 x 32, the NCHW head, the pixel-shuffle tail, a padded concat map (cin_map)"""
    _property(_conv("f32", n, h, w, 64, 64, 3, res="in", res_mode=1, kernel=F32_8W if n == 9 else F32_4W))
    _property(_conv("f32", n, h, w, 3, 64, 3, nchw=True, act=0, kernel=r"conv_f32_kernel<4, 3, true, 4,"))
    _property(_conv("f32", n, h, w, 64, 48, 3, shuffle=True, act=0, in_pitch=72, in_coff=4, kernel=F32_8W if n == 9 else F32_4W))
    cmap = list(range(10)) + [-1, -1] + list(range(10, 20)) + [-1, -1]          # 24 physical slots carrying 20 logical channels
    _property(_conv("f32", n, h, w, 24, 32, 1, cin_map=cmap, act=0, kernel=F32_4W))


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 5, 3), (9, 150, 171)])
@pytest.mark.parametrize("res_mode,cat_c", [(1, 48), (2, 32)])
def test_f32_fused_1x1_tail(n, h, w, res_mode, cat_c):
    """esr_conv_desc.tail_* (fp32): cat_c = 48 with a pre-activation residual is imdb_tail_kernel, the other conv_f32_kernel's TAIL variant;
    tail_cat is a slice of a wider buffer"""
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, cat_c)
    w3, b3 = torch.randn(16, 48, 3, 3, generator=g) * 0.1, torch.randn(16, generator=g)
    w1, b1 = torch.randn(64, cat_c + 16, 1, 1, generator=g) * 0.1, torch.randn(64, generator=g)
    x, cat, r = (_core(n, h, w, c, c, torch.float32, g) for c in (48, cat_c, 64))

    def make(variant):
        ins = {"x": _widen(x, 56, 8, variant, 1), "cat": _widen(cat, 64, 8, variant, 2), "r": _widen(r, 72, 4, variant, 3)}
        outs = {"y": ((n, h, w, 72), torch.float32, (-1, 4, 64))}

        def launch(t):
            ops.conv2d(t["x"], w3, b3, in_coff=8, cin=48, act=1 if res_mode == 2 else 0, res=t["r"], res_coff=4, res_mode=res_mode, out=t["y"],
                       out_coff=4, tail_weight=w1, tail_bias=b1, tail_cat=t["cat"], tail_cat_coff=8, tail_mid_act=1)
        return Case(ins, outs, launch, r"imdb_tail_kernel<true>" if cat_c == 48 else r"conv_f32_kernel<1, 3, false, 4, 4,")
    _property(make)


WINO = r"wino_f32_kernel<"


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 33, 31), (2, 5, 3), (4, 129, 127)])
def test_f32_winograd(n, h, w):
    """wino_f32_kernel, F(2x2, 3x3): 64 and 48 input channels, NHWC and channel-blocked input, with its split and blocked stores.  Every shape
    here has fewer than 4096 strips of 4 x 16, so none reaches wino8_f32_kernel (the next test does)"""
    from ntire2022_esr_amd import _lib as L
    d = L.ConvDesc()
    d.ksize, d.in_layout, d.out_layout, d.cin, d.cout = 3, L.NHWC, L.NHWC, 64, 64
    d.inp = L.View(None, 64, 0)
    assert L.lib().esr_wino_supported(ctypes.byref(d)) == 1
    _property(_conv("f32", n, h, w, 64, 64, 3, wino=True, in_pitch=72, in_coff=8, out_pitch=72, out_coff=4, res="hbm", res_mode=1,
                    kernel=WINO))
    _property(_conv("f32", n, h, w, 48, 64, 3, wino=True, split=16, out_pitch=64, out_coff=32, out1_pitch=48, kernel=WINO))
    _property(_conv("f32", n, h, w, 48, 64, 3, wino=True, split=16, out_pitch=24, out_coff=4, out1_pitch=56, out1_coff=8, blocked_out1=True,
                    kernel=WINO))
    _wino_blocked_in(n, h, w, WINO)


def _wino_blocked_in(n, h, w, kernel):
    """a channel-blocked INPUT [N, C/8, H, W, 8] (planes 1 .. 6 of 8 are read) with a split store into an NHWC slice and a blocked out1"""
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, 8)
    core = torch.randn(n, 6, h, w, 8, generator=g)
    wt, b = torch.randn(64, 48, 3, 3, generator=g) * 0.1, torch.randn(64, generator=g)

    def make(variant):
        xb = torch.randn(n, 8, h, w, 8, generator=_gen(variant, 5)) * 2
        xb[:, 1:7] = core
        outs = {"y": ((n, h, w, 24), torch.float32, (-1, 4, 16)), "y1": ((n, 7, h, w, 8), torch.float32, (1, 1, 6))}
        return Case({"x": xb}, outs, lambda t: ops.conv2d(t["x"], wt, b, act=1, blocked_in=True, in_coff=8, cin=48, split=16, out=t["y"], out_coff=4,
                                                          out1=t["y1"], out1_coff=8, blocked_out1=True, wino=True), kernel,
                    {"x": w * 64, "y1": w * 56})
    _property(make)


def test_f32_wino8_is_the_kernel_at_its_strip_count():
    """wino8_f32_kernel takes a 48 -> 64 layer from 4096 strips of 4 x 16 pixels (5 x 16 x 63 here, ragged in both directions): NHWC and
    blocked input, split store with an NHWC and a blocked out1"""
    n, h, w = 5, 250, 243
    _property(_conv("f32", n, h, w, 48, 64, 3, wino=True, in_pitch=56, in_coff=8, split=16, out_pitch=64, out_coff=32, out1_pitch=56, out1_coff=8,
                    kernel=r"wino8_f32_kernel<1, 0, 6>"))
    _wino_blocked_in(n, h, w, r"wino8_f32_kernel<1, 1, 6>")


# conv_s16_kernel<NT, KS, NW, BF16, GRES, PNT1, PNT2, HILO>: NW = 8 on 16 x 32 tiles, NW = 4 (two blocks per CU) on 16 x 16 tiles
S16 = r"conv_s16_kernel<\d, [13], 8, (true|false), (true|false), \d, \d, false>"
S16_4W = r"conv_s16_kernel<3, 3, 4, (true|false), false, 0, 0, false>"
HILO = r"conv_s16_kernel<[34], 3, 8, true, (true|false), 0, 0, true>"
HILO_4W = r"conv_s16_kernel<3, 3, 4, true, false, 0, 0, true>"
HILO_POST = r"conv_s16_kernel<4, 3, 8, true, false, 2, 0, true>"
# the 4-wave shape starts at 512 tiles of 16 x 16: partial tiles in both directions, a batch of strips, one more / one less than a multiple
FOUR_WAVE = [(9, 150, 97), (86, 1, 90), (4, 177, 191)]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", SMALL)
def test_s16_general_kernel(store, n, h, w):
    """conv_s16_kernel: k = 1 and 3; TIGHT pitch (cin 40 and 50: the tensor's last pixel lies directly in front of the guard, its last K chunk
    reaches 8 channels into it and must be clipped by the buffer resource); slices of wider buffers; residual from HBM"""
    for cin, cout, k in ((40, 64, 3), (50, 50, 3), (50, 25, 1)):
        _property(_conv(store, n, h, w, cin, cout, k, kernel=S16))                                      # pitch = round_up(cin, 8): tight
    _property(_conv(store, n, h, w, 50, 50, 3, res="in", res_mode=1, kernel=S16))
    _property(_conv(store, n, h, w, 46, 46, 3, in_pitch=64, in_coff=8, out_pitch=64, out_coff=8, res="hbm", res_mode=2, kernel=S16))
    _property(_conv(store, n, h, w, 48, 48, 1, in_pitch=64, in_coff=16, out_pitch=56, out_coff=8, res="hbm", res_mode=1, act=3, kernel=S16))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (1, 1, 90), (2, 5, 3)])
def test_s16_split_shuffle_head_and_post_chain(store, n, h, w):
    """conv_s16_kernel: split store, pixel-shuffle tail (fp32 NCHW out), the NCHW head of a 16-bit network, the post / post2 chain with
    store_main=False, RFDB's stored result + one post 1x1, the border table"""
    _property(_conv(store, n, h, w, 64, 64, 3, in_pitch=128, in_coff=64, split=16, out_pitch=64, out_coff=32, out1_pitch=56, out1_coff=8, kernel=S16))
    _property(_conv(store, n, h, w, 64, 48, 3, shuffle=True, act=0, kernel=S16))
    _property(_conv("f32", n, h, w, 3, 46, 3, nchw=True, nchw_store=store, act=0, kernel=r"conv_f32_kernel<3, 3, true, 4,"))      # esr_conv2d_f32's own head
    _property(_conv(store, n, h, w, 48, 46, 3, res="hbm", res_mode=2, post=46, post_act=0, post2=16, store_main=False, kernel=S16))
    _property(_conv(store, n, h, w, 50, 50, 3, in_pitch=64, res="in", res_mode=1, post=25, kernel=S16))
    _property(_conv(store, n, h, w, 48, 48, 3, res="in", res_mode=1, act=3, border=True, kernel=S16))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 33, 31), (1, 90, 1)])
def test_s16_segmented_input(store, n, h, w):
    """esr_conv_desc.in_seg_*: the 1x1 over a concat kept as four dense tensors one stride apart"""
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, 4)
    xs = (torch.randn(4, n, h, w, 32, generator=g)).to(DT[store])
    wt, b = torch.randn(48, 128, generator=g) * 0.1, torch.randn(48, generator=g)

    def make(variant):
        def launch(t):
            ops.conv2d(t["x"], wt, b, act=1, out=t["y"], out_coff=8)
        return Case({"x": xs}, {"y": ((n, h, w, 64), DT[store], (-1, 8, 48))}, launch, S16)
    _property(make)


def _hilo_pair(t):
    hi = t.to(torch.bfloat16)
    return torch.stack([hi, (t - hi.float()).to(torch.bfloat16)]).contiguous()


def _hilo_case(n, h, w, c, cp, kernel, lr_only=False):
    """hi + lo in / res / out (bf16): the head (pair out), the LR conv (pair residual, pair out), the upsampler (pair in, shuffle out)"""
    from ntire2022_esr_amd import _lib as L, ops
    g = _gen(n, h, w, c)
    x = _core(n, h, w, c, cp, torch.bfloat16, g)
    rp = _hilo_pair(F.pad(torch.randn(n, h, w, c, generator=g) * 3, (0, cp - c)))
    xp = _hilo_pair(F.pad(torch.randn(n, h, w, c, generator=g) * 2, (0, cp - c)))
    wt, b = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g)
    wu, bu = torch.randn(48, c, 3, 3, generator=g) * 0.1, torch.randn(48, generator=g)
    pair_out = {"y": ((2, n, h, w, _up(c, 16)), torch.bfloat16, "all")}

    def head(variant):
        return Case({"x": x}, pair_out, lambda t: ops.conv2d(t["x"], wt, b, cin=c, hilo=L.HILO_OUT, out=t["y"]), kernel[0])

    def lr(variant):
        return Case({"x": x, "r": rp}, pair_out, lambda t: ops.conv2d(t["x"], wt, b, cin=c, res=t["r"], res_mode=1, hilo=L.HILO_RES | L.HILO_OUT,
                                                                      out=t["y"]), kernel[1])

    def up(variant):
        return Case({"x": xp}, {"y": ((n, 3, 4 * h, 4 * w), torch.float32, "all")},
                    lambda t: ops.conv2d(t["x"], wu, bu, cin=c, hilo=L.HILO_IN, shuffle_out=True, out=t["y"]), kernel[2])
    _property(lr)
    if not lr_only:
        _property(head)
        _property(up)


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (1, 1, 90), (2, 5, 3)])
@pytest.mark.parametrize("c", [46, 50])
def test_s16_hilo_general_kernel(n, h, w, c):
    _hilo_case(n, h, w, c, _up(c, 16), (HILO, HILO, HILO))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", FOUR_WAVE)
def test_s16_four_wave_shape(store, n, h, w):
    """conv_s16_kernel's two-blocks-per-CU shape (S16_4W: 4 waves, 16 x 16 tiles): 32 -> 48 out of / into slices of wider buffers, and
    24 -> 40 at a tight pitch (48 input channels at these tile counts are conv48r_kernel's)"""
    _property(_conv(store, n, h, w, 32, 48, 3, in_pitch=48, in_coff=8, out_pitch=64, out_coff=8, kernel=S16_4W))
    _property(_conv(store, n, h, w, 24, 40, 3, kernel=S16_4W))             # tight pitch 24: the second K chunk's upper half is the next pixel


def _pack_desc(L, t, n, h, w, store):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.storage = n, h, w, 3, L.STORE[store]
    d.inp = L.View(ctypes.c_void_p(t["x"].data_ptr()), 0, 0)
    d.out0 = L.View(ctypes.c_void_p(t["slots"].data_ptr()), 32, 8)
    return d


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", SMALL)
def test_pack_input(store, n, h, w):
    """pack_input_kernel (esr_pack_input_s16): the NCHW fp32 network input as 16 16-bit slots [hi | lo | hi | 0] per pixel, stored into
    channels [8, 24) of a pitch-32 buffer"""
    from ntire2022_esr_amd import _lib as L
    x = torch.rand(n, 3, h, w, generator=_gen(n, h, w, 3)) * 255
    _property(_desc_case(L.OP_PACK_INPUT, lambda t: _pack_desc(L, t, n, h, w, store), {"x": x},
                         {"slots": ((n, h, w, 32), DT[store], (-1, 8, 16))}, rf"pack_input_kernel<{'true' if store == 'bf16' else 'false'}>"))


def _head(store, n, h, w, cout, kernel, hilo=False, post=0):
    """the head of a 16-bit plan as the engine runs it: pack_input_kernel, then conv_s16_kernel over the 16 slots with the weights as
    [w_hi | w_hi | w_lo] (engine.pack_head_s16); `slots` is written by the first launch and read by the second"""
    from ntire2022_esr_amd import _lib as L, ops
    g = _gen(n, h, w, cout, 3)
    dt = DT[store]
    x = torch.rand(n, 3, h, w, generator=g) * 255
    wt, b = torch.randn(cout, 3, 3, 3, generator=g) * 0.1, torch.randn(cout, generator=g)
    hi = wt.to(dt).float()
    w9 = torch.cat([hi, hi, wt - hi], dim=1)
    pw = (torch.randn(post, cout, generator=g) * 0.2, torch.randn(post, generator=g)) if post else None
    cp = _up(cout, 16) if hilo else _up(cout, 8)

    def make(variant):
        outs = {"slots": ((n, h, w, 32), dt, (-1, 8, 16)), "y": ((2, n, h, w, cp), dt, "all") if hilo else ((n, h, w, cp + 8), dt, (-1, 8, cp))}
        if post:
            outs["p"] = ((n, h, w, _up(post, 8) + 8), dt, (-1, 0, _up(post, 8)))

        def launch(t):
            ops._launch(L.OP_PACK_INPUT, _pack_desc(L, t, n, h, w, store), torch.cuda.current_stream().cuda_stream)
            kw = dict(cin=9, in_coff=8, out=t["y"], out_coff=0 if hilo else 8, hilo=L.HILO_OUT if hilo else 0)
            if post:
                kw.update(post_weight=pw[0], post_bias=pw[1], post_act=1, post_out=t["p"])
            ops.conv2d(t["slots"], w9, b, **kw)
        return Case({"x": x}, outs, launch, (r"pack_input_kernel<", kernel))
    return make


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,kernel", [(2, 23, 37, S16), (1, 31, 33, S16), (1, 1, 90, S16)] + [s + (S16_4W,) for s in FOUR_WAVE])
def test_s16_head_on_packed_input(store, n, h, w, kernel):
    """pack_input_kernel + conv_s16_kernel on 16 slots; from 512 tiles the head of a 46-channel network takes the 4-wave shape"""
    _property(_head(store, n, h, w, 46, kernel))


@pytest.mark.parametrize("n,h,w,kernel", [(2, 23, 37, HILO), (1, 31, 33, HILO), (1, 1, 90, HILO)] + [s + (HILO_4W,) for s in FOUR_WAVE])
def test_s16_hilo_head_on_packed_input(n, h, w, kernel):
    """the head with a hi + lo pair out (bf16): HILO / HILO_4W (46 channels, 512 .. 4095 tiles), and HILO_POST -- 50 channels with block 1's
    first distillation 1x1 (25 channels: two post tiles) in the epilogue"""
    _property(_head("bf16", n, h, w, 46, kernel, hilo=True))
    _property(_head("bf16", n, h, w, 50, HILO_POST, hilo=True, post=25))


@pytest.mark.parametrize("n,h,w", PERSIST)
def test_conv48rl_and_conv64m_hilo(n, h, w):
    """the LR conv on hi + lo pairs at >= 256 tiles: conv48rp_kernel<true, true> (48 channels) and conv64m_kernel<true, false, true, ..> (64)"""
    _hilo_case(n, h, w, 46, 48, (None, r"conv48rp_kernel<true, true>", None), lr_only=True)
    _hilo_case(n, h, w, 50, 64, (None, r"conv64m_kernel<true, false, true,", None), lr_only=True)


# conv48r_kernel counts tiles of 16 x 32: from 256 of them on 16 x 16 tiles (RW = 4), from 1024 on 16 x 32 tiles (RW = 8)
C48R = [s + (4,) for s in ((2, 257, 250), (48, 1, 90), (9, 150, 97))] + [s + (8,) for s in ((256, 33, 17), (171, 1, 90))]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,rw", C48R)
def test_conv48r(store, n, h, w, rw):
    """conv48r_kernel<bf16, NT, EXT, RW, ..>: plain with three output tiles, two tiles with the border table and GELU, residual = input"""
    bf = "true" if store == "bf16" else "false"
    _property(_conv(store, n, h, w, 46, 46, 3, in_pitch=48, out_pitch=64, out_coff=8, cin_phys=48, kernel=rf"conv48r_kernel<{bf}, 3, false, {rw},"))
    _property(_conv(store, n, h, w, 48, 24, 3, border=True, act=3, kernel=rf"conv48r_kernel<{bf}, 2, true, {rw},"))
    _property(_conv(store, n, h, w, 48, 48, 3, res="in", res_mode=1, act=0, kernel=rf"conv48r_kernel<{bf}, 3, true, {rw},"))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", PERSIST)
def test_conv48rp(store, n, h, w):
    """conv48rp_kernel: RLFB c3_r + the post chain, the main result not stored"""
    bf = "true" if store == "bf16" else "false"
    _property(_conv(store, n, h, w, 48, 46, 3, res="hbm", res_mode=2, post=46, post_act=0, post2=16, store_main=False, kernel=rf"conv48rp_kernel<{bf}, false>"))


@pytest.mark.parametrize("n,h,w", PERSIST)
def test_conv48rq(n, h, w):
    """conv48rq_kernel (fp16 storage only): stored result + one post 1x1 of two tiles"""
    _property(_conv("f16", n, h, w, 48, 48, 3, res="in", res_mode=1, act=1, post=24, post_act=1, kernel=r"conv48rq_kernel<false,"))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", PERSIST)
def test_persistent_64_channel_kernels(store, n, h, w):
    """conv64r_kernel (two output tiles), conv64m_kernel: plain (four output tiles, tight pitch 56 of nf = 50 too), with a post 1x1, and ESDB's
    three-chunk form (border table + GELU + input)"""
    bf = "true" if store == "bf16" else "false"
    _property(_conv(store, n, h, w, 50, 25, 3, in_pitch=64, cin_phys=64, kernel=rf"conv64r_kernel<{bf}, 2,"))
    _property(_conv(store, n, h, w, 64, 64, 3, out_pitch=80, out_coff=8, kernel=rf"conv64m_kernel<{bf}, false, false, 4,"))
    _property(_conv(store, n, h, w, 50, 50, 3, res="in", res_mode=1, kernel=rf"conv64m_kernel<{bf}, false, false, 4,"))             # tight: pitch 56
    _property(_conv(store, n, h, w, 50, 50, 3, in_pitch=64, res="in", res_mode=1, post=25, cin_phys=64, kernel=rf"conv64m_kernel<{bf}, true, false, 4,"))
    _property(_conv(store, n, h, w, 48, 48, 3, res="in", res_mode=1, act=3, border=True, kernel=rf"conv64m_kernel<{bf}, false, false, 3, true>"))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", PERSIST)
@pytest.mark.parametrize("esdb", [False, True])
def test_rfdb_and_esdb_tails(store, n, h, w, esdb):
    """rfdb_tail_kernel (ABI v12): c4 -> cat(d1, d2, d3, r4) -> c5 -> esa.conv1 in one launch; RFDB over 64 physical channels, ESDB over 48 with
    the border table and GELU.  v goes into a slice of a wider buffer, the three distilled tensors are one planar [3, N, H, W, 32] input."""
    _tails(store, n, h, w, esdb, (48, 24, 16) if esdb else (50, 25, 12))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("esdb", [False, True])
def test_rfdb_and_esdb_tails_at_their_smallest_widths(store, esdb):
    """... at the lower end of every channel range rfdb_tail_takes admits, on the smallest shape the kernel takes (256 tiles, a ragged right edge)"""
    _tails(store, 4, 128, 120, esdb, (33, 17, 1) if esdb else (49, 17, 1))


def _tails(store, n, h, w, esdb, widths):
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, pack_post_s16, pack_tail_s16
    dt = DT[store]
    nf, dc, f = widths
    cp = 48 if esdb else 64
    g = _gen(n, h, w, nf)
    r3 = _core(n, h, w, nf, cp, dt, g)
    ds = F.pad(torch.randn(3, n, h, w, dc, generator=g), (0, 32 - dc)).to(dt)
    w4, b4 = torch.randn(dc, nf, 3, 3, generator=g) * 0.1, torch.randn(dc, generator=g)
    w5, b5 = torch.randn(nf, 4 * dc, generator=g) * 0.15, torch.randn(nf, generator=g)
    wc, bc = torch.randn(f, nf, generator=g) * 0.2, torch.randn(f, generator=g)
    table = torch.randn(16, 32, generator=g) * 0.2
    table[0] = 0
    keep = [pack_conv_s16(w4, b4, store, cin_phys=cp).to(DEV), pack_tail_s16(w5, b5, 3, dc, dc, store).to(DEV), pack_post_s16(wc, bc, store).to(DEV),
            table.to(DEV)]

    def make(variant):
        outs = {"v": ((n, h, w, 72), dt, (-1, 8, _up(nf, 8))), "c1": ((n, h, w, 24), dt, (-1, 0, _up(f, 8)))}

        def launch(t):
            d = L.ConvDesc()
            d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, nf, dc, 3
            d.in_layout = d.out_layout = L.NHWC
            d.storage = d.compute = L.STORE[store]
            d.act, d.slope = L.ACT_NONE, 0.05
            d.inp = L.View(ctypes.c_void_p(t["r3"].data_ptr()), cp, 0)
            d.out0 = L.View(ctypes.c_void_p(t["v"].data_ptr()), 72, 8)
            d.wpacked, d.tail_wpacked = keep[0].data_ptr(), keep[1].data_ptr()
            d.tail_cat = L.View(ctypes.c_void_p(t["ds"].data_ptr()), 32, 0)
            d.tail_cat_c, d.tail_cout, d.tail_mid_act = 96, nf, (L.ACT_GELU if esdb else L.ACT_LRELU)
            d.tail_seg_stride16 = t["ds"][0].numel() * 2 // 16
            d.post_wpacked, d.post_out = keep[2].data_ptr(), L.View(ctypes.c_void_p(t["c1"].data_ptr()), 24, 0)
            d.post_cout, d.post_act = f, L.ACT_NONE
            if esdb:
                d.border_bias = keep[3].data_ptr()
            assert L.lib().esr_conv_tail_supported(ctypes.byref(d)) == 1
            ops._launch(L.OP_CONV, d, torch.cuda.current_stream().cuda_stream)
        return Case({"r3": r3, "ds": ds}, outs, launch, r"rfdb_tail_kernel<")
    _property(make)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 5, 3)])
def test_rlfb_chain(store, n, h, w):
    """rlfb_chain_kernel: three 3x3s + two 1x1s in one launch; v and c1 into buffers wider than their channels.  The strip is 5 x 3:
    esr_conv_chain_supported refuses h < 4, so 1 x 90 is not a shape of this kernel"""
    _chain(store, n, h, w, 46, 48, 16)


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_rlfb_chain_at_its_smallest_widths(store):
    _chain(store, 2, 23, 37, 33, 33, 1)


def _chain(store, n, h, w, nf, mf, f):
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, nf)
    ws = [torch.randn(mf, nf, 3, 3, generator=g) * 0.06, torch.randn(mf, mf, 3, 3, generator=g) * 0.06, torch.randn(nf, mf, 3, 3, generator=g) * 0.06]
    bs = [torch.randn(c, generator=g) * 0.1 for c in (mf, mf, nf)]
    w5, b5, w1, b1 = torch.randn(nf, nf, generator=g) * 0.15, torch.randn(nf, generator=g) * 0.1, torch.randn(f, nf, generator=g) * 0.15, torch.randn(f, generator=g) * 0.1
    x = _core(n, h, w, nf, 48, DT[store], g)

    def make(variant):
        outs = {"v": ((n, h, w, 64), DT[store], (-1, 0, 48)), "c1": ((n, h, w, 24), DT[store], (-1, 0, _up(f, 8)))}
        return Case({"x": x}, outs, lambda t: ops.conv_chain(t["x"], ws, bs, w5, b5, w1, b1, cin=nf, v_out=t["v"], c1_out=t["c1"]), r"rlfb_chain_kernel<")
    _property(make)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (1, 1, 90), (2, 5, 3)])
def test_hfab(store, n, h, w):
    """hfab_kernel (ESR_RES_GATE chain): nf = 50 in pitch 56; channels of `in` at and beyond cin are never read (foreign noise there)"""
    _hfab(store, n, h, w, 50, 16, 56)


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_hfab_at_its_smallest_widths(store):
    """cin = 33 in pitch 40 (three chunks, one channel of the last 16-byte piece kept, seven slots of foreign noise cleared), cmid = 1"""
    _hfab(store, 2, 23, 37, 33, 1, 40)


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_distill_step_at_its_smallest_widths(store):
    """distill_step_kernel at cin = cmid = cout = 17 (the residual form): `in` in pitch 24 with foreign noise in its seven pad slots, d and out
    into slices of wider buffers"""
    from ntire2022_esr_amd import ops
    n, h, w, c = 2, 23, 37, 17
    g = _gen(n, h, w, c)
    wd, bd = torch.randn(c, c, 1, 1, generator=g) * 0.15, torch.randn(c, generator=g) * 0.2
    wr, br = torch.randn(c, c, 3, 3, generator=g) * 0.05, torch.randn(c, generator=g) * 0.1
    wb, bb = torch.randn(c, c, 3, 3, generator=g) * 0.05, torch.randn(c, generator=g) * 0.1
    x = torch.randn(n, h, w, c, generator=g).to(DT[store])

    def make(variant):
        outs = {"d": ((n, h, w, 40), DT[store], (-1, 8, 24)), "y": ((n, h, w, 32), DT[store], (-1, 0, 24))}
        return Case({"x": _widen(x, 24, 0, variant, 7)}, outs,
                    lambda t: ops.distill_step(t["x"], wd, bd, wr, br, wb, bb, res=True, cin=c, d_out=t["d"], d_coff=8, out=t["y"]),
                    r"distill_step_kernel<(true|false), 2, true>")
    _property(make)


@pytest.mark.parametrize("store", ["bf16", "f16"])
def test_resblock_head_at_its_smallest_width(store):
    """resblock_head_kernel with one esa.conv1 channel (c1: one 16-byte granule stored), with g"""
    from ntire2022_esr_amd import ops
    n, h, w, c = 2, 23, 37, 32
    g = _gen(n, h, w, c)
    w1, b1 = torch.randn(c, c, 3, 3, generator=g) * 0.06, torch.randn(c, generator=g) * 0.1
    w2, b2 = torch.randn(c, c, 3, 3, generator=g) * 0.06, torch.randn(c, generator=g) * 0.1
    wc, bc = torch.randn(1, c, 1, 1, generator=g) * 0.15, torch.randn(1, generator=g) * 0.2
    x, gg = torch.randn(n, h, w, c, generator=g).to(DT[store]), (torch.randn(n, h, w, c, generator=g) * 0.5).to(DT[store])

    def make(variant):
        outs = {"xs": ((n, h, w, 40), DT[store], (-1, 8, 32)), "u": ((n, h, w, 32), DT[store], "all"), "c1": ((n, h, w, 16), DT[store], (-1, 0, 8))}
        return Case({"x": _widen(x, 48, 8, variant, 3), "g": gg}, outs,
                    lambda t: ops.resblock_head(t["x"], w1, b1, w2, b2, wc, bc, g=t["g"], in_coff=8, x_out=t["xs"], x_coff=8, u_out=t["u"], c1_out=t["c1"]),
                    r"resblock_head_kernel<(true|false), true>")
    _property(make)


def _hfab(store, n, h, w, cin, cmid, pitch):
    from ntire2022_esr_amd import _lib as L, ops
    g = _gen(n, h, w, cin)
    ws = [torch.randn(cmid, cin, 3, 3, generator=g) * 0.1, torch.randn(cmid, cmid, 3, 3, generator=g) * 0.1, torch.randn(cmid, cmid, 3, 3, generator=g) * 0.1,
          torch.randn(cin, cmid, 3, 3, generator=g) * 0.1]
    bs = [torch.randn(c, generator=g) * 0.1 for c in (cmid, cmid, cmid, cin)]
    x = (torch.randn(n, h, w, cin, generator=g) * 2).to(DT[store])

    def make(variant):
        return Case({"x": _widen(x, pitch, 0, variant, 5)}, {"y": ((n, h, w, pitch), DT[store], "all")},
                    lambda t: ops.conv_chain(t["x"], ws, bs, slope=0.1, res_mode=L.RES_GATE, cin=cin, out=t["y"]), r"hfab_kernel<")
    _property(make)


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (1, 1, 90), (2, 5, 3)])
def test_bsconv(store, n, h, w):
    """esr_bsconv_f32 with the distillation output; input a slice of a wider buffer, residual from HBM"""
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, 48)
    c, dco, gran = 48, 24, (4 if store == "f32" else 8)
    pw, pb = torch.randn(c, c, generator=g) * 0.2, torch.randn(c, generator=g)
    dw, db = torch.randn(c, 1, 3, 3, generator=g) * 0.3, torch.randn(c, generator=g)
    wd, bd = torch.randn(dco, c, generator=g) * 0.2, torch.randn(dco, generator=g)
    x, r = _core(n, h, w, c, c, DT[store], g), _core(n, h, w, c, c, DT[store], g)

    def make(variant):
        outs = {"y": ((n, h, w, c + 8), DT[store], (-1, 0, c)), "d": ((n, h, w, dco + 8), DT[store], (-1, 0, dco))}
        return Case({"x": _widen(x, c + 2 * gran, gran, variant, 1), "r": r}, outs,
                    lambda t: ops.bsconv(t["x"], pw, pb, dw, db, act=3, res=t["r"], res_mode=1, in_coff=gran, cin=c, d_weight=wd, d_bias=bd, d_act=3,
                                         out=t["y"], d_out=t["d"]), r"bsconv_kernel<")
    _property(make)


def _desc_case(kind, build, ins, outs, kernel):
    from ntire2022_esr_amd import ops

    def make(variant):
        def launch(t):
            ops._launch(kind, build(t), torch.cuda.current_stream().cuda_stream)
        return Case(ins(variant) if callable(ins) else ins, outs, launch, kernel)
    return make


@pytest.mark.parametrize("n,h,w", [(2, 23, 31), (1, 31, 33), (2, 1, 5), (1, 90, 1)])
def test_dwconv(n, h, w):
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_dw
    g = _gen(n, h, w, 12)
    c = 46
    wt, b = torch.randn(c, 1, 3, 3, generator=g) * 0.3, torch.randn(c, generator=g)
    pk = pack_dw(wt, b).to(DEV)
    x, r = _core(n, h, w, c, 48, torch.float32, g), _core(n, h, w, c, 48, torch.float32, g)

    def build(t):
        d = L.ConvDesc()
        d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, c, c, 3
        d.act, d.slope, d.res_mode = 3, 0.05, 1
        d.inp = L.View(ctypes.c_void_p(t["x"].data_ptr()), 64, 8)
        d.out0 = L.View(ctypes.c_void_p(t["y"].data_ptr()), 64, 4)
        d.res = L.View(ctypes.c_void_p(t["r"].data_ptr()), 48, 0)
        d.wpacked = pk.data_ptr()
        return d
    _property(_desc_case(L.OP_DWCONV, build, lambda v: {"x": _widen(x, 64, 8, v, 1), "r": r},
                         {"y": ((n, h, w, 64), torch.float32, (-1, 4, 48))}, r"dwconv3x3_kernel<0>"))


def _nhwc16(t, dt):
    return F.pad(t.permute(0, 2, 3, 1), (0, 16 - t.shape[1])).to(dt).contiguous()


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 15, 15)])
def test_esa_conv3x3s2_and_pools(store, n, h, w):
    """esr_conv3x3s2_f32, esr_maxpool7s3_f32 (fp32 maps) and esr_maxpool7s7_f32 on the conv1 map [n, h, w, 16]"""
    from ntire2022_esr_amd import _lib as L
    from ntire2022_esr_amd.engine import pack_dense
    g = _gen(n, h, w, 3)
    f = 12
    x = _nhwc16(torch.randn(n, f, h, w, generator=g), DT[store])
    wt, b = torch.randn(f, f, 3, 3, generator=g) * 0.2, torch.randn(f, generator=g)
    pk = pack_dense(wt, b, 16, 16).to(DEV)
    h2, w2, h7, w7 = (h - 3) // 2 + 1, (w - 3) // 2 + 1, (h - 5) // 7 + 1, (w - 5) // 7 + 1

    def desc(hi, wi, ho, wo, storage):
        def build(t):
            d = L.EsaDesc()
            d.n, d.h, d.w, d.c, d.f, d.h_lo, d.w_lo, d.storage = n, hi, wi, 0, f, ho, wo, storage
            d.x, d.y = L.View(ctypes.c_void_p(t["x"].data_ptr()), 16, 0), L.View(ctypes.c_void_p(t["y"].data_ptr()), 16, 0)
            d.w0 = pk.data_ptr()
            return d
        return build
    _property(_desc_case(L.OP_CONV3X3S2, desc(h, w, h2, w2, L.STORE[store]), {"x": x},
                         {"y": ((n, h2, w2, 16), torch.float32, "all")}, r"conv3x3s2_kernel<"))
    _property(_desc_case(L.OP_MAXPOOL7S7, desc(h, w, h7, w7, L.STORE[store]), {"x": x},
                         {"y": ((n, h7, w7, 16), torch.float32, "all")}, r"esa_pool7_kernel<"))


@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 7, 90)])
def test_esa_maxpool7s3(n, h, w):
    """esr_maxpool7s3_f32 (fp32 maps only; a window needs 7 rows and columns, so the strip is 7 x 90: one output row)"""
    from ntire2022_esr_amd import _lib as L
    f = 12
    x = _nhwc16(torch.randn(n, f, h, w, generator=_gen(n, h, w, 73)), torch.float32)
    h3, w3 = (h - 7) // 3 + 1, (w - 7) // 3 + 1

    def build(t):
        d = L.EsaDesc()
        d.n, d.h, d.w, d.c, d.f, d.h_lo, d.w_lo, d.storage = n, h, w, 0, f, h3, w3, 0
        d.x, d.y = L.View(ctypes.c_void_p(t["x"].data_ptr()), 16, 0), L.View(ctypes.c_void_p(t["y"].data_ptr()), 16, 0)
        return d
    _property(_desc_case(L.OP_MAXPOOL7S3, build, {"x": x}, {"y": ((n, h3, w3, 16), torch.float32, "all")}, r"maxpool7s3_kernel"))


def _lowres_desc(L, t, n, h, w, f, storage, blobs, s2):
    d = L.EsaLowresDesc()
    d.n, d.h, d.w, d.f, d.storage = n, h, w, f, storage
    d.x = L.View(ctypes.c_void_p(t["x"].data_ptr()), 16, 0)
    d.pooled, d.y = t["pooled"].data_ptr(), t["y"].data_ptr()
    if s2:
        d.n_layers, d.w_s2 = 2, blobs[0].data_ptr()
        d.layer[0].kind, d.layer[0].act, d.layer[0].w = 0, L.ACT_RELU, blobs[1].data_ptr()
        d.layer[1].kind, d.layer[1].act, d.layer[1].w = 0, L.ACT_NONE, blobs[2].data_ptr()
    else:
        d.n_layers, d.w_s2 = 2, None
        d.layer[0].kind, d.layer[0].act, d.layer[0].w, d.layer[0].w_dw = 2, L.ACT_RELU, blobs[0].data_ptr(), blobs[1].data_ptr()
        d.layer[1].kind, d.layer[1].act, d.layer[1].w = 3, L.ACT_NONE, blobs[3].data_ptr()
    return d


def _lowres_blobs(f, g, center_tap=False):
    from ntire2022_esr_amd.engine import pack_dense
    ws = [(torch.randn(f, f, 3, 3, generator=g) * 0.2, torch.randn(f, generator=g) * 0.1) for _ in range(3)]
    if center_tap:          # conv2 = the identity on the centre tap: its output is x[2i + 1, 2j + 1] exactly
        w0 = torch.zeros(f, f, 3, 3)
        w0[torch.arange(f), torch.arange(f), 1, 1] = 1.0
        ws[0] = (w0, torch.zeros(f))
    w32 = torch.zeros(f, 32, 3, 3)
    w32[:, :f], w32[:, 16:16 + f] = ws[2][0], ws[1][0]
    return [pack_dense(wl, bl, 16, 16).to(DEV) for wl, bl in ws] + [pack_dense(w32, ws[2][1], 32, 16).to(DEV)]


@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 33, 37), (1, 31, 33), (2, 17, 90)])
@pytest.mark.parametrize("s2", [True, False])
def test_esa_lowres(store, n, h, w, s2):
    """esr_esa_lowres_f32, both forms (conv2 s2 + max_pool(7, 3) + layers; max_pool(7, 7, 1) + the pair + conv_23): `pooled` and `y` guarded"""
    from ntire2022_esr_amd import _lib as L
    g = _gen(n, h, w, 16)
    f = 12
    x = _nhwc16(torch.randn(n, f, h, w, generator=g) * 3, DT[store])
    blobs = _lowres_blobs(f, g)
    ho, wo = (((h - 3) // 2 + 1 - 7) // 3 + 1, ((w - 3) // 2 + 1 - 7) // 3 + 1) if s2 else ((h - 5) // 7 + 1, (w - 5) // 7 + 1)
    outs = {"pooled": ((n, ho, wo, 16), torch.float32, "all"), "y": ((n, ho, wo, 16), torch.float32, "all")}
    _property(_desc_case(L.OP_ESA_LOWRES, lambda t: _lowres_desc(L, t, n, h, w, f, L.STORE[store], blobs, s2), {"x": x}, outs,
                         r"esa_s2pool(16)?_kernel<\d> \+ esa_chain_kernel" if s2 else r"esa_pool7_kernel<\d> \+ esa_pool7_branch_kernel"))


@pytest.mark.parametrize("store,c,posts,skip", [("f32", 50, 0, False), ("bf16", 50, 0, False), ("bf16", 50, 1, False), ("f16", 48, 2, True), ("bf16", 48, 2, True),
                                                ("f16", 48, 1, True)])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (1, 1, 90)])
def test_esa_apply(store, c, posts, skip, n, h, w):
    """esr_esa_apply_f32 with 0, 1 and 2 posts; skip_y: the y buffer is declared as not stored and must keep every byte"""
    from ntire2022_esr_amd import _lib as L, ops
    g = _gen(n, h, w, c, posts)
    dt, f, gran = DT[store], (12 if c == 50 else 16), (4 if store == "f32" else 8)
    pitch = _up(c, 8)
    x = _core(n, h, w, c, pitch, dt, g, 3.0)
    c1 = _core(n, h, w, f, 16, dt, g)
    c3 = _core(n, 3, 4, f, 16, torch.float32, g)
    res = _core(n, h, w, c, pitch, dt, g)
    wf, bf = torch.randn(f, f, generator=g) * 0.3, torch.randn(f, generator=g)
    w4, b4 = torch.randn(c, f, generator=g) * 0.3, torch.randn(c, generator=g)
    co = [(25,), (48, 24)][posts - 1] if posts else ()
    post = None
    if posts == 1:
        post = [dict(weight=torch.randn(co[0], c, generator=g) * 0.2, bias=torch.randn(co[0], generator=g), act=L.ACT_LRELU)]
        if skip:
            post = [dict(weight=torch.randn(48, c, generator=g) * 0.2, bias=torch.randn(48, generator=g), act=L.ACT_NONE, res="res")]
            co = (48,)
    elif posts == 2:
        post = [dict(weight=torch.randn(48, c, generator=g) * 0.2, bias=torch.randn(48, generator=g), act=L.ACT_NONE, res="res"),
                dict(weight=torch.randn(24, 48, generator=g) * 0.2, bias=torch.randn(24, generator=g), act=L.ACT_GELU)]
    assert not posts or L.lib().esr_esa_apply_post_supported(c, co[0], co[1] if posts == 2 else 0) == 1

    def make(variant):
        ins = {"x": x, "c1": c1, "c3": c3}
        if post and post[0].get("res") is not None:
            ins["res"] = res
        outs = {"y": ((n, h, w, pitch), dt, None if skip else (-1, 0, _up(c, gran)))}
        for i, cc in enumerate(co):
            outs[f"p{i}"] = ((n, h, w, _up(cc, 8) + 8), dt, (-1, 0, _up(cc, 8)))

        def launch(t):
            p = None if post is None else [dict(q, res=t["res"]) if q.get("res") is not None else q for q in post]
            ops.esa_apply(t["x"], t["c1"], t["c3"], wf, bf, w4, b4, out=t["y"], post=p, skip_y=skip, post_out=[t[f"p{i}"] for i in range(len(co))] or None)
        return Case(ins, outs, launch, r"esa_apply_mfma_kernel<" if store != "f32" else r"esa_apply_kernel<0>")
    _property(make)


@pytest.mark.parametrize("store,tol", [("f32", 2e-5), ("bf16", 2.0 ** -7), ("f16", 2.0 ** -10)])
@pytest.mark.parametrize("c", [48, 50, 64])
@pytest.mark.parametrize("n,h,w", [(2, 19, 23), (1, 31, 33), (1, 1, 90)])
def test_channel_attention_nhwc_views(store, tol, c, n, h, w):
    """esr_channel_attention_f32 on NHWC views with coff > 0 and pitch > round_up(c, 4) (c = 50: the c % 4 != 0 path).  fp64 atomics: (b) and (c)
    are the fp64 restatement and the tolerances of tests/test_gpu_ca.py; (a) holds bit for bit"""
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, c)
    dt, cr, c4 = DT[store], 12, _up(c, 4)
    x = F.pad(torch.randn(n, h, w, c, generator=g) * 2 + 1.5, (0, c4 - c)).to(dt)
    w1, b1 = torch.randn(cr, c, generator=g) * 0.3, torch.randn(cr, generator=g) * 0.1
    w2, b2 = torch.randn(c, cr, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1
    xd = x[..., :c].double()
    s = xd.std(dim=(1, 2), unbiased=False) + xd.mean(dim=(1, 2))
    ref = xd * torch.sigmoid(torch.relu(s @ w1.double().T + b1.double()) @ w2.double().T + b2.double())[:, None, None, :]

    def make(variant):
        return Case({"x": _widen(x, c4 + 16, 8, variant, 1)}, {"y": ((n, h, w, c4 + 12), dt, (-1, 4, c4))},
                    lambda t: ops.channel_attention(t["x"], w1, b1, w2, b2, contrast=True, coff=8, out=t["y"], out_coff=4))
    results, _ = _run_guarded(make)
    for r in results + [_run_fresh(make)]:
        err = (r["y"][..., :c].double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)
        assert float(err.max()) < tol


@pytest.mark.parametrize("n,h,w", [(2, 19, 23), (1, 1, 90), (2, 5, 3)])
def test_channel_attention_nchw(n, h, w):
    from ntire2022_esr_amd import ops
    g = _gen(n, h, w, 50, 1)
    c, cr = 50, 12
    x = torch.randn(n, c, h, w, generator=g) * 2 + 1.5
    w1, b1 = torch.randn(cr, c, generator=g) * 0.3, torch.randn(cr, generator=g) * 0.1
    w2, b2 = torch.randn(c, cr, generator=g) * 0.3, torch.randn(c, generator=g) * 0.1
    xd = x.double()
    s = xd.mean(dim=(2, 3))
    ref = xd * torch.sigmoid(torch.relu(s @ w1.double().T + b1.double()) @ w2.double().T + b2.double())[:, :, None, None]

    def make(variant):
        return Case({"x": x}, {"y": ((n, c, h, w), torch.float32, "all")}, lambda t: ops.channel_attention(t["x"], w1, b1, w2, b2, nchw=True, out=t["y"]))
    results, _ = _run_guarded(make)
    for r in results + [_run_fresh(make)]:
        assert float(((r["y"].double().cpu() - ref).abs() / ref.abs().clamp_min(1.0)).max()) < 2e-5


def _u8_pair(h, w):
    g = _gen(h, w)
    a = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    return a, (a.int() + torch.randint(-9, 10, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8)


@pytest.mark.parametrize("h,w", [(23, 37), (31, 33), (1, 90)])
def test_tensor2uint(h, w):
    """esr_tensor2uint_u8 and esr_tensor2uint_u8_chk (the flag word is guarded too)"""
    from ntire2022_esr_amd import ops
    img = torch.rand(3, h, w, generator=_gen(h, w, 5)) * 1.2 - 0.1
    _property(lambda v: Case({"x": img}, {"u8": ((h, w, 3), torch.uint8, "all")}, lambda t: ops.tensor2uint_device(t["x"], 1.0, out=t["u8"])))

    def chk(v):
        def launch(t):
            t["flag"].zero_()
            ops.tensor2uint_device(t["x"], 1.0, nonfinite=t["flag"], out=t["u8"])
        return Case({"x": img}, {"u8": ((h, w, 3), torch.uint8, "all"), "flag": ((1,), torch.int32, "all")}, launch)
    _property(chk)


@pytest.mark.parametrize("h,w,border", [(23, 37, 0), (23, 37, 4), (31, 33, 4), (1, 90, 0)])
def test_sqerr(h, w, border):
    """esr_sqerr_u8 (the descriptor refuses 2 * border >= h: the strip runs with border 0)"""
    from ntire2022_esr_amd import ops
    a, b = _u8_pair(h, w)
    _property(lambda v: Case({"a": a, "b": b}, {"acc": ((1,), torch.int64, "all")}, lambda t: ops.sqerr_device(t["a"], t["b"], border, out=t["acc"])))


@pytest.mark.parametrize("h,w,border", [(23, 37, 0), (23, 37, 4), (31, 33, 0), (33, 31, 4), (11, 90, 0), (19, 90, 4)])
def test_ssim(h, w, border):
    """esr_ssim_u8, borders 0 and 4; the partials buffer is guarded too.  An 11 x 11 window needs 11 rows and columns inside the border, so
    the strips are 11 x 90 and 19 x 90: one row of windows"""
    from ntire2022_esr_amd import _lib as L, ops
    a, b = _u8_pair(h, w)
    npart = int(L.lib().esr_ssim_partials(h, w, 3, border))
    assert npart > 0
    _property(lambda v: Case({"a": a, "b": b}, {"part": ((npart,), torch.float64, "all")}, lambda t: ops.ssim_sum_device(t["a"], t["b"], border, partials=t["part"])))


# ---- all-negative pool inputs: a zero-padded window edge would win the maximum ---------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("n,h,w", [(2, 23, 37), (1, 31, 33), (2, 15, 90)])
def test_pools_on_strictly_negative_inputs(store, n, h, w):
    """esr_maxpool7s3_f32, esr_maxpool7s7_f32 and both pooling paths of esr_esa_lowres_f32 on -|randn| - 1: exact against F.max_pool2d on the
    same values (the pools of the other tests see randn * 3, where every 7 x 7 window holds a positive value).  conv2 of the stride-2 form is
    the identity on its centre tap, so the map it pools is x[2i + 1, 2j + 1] exactly."""
    from ntire2022_esr_amd import _lib as L
    g = _gen(n, h, w, 99)
    f, dt = 12, DT[store]
    xq = (-torch.randn(n, f, h, w, generator=g).abs() - 1).to(dt).float()
    assert float(xq.max()) <= -1.0
    xd = _nhwc16(xq, dt).to(DEV)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def esa(hi, wi, ho, wo, x, storage):
        y = torch.full((n, ho, wo, 16), float("nan"), device=DEV)
        d = L.EsaDesc()
        d.n, d.h, d.w, d.f, d.h_lo, d.w_lo, d.storage = n, hi, wi, f, ho, wo, storage
        d.x, d.y = L.View(ctypes.c_void_p(x.data_ptr()), 16, 0), L.View(ctypes.c_void_p(y.data_ptr()), 16, 0)
        return d, y
    want7 = F.max_pool2d(xq, 7, 7, padding=1)
    d, y = esa(h, w, want7.shape[2], want7.shape[3], xd, L.STORE[store])
    L.check(L.lib().esr_maxpool7s7_f32(ctypes.byref(d), st), "esr_maxpool7s7_f32")
    assert torch.equal(y.cpu()[..., :f].permute(0, 3, 1, 2), want7)
    x32 = _nhwc16(xq, torch.float32).to(DEV)
    want3 = F.max_pool2d(xq, 7, 3)
    d, y = esa(h, w, want3.shape[2], want3.shape[3], x32, 0)
    L.check(L.lib().esr_maxpool7s3_f32(ctypes.byref(d), st), "esr_maxpool7s3_f32")
    assert torch.equal(y.cpu()[..., :f].permute(0, 3, 1, 2), want3)
    blobs = _lowres_blobs(f, g, center_tap=True)
    h2, w2 = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    for s2, want in ((True, F.max_pool2d(xq[:, :, 1:2 * h2:2, 1:2 * w2:2], 7, 3)), (False, want7)):
        t = {"x": xd, "pooled": torch.full((n, want.shape[2], want.shape[3], 16), float("nan"), device=DEV),
             "y": torch.full((n, want.shape[2], want.shape[3], 16), float("nan"), device=DEV)}
        d = _lowres_desc(L, t, n, h, w, f, L.STORE[store], blobs, s2)
        L.check(L.lib().esr_esa_lowres_f32(ctypes.byref(d), st), "esr_esa_lowres_f32")
        torch.cuda.synchronize()
        assert torch.equal(t["pooled"].cpu()[..., :f].permute(0, 3, 1, 2), want), ("s2" if s2 else "s7")


# ---- caller-provided outputs are validated before anything is launched -----------------------------------------------------------------
def test_provided_outputs_are_validated():
    """EsrError for a provided output of the wrong dtype, pitch or shape, for post_out without post weights, and for HFAB's `out` (which
    used to reach the kernel unchecked); the checks of the value itself: tests/test_ops_provided.py"""
    from ntire2022_esr_amd import _lib as L, ops
    n, h, w = 1, 9, 11
    g = _gen(n, h, w)
    x = torch.randn(n, h, w, 48, generator=g).to(torch.bfloat16).to(DEV)
    wt, b = torch.randn(48, 48, 3, 3, generator=g) * 0.1, torch.randn(48, generator=g)
    pw, pb = torch.randn(24, 48, generator=g) * 0.2, torch.randn(24, generator=g)

    def out(c, dt=torch.bfloat16, hh=h, dev=DEV):
        return torch.zeros(n, hh, w, c, dtype=dt, device=dev)
    for bad in (out(24, torch.float16), out(20), out(16), out(24, hh=h + 1), out(24, dev="cpu")):
        with pytest.raises(L.EsrError, match="post_out"):
            ops.conv2d(x, wt, b, post_weight=pw, post_bias=pb, post_out=bad)
    with pytest.raises(L.EsrError, match="without the post weights"):
        ops.conv2d(x, wt, b, post_out=out(24))
    with pytest.raises(L.EsrError, match="post2_out"):
        ops.conv2d(x, wt, b, post_weight=pw, post_bias=pb, post2_weight=torch.randn(16, 24, generator=g), post2_bias=None, post2_out=out(12))
    ws = [torch.randn(16, 48, 3, 3, generator=g) * 0.1] + [torch.randn(16, 16, 3, 3, generator=g) * 0.1] * 2 + [torch.randn(48, 16, 3, 3, generator=g) * 0.1]
    bs = [None] * 4
    for bad in (out(40), out(48, torch.float16), out(48, hh=h + 1)):
        with pytest.raises(L.EsrError, match="conv_chain: out"):
            ops.conv_chain(x, ws, bs, slope=0.1, res_mode=L.RES_GATE, cin=48, out=bad)
    rl = [torch.randn(48, 48, 3, 3, generator=g) * 0.06 for _ in range(3)]
    with pytest.raises(L.EsrError, match="v_out"):
        ops.conv_chain(x, rl, [None] * 3, torch.randn(48, 48, generator=g), None, torch.randn(16, 48, generator=g), None, v_out=out(40))
    with pytest.raises(L.EsrError, match="c1_out"):
        ops.conv_chain(x, rl, [None] * 3, torch.randn(48, 48, generator=g), None, torch.randn(16, 48, generator=g), None, c1_out=out(16, torch.float16))
