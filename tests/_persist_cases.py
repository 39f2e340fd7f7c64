"""The per-form value cases of the persistent kernels, shared by the suites they were lifted from (tests/test_gpu_h16.py,
tests/test_gpu_c64m.py, tests/test_gpu_wino.py, tests/test_gpu_conv.py) and by tests/test_gpu_thin_batches.py.

A persistent kernel is chosen only when a launch has enough tiles (s16_select / s16_four_waves in csrc/esr_s16.hip, conv_block_waves in
csrc/esr_hip.hip, the strip count in esr_conv2d_wino).  Each function below is one form: it builds the inputs of a batch of `n` images of
`hw`, runs the launch under ops.kernel_trace() and returns a Case -- the outputs as launched, the fp64 restatement of the same operation on
the same 16-bit inputs and the blob's EFFECTIVE weights, the device symbols, and `chunk(lo, hi)`: the same launch on images [lo, hi) alone.
The callers hold the assertions; nothing here compares.

`period` builds the batch as base[i % period] from `period` distinct random images (None: n distinct images, what the lifted tests use), so
that output i must equal output i % period bit for bit.

SHAPES and FORMS are the thin-batch table: sixteen image shapes that cover every row residue of a wave, one to four tiles across, one to
three down, and the forms with the tile threshold each is chosen at.  The module imports without a GPU (tests/test_thin_batch_table.py)."""
import ctypes

import torch
import torch.nn.functional as F

DEV = "cuda:0"
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
ACTS = {0: lambda t: t, 1: lambda t: F.leaky_relu(t, 0.05), 2: F.relu, 3: lambda t: F.gelu(t)}

SHAPES = [(1, 1), (1, 33), (2, 16), (3, 17), (4, 49), (5, 15), (7, 2), (8, 32),
          (9, 31), (15, 1), (16, 48), (17, 17), (31, 16), (32, 33), (33, 15), (33, 49)]


def tiles_per_image(hw, unit):
    """tiles of one image in a form's own unit: "t16" 16 x 16, "t32" 16 wide x 32 high, "strip" 4 rows x 16 columns"""
    rows = {"t16": 16, "t32": 32, "strip": 4}[unit]
    return ((hw[1] + 15) // 16) * ((hw[0] + rows - 1) // rows)


def batch_for(hw, unit, threshold):
    """the smallest batch that reaches `threshold` tiles, plus one image (keeps the tile count off any multiple of the grid)"""
    tpi = tiles_per_image(hw, unit)
    return (threshold + tpi - 1) // tpi + 1


def chunk_bounds(n, k):
    """n images as k consecutive chunks of (nearly) equal size"""
    step = (n + k - 1) // k
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


class Case:
    """one launch of one form: names (device symbols), outs (tensors as launched; a hi + lo pair is [2, n, h, w, P]), refs (fp64 NCHW, one per
    output), pads (per output: the logical channel count behind which the granule must be zero, or None), chunk(lo, hi) -> (outs, names)"""

    def __init__(self, names, outs, refs, chunk=None, pair=False, pads=None, **extra):
        self.names, self.outs, self.refs, self.chunk, self.pair = names, outs, refs, chunk, pair
        self.pads = pads if pads is not None else [None] * len(outs)
        self.extra = extra

    def got(self, k=0):
        """output k as fp64 NCHW over the reference's channels (a pair: hi + lo)"""
        y = self.outs[k]
        v = y[0].double() + y[1].double() if self.pair else y.double()
        return v.permute(0, 3, 1, 2)[:, :self.refs[k].shape[1]]

    def image(self, k, i):
        """image i of output k (every stored channel)"""
        return self.outs[k][:, i] if self.pair else self.outs[k][i]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _rep(t, n, period, axis=0):
    """the batch base[i % period] of a tensor of `period` images (period None: t is the batch)"""
    if period is None:
        return t
    return t.index_select(axis, (torch.arange(n) % period).to(t.device)).contiguous()


def _hilo(t, cp):
    """NCHW fp32 -> bf16 pair [2, N, H, W, cp]: high parts, low parts (value = hi + lo; pad channels zero)"""
    t = F.pad(_nhwc(t), (0, cp - t.shape[1]))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo]).contiguous()


def _hilo_w(w, dt):
    """the 16-bit hi + lo value of an fp32 weight (what the 1x1 images hold)"""
    hi = w.to(dt).float()
    return (hi + (w - hi).to(dt).float()).double()


def border_mask(hw):
    """[h, w] table row of each pixel: (x == 0) | (x == W - 1) << 1 | (y == 0) << 2 | (y == H - 1) << 3"""
    ys, xs = torch.arange(hw[0], device=DEV), torch.arange(hw[1], device=DEV)
    return ((xs == 0).long() + 2 * (xs == hw[1] - 1).long())[None, :] + (4 * (ys == 0).long() + 8 * (ys == hw[0] - 1).long())[:, None]


def conv48r(compute, n, hw, cin, cout, act, res_in, border, period=None):
    """3x3 over 48 physical input channels, plain / + input / two output tiles / a RANDOM border table (no fp64 side for that one: refs[0] is
    None): conv48r_kernel from 256 tiles of 16 x 32 (tests/test_gpu_h16.py::test_conv48r_equals_conv_s16)"""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(cin + cout + act + hw[0] + n)
    cp = 48
    xb = torch.randn(period or n, cin, *hw, generator=g).to(dt)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    table = (torch.randn(16, (cout + 15) // 16 * 16, generator=g) * 0.2) if border else None
    if table is not None:
        table[0] = 0                                    # row 0 = interior pixels of a border tile
    blob = pack_conv_s16(w, b, compute, cin_phys=cp).to(DEV)
    xin = _rep(F.pad(_nhwc(xb), (0, cp - cin)).to(DEV), n, period)
    kw = dict(act=act, cin=cin, packed=blob, border=None if table is None else table.to(DEV))
    if res_in:
        kw.update(res=xin, res_mode=L.RES_PRE_ACT)

    def chunk(lo, hi):
        kw1 = dict(kw)
        if res_in:
            kw1["res"] = xin[lo:hi]
        with ops.kernel_trace() as names:
            y1 = ops.conv2d(xin[lo:hi].contiguous(), w, b, **kw1)
        return [y1], names

    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w, b, **kw)
    ref = None
    if not border:
        weff, _ = unpack_conv_s16(blob.cpu(), cin, cout, 3, compute, cin_phys=cp)
        conv = F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=1)
        if res_in:
            conv = conv + xb.double().to(DEV)[:, :cout]
        ref = _rep(ACTS[act](conv), n, period)
    return Case(names, [y], [ref], chunk, pads=[cout], xin=xin, w=w, b=b, kw=kw)


def bsconv48(compute, n, hw, c, act, res_in, period=None, post=None):
    """ESDB's merged BSConvU over 48 input channels (BSRN._merged_bsconv: dense 3x3 weights + the border table of the pointwise bias) with its
    fp64 restatement as the BSConvU itself: the pointwise conv, then the depthwise 3x3 over the ZERO-PADDED pointwise output -- the dense conv
    with the blob's effective weights plus dw(pad0(bp)) + bd, the bias image derived without the table, as
    tests/test_gpu_bsrn.py::test_bsconv_as_dense3x3_with_border_table --, then + x, then the activation.  c = 24: c4 (conv48r_kernel<.., 2, true>);
    c = 48 with + x and GELU: c{j}_r (conv64m_kernel<.., 3, true>), `post` = (pc, act) adds the next distillation 1x1 (fp16)."""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.bsrn import BSRN
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    cin = 48
    g = torch.Generator().manual_seed(n + c + hw[0] + 31 * hw[1] + act)
    pw, dw = torch.nn.Linear(cin, c), torch.nn.Conv2d(c, c, 3, padding=1, groups=c)
    with torch.no_grad():
        pw.weight.copy_(torch.randn(c, cin, generator=g) * 0.2); pw.bias.copy_(torch.randn(c, generator=g))
        dw.weight.copy_(torch.randn(c, 1, 3, 3, generator=g) * 0.3); dw.bias.copy_(torch.randn(c, generator=g))
    w, bias, table = BSRN._merged_bsconv(pw, dw)
    blob = pack_conv_s16(w, bias, compute, cin_phys=cin)
    weff, _ = unpack_conv_s16(blob, cin, c, 3, compute, cin_phys=cin)
    xb = torch.randn(period or n, cin, *hw, generator=g).to(dt)
    bp = pw.bias.detach().double().reshape(1, c, 1, 1).expand(1, c, *hw)
    bias_img = F.conv2d(bp, dw.weight.detach().double(), dw.bias.detach().double(), padding=1, groups=c)      # dw(pad0(bp)) + bd
    conv = F.conv2d(xb.double().to(DEV), weff.double().to(DEV), None, padding=1) + bias_img.to(DEV)
    if res_in:
        conv = conv + xb.double().to(DEV)[:, :c]
    ref = _rep(ACTS[act](conv), n, period)
    xin = _rep(_nhwc(xb).to(DEV), n, period)
    kw = dict(act=act, cin=cin, packed=blob.to(DEV), border=table.to(DEV))
    if res_in:
        kw.update(res=xin, res_mode=L.RES_PRE_ACT)
    if post:
        wp, bpost = torch.randn(post[0], c, generator=g) * 0.2, torch.randn(post[0], generator=g)
        kw.update(post_weight=wp, post_bias=bpost, post_act=post[1])

    def launch(lo, hi):
        kw1 = dict(kw)
        if res_in:
            kw1["res"] = xin[lo:hi]
        with ops.kernel_trace() as names:
            out = ops.conv2d(xin[lo:hi].contiguous() if (lo, hi) != (0, n) else xin, w, bias, **kw1)
        return list(out) if post else [out], names

    outs, names = launch(0, n)
    refs, pads = [ref], [c]
    if post:
        # the 1x1 reads the ROUNDED activations (fp16: the stored y) and the weights' high parts, as test_esdb_r_on_conv64m_matches_fp64_reference
        got = outs[0].double().permute(0, 3, 1, 2)[:, :c]
        refs.append(ACTS[post[1]](torch.einsum("oc,nchw->nohw", wp.to(dt).double().to(DEV), got) + bpost.double().to(DEV)[None, :, None, None]))
        pads.append(post[0])
    return Case(names, outs, refs, launch, pads=pads)


def rlfb_post(compute, n, hw, mf, nf, f, seed, period=None):
    """RLFB's tail in one launch: u = lrelu(c3_r(x)) + r (never stored), v = c5(u), c1 = esa.conv1(v): conv48rp_kernel<.., false> from 256 tiles
    of 16 x 16 (tests/test_gpu_h16.py::test_s16_post_chain_rlfb, ::test_conv48rp_equals_conv_s16: the same inputs under two seeds)"""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(seed)
    xb = torch.randn(period or n, mf, *hw, generator=g).to(dt)
    rb = torch.randn(period or n, nf, *hw, generator=g).to(dt)
    w, b = torch.randn(nf, mf, 3, 3, generator=g) * 0.1, torch.randn(nf, generator=g)
    w5, b5 = torch.randn(nf, nf, generator=g) * 0.2, torch.randn(nf, generator=g)
    w1, b1 = torch.randn(f, nf, generator=g) * 0.2, torch.randn(f, generator=g)
    weff, _ = unpack_conv_s16(pack_conv_s16(w, b, compute), mf, nf, 3, compute)
    u = F.leaky_relu(F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=1), 0.05) + rb.double().to(DEV)
    # bf16: hi + lo operands (the chain sees ~fp32 values and weights); fp16: the 11-bit high parts only -- operands of the
    # chain's MFMAs are the fp16 roundings of the fp32 tile and of the weights (the network's own storage precision)
    q = (lambda t: t) if compute == "bf16" else (lambda t: t.to(torch.float16).double())
    v = F.conv2d(q(u), q(w5.double().to(DEV))[:, :, None, None], b5.double().to(DEV))
    c1 = F.conv2d(q(v), q(w1.double().to(DEV))[:, :, None, None], b1.double().to(DEV))
    x = _rep(F.pad(_nhwc(xb), (0, 48 - mf)).to(DEV), n, period)
    r = _rep(F.pad(_nhwc(rb), (0, 48 - nf)).to(DEV), n, period)
    kw = dict(act=1, res_mode=2, post_weight=w5, post_bias=b5, post2_weight=w1, post2_bias=b1, store_main=False, cin=mf)

    def chunk(lo, hi):
        with ops.kernel_trace() as names:
            y1, v1, c11 = ops.conv2d(x[lo:hi].contiguous(), w, b, res=r[lo:hi].contiguous(), **kw)
        assert y1 is None
        return [v1, c11], names

    with ops.kernel_trace() as names:
        y, yv, yc = ops.conv2d(x, w, b, res=r, **kw)
    return Case(names, [yv, yc], [_rep(v, n, period), _rep(c1, n, period)], chunk, pads=[nf, f], main=y)


def lr_hilo(n, c, hw, act, cp, period=None):
    """the LR conv behind the long skip on hi + lo pairs (bf16): conv(x) + (r_hi + r_lo), a pair out -- conv48rp_kernel<true, true> (cp = 48) /
    conv64m_kernel<true, false, true, 4, false> (cp = 64) from 256 tiles of 16 x 16 (tests/test_gpu_h16.py::test_conv48rl_equals_conv_s16,
    tests/test_gpu_c64m.py::test_conv64m_hilo_lr_conv_matches_fp64_reference)"""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(n * 100 + c + hw[0])
    xb = torch.randn(period or n, c, *hw, generator=g).to(torch.bfloat16)
    r32 = torch.randn(period or n, c, *hw, generator=g) * 3.0
    w = torch.randn(c, c, 3, 3, generator=g) * 0.1
    b = torch.randn(c, generator=g)
    blob = pack_conv_s16(w, b, "bf16", cin_phys=cp).to(DEV)
    weff, _ = unpack_conv_s16(blob.cpu(), c, c, 3, "bf16", cin_phys=cp)
    xin = _rep(F.pad(_nhwc(xb), (0, cp - c)).to(DEV), n, period)
    rinb = _hilo(r32, cp).to(DEV)
    rin = _rep(rinb, n, period, axis=1)
    kw = dict(cin=c, packed=blob, act=act, res_mode=L.RES_PRE_ACT, hilo=L.HILO_RES | L.HILO_OUT)

    def chunk(lo, hi):
        with ops.kernel_trace() as names:
            y1 = ops.conv2d(xin[lo:hi].contiguous(), w, b, res=rin[:, lo:hi].contiguous(), **kw)
        return [y1], names

    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w, b, res=rin, **kw)
    rsum = (rinb[0].double() + rinb[1].double()).permute(0, 3, 1, 2)[:, :c]
    ref = ACTS[act](F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=1) + rsum)
    return Case(names, [y], [_rep(ref, n, period)], chunk, pair=True, pads=[c], rin=rin)


def conv48rq(hw, n, border, act, pact, c, pc, period=None):
    """fp16: a 48 -> 48 3x3 + input (+ a random border table) whose stored result feeds one post 1x1 of two output tiles -- conv48rq_kernel from
    256 tiles of 16 x 16 (tests/test_gpu_h16.py::test_conv48rq_equals_conv_s16).  The fp64 side (for the forms without a table): the conv with the
    blob's effective weights + x, activated; the 1x1 on the STORED y with the fp16 roundings of its weights, as the fp16 post forms of
    tests/test_gpu_c64m.py."""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    g = torch.Generator().manual_seed(n * 10 + hw[0])
    xb = F.pad(torch.randn(period or n, *hw, c, generator=g), (0, 48 - c)).to(torch.float16).to(DEV)
    x = _rep(xb, n, period)
    w, b = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g)
    wp, bp = torch.randn(pc, c, generator=g) * 0.2, torch.randn(pc, generator=g)
    table = None
    if border:
        table = torch.randn(16, 48, generator=g) * 0.2
        table[0] = 0
        table[:, c:] = 0
        table = table.to(DEV)
    blob = pack_conv_s16(w, b, "f16").to(DEV)
    kw = dict(act=act, packed=blob, border=table, res_mode=L.RES_PRE_ACT, post_weight=wp, post_bias=bp, post_act=pact, cin=c)

    def chunk(lo, hi):
        xi = x[lo:hi].contiguous()
        with ops.kernel_trace() as names:
            y1, p1 = ops.conv2d(xi, w, b, res=xi, **kw)
        return [y1, p1], names

    with ops.kernel_trace() as names:
        y, yp = ops.conv2d(x, w, b, res=x, **kw)
    refs = [None, None]
    if not border:
        weff, _ = unpack_conv_s16(blob.cpu(), c, c, 3, "f16")
        xd = xb[..., :c].permute(0, 3, 1, 2).double()
        refs[0] = _rep(ACTS[act](F.conv2d(xd, weff.double().to(DEV), b.double().to(DEV), padding=1) + xd), n, period)
        got = y.double().permute(0, 3, 1, 2)[:, :c]
        refs[1] = ACTS[pact](torch.einsum("oc,nchw->nohw", wp.to(torch.float16).double().to(DEV), got) + bp.double().to(DEV)[None, :, None, None])
    return Case(names, [y, yp], refs, chunk, pads=[c, pc], x=x, blob=blob)


def conv64(compute, n, hw, cin, cout, act, res_in, period=None):
    """3x3 over 64 physical input channels, plain or + input: two output tiles conv64r_kernel, four conv64m_kernel<.., 4, false>, from 256 tiles
    of 16 x 16 (tests/test_gpu_h16.py::test_conv64r_equals_conv_s16)"""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(cin + cout + act + hw[0] + n)
    cp = 64
    xb = torch.randn(period or n, cin, *hw, generator=g).to(dt)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    blob = pack_conv_s16(w, b, compute, cin_phys=cp).to(DEV)
    xin = _rep(F.pad(_nhwc(xb), (0, cp - cin)).to(DEV), n, period)
    kw = dict(act=act, cin=cin, packed=blob)
    if res_in:
        kw.update(res=xin, res_mode=L.RES_PRE_ACT)

    def chunk(lo, hi):
        kw1 = dict(kw)
        if res_in:
            kw1["res"] = xin[lo:hi]
        with ops.kernel_trace() as names:
            y1 = ops.conv2d(xin[lo:hi].contiguous(), w, b, **kw1)
        return [y1], names

    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w, b, **kw)
    weff, _ = unpack_conv_s16(blob.cpu(), cin, cout, 3, compute, cin_phys=cp)
    conv = F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=1)
    if res_in:
        conv = conv + xb.double().to(DEV)[:, :cout]
    return Case(names, [y], [_rep(ACTS[act](conv), n, period)], chunk, pads=[cout])


def conv64m(compute, n, c, hw, res_in, seed, pc=None, period=None):
    """conv64m_kernel<.., 4, false>: lrelu(conv3x3(x) [+ x]) over 64 physical channels, plain or (pc) with the next distillation 1x1 + LeakyReLU in
    its epilogue (tests/test_gpu_c64m.py::test_conv64m_plain_matches_fp64_reference, ::test_conv64m_post_matches_fp64_reference)"""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(seed)
    xb = F.pad(torch.randn(period or n, *hw, c, generator=g), (0, 64 - c)).to(dt).to(DEV)
    x = _rep(xb, n, period)
    w, b = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g)
    if pc:
        wp, bp = torch.randn(pc, c, generator=g) * 0.2, torch.randn(pc, generator=g)
    blob = pack_conv_s16(w, b, compute, cin_phys=64)
    weff, _ = unpack_conv_s16(blob, c, c, 3, compute, cin_phys=64)
    xd = xb[..., :c].permute(0, 3, 1, 2).double()
    conv = F.conv2d(xd, weff.double().to(DEV), b.double().to(DEV), padding=1)
    ref = _rep(F.leaky_relu(conv + xd if res_in else conv, 0.05), n, period)
    kw = dict(act=1, cin=c, packed=blob.to(DEV))
    if pc:
        kw.update(post_weight=wp, post_bias=bp, post_act=1)
    if res_in:
        kw.update(res=x, res_mode=L.RES_PRE_ACT)

    def post_ref(got):
        """the post 1x1 + LeakyReLU.  bf16: it sees the fp32 activations as hi + lo (16 mantissa bits) and hi + lo weights; fp16: the rounded
        activations (the stored y) and the weights' high parts"""
        pin, pwt = (ref, wp.double().to(DEV)) if compute == "bf16" else (got, wp.to(dt).double().to(DEV))
        return F.leaky_relu(torch.einsum("oc,nchw->nohw", pwt, pin) + bp.double().to(DEV)[None, :, None, None], 0.05)

    def launch():
        with ops.kernel_trace() as names:
            out = ops.conv2d(x, w, b, **kw)
        return (list(out) if pc else [out]), names

    outs, names = launch()
    case = Case(names, outs, [ref], None, pads=[c] + ([pc] if pc else []), launch=launch, post_ref=post_ref)
    if pc:
        case.refs.append(post_ref(case.got(0)))
    return case


def esdb_r(compute, post, n, c, hw, pc, period=None):
    """conv64m_kernel<.., 3, true>: gelu(dense 3x3(x) + a RANDOM table's row + x) over 48 physical channels, plain or (fp16) with the next
    distillation Linear + GELU (tests/test_gpu_c64m.py::test_esdb_r_on_conv64m_matches_fp64_reference)"""
    from ntire2022_esr_amd import ops, _lib as L
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(n + c + hw[0] + post)
    xb = F.pad(torch.randn(period or n, *hw, c, generator=g), (0, 48 - c)).to(dt).to(DEV)
    x = _rep(xb, n, period)
    w, b = torch.randn(c, c, 3, 3, generator=g) * 0.1, torch.randn(c, generator=g)
    wp, bp = torch.randn(pc, c, generator=g) * 0.2, torch.randn(pc, generator=g)
    table = torch.randn(16, 48, generator=g) * 0.2
    table[0] = 0
    table[:, c:] = 0
    table = table.to(DEV)
    blob = pack_conv_s16(w, b, compute, cin_phys=48)
    weff, _ = unpack_conv_s16(blob, c, c, 3, compute, cin_phys=48)
    kw = dict(act=L.ACT_GELU, cin=c, packed=blob.to(DEV), border=table, res=x, res_mode=L.RES_PRE_ACT)
    if post:
        kw.update(post_weight=wp, post_bias=bp, post_act=L.ACT_GELU)
    xd = xb[..., :c].permute(0, 3, 1, 2).double()
    pre = F.conv2d(xd, weff.double().to(DEV), b.double().to(DEV), padding=1) + table.double()[border_mask(hw)][..., :c].permute(2, 0, 1)[None] + xd
    ref = _rep(F.gelu(pre), n, period)

    def post_ref(got):
        return F.gelu(torch.einsum("oc,nchw->nohw", wp.to(dt).double().to(DEV), got) + bp.double().to(DEV)[None, :, None, None])

    def launch():
        with ops.kernel_trace() as names:
            out = ops.conv2d(x, w, b, **kw)
        return (list(out) if post else [out]), names

    outs, names = launch()
    case = Case(names, outs, [ref], None, pads=[c] + ([pc] if post else []), launch=launch, post_ref=post_ref)
    if post:
        case.refs.append(post_ref(case.got(0)))
    return case


def block_tail(compute, n, hw, C, dc, f, esdb, period=None):
    """rfdb_tail_kernel: r4 = round(act(c4(r3))) (never stored), v = c5 . [d1 d2 d3 r4], c1 = conv1 . v in one launch, from 256 tiles of 16 x 16.
    RFDB form (esdb False): c4 a 3x3 over 64 physical channels, LeakyReLU (tests/test_gpu_c64m.py::test_rfdb_tail_matches_fp64_reference); ESDB
    form: c4 the merged BSConvU over 48 with its border table and GELU (::test_esdb_tail_matches_fp64_reference).  outs / refs: v, c1; extra
    "slack": the absolute terms of the two bounds; names None: esr_conv_tail_supported refused the descriptor (extra d, st for the caller)."""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.bsrn import BSRN
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16, pack_tail_s16, pack_post_s16
    dt = DT[compute]
    cp = 48 if esdb else 64
    g = torch.Generator().manual_seed(n + hw[0] + C)
    table = None
    if esdb:
        pw, dw = torch.nn.Linear(C, dc), torch.nn.Conv2d(dc, dc, 3, padding=1, groups=dc)
        with torch.no_grad():
            pw.weight.copy_(torch.randn(dc, C, generator=g) * 0.2); pw.bias.copy_(torch.randn(dc, generator=g))
            dw.weight.copy_(torch.randn(dc, 1, 3, 3, generator=g) * 0.4); dw.bias.copy_(torch.randn(dc, generator=g) * 0.3)
        w4, b4, table = BSRN._merged_bsconv(pw, dw)
    m = period or n
    r3b = F.pad(torch.randn(m, *hw, C, generator=g), (0, cp - C)).to(dt).to(DEV)
    dsb = F.pad(torch.randn(3, m, *hw, dc, generator=g), (0, 32 - dc)).to(dt).to(DEV)
    if not esdb:
        w4, b4 = torch.randn(dc, C, 3, 3, generator=g) * 0.1, torch.randn(dc, generator=g)
    w5, b5 = torch.randn(C, 4 * dc, generator=g) * 0.15, torch.randn(C, generator=g)
    wc, bc = torch.randn(f, C, generator=g) * 0.2, torch.randn(f, generator=g)
    blob4 = pack_conv_s16(w4, b4, compute, cin_phys=cp)
    w4e, _ = unpack_conv_s16(blob4, C, dc, 3, compute, cin_phys=cp)
    blob5 = pack_tail_s16(w5, b5, 3, dc, dc, compute).to(DEV)
    blobc = pack_post_s16(wc, bc, compute).to(DEV)
    blob4 = blob4.to(DEV)
    tab = table.to(DEV) if esdb else None
    assert tab is None or tuple(tab.shape) == (16, 32)
    r3, ds = _rep(r3b, n, period), _rep(dsb, n, period, axis=1)
    v = torch.full((n, *hw, cp), 7.0, dtype=dt, device=DEV)
    c1 = torch.full((n, *hw, 16), 7.0, dtype=dt, device=DEV)
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], C, dc, 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = d.compute = L.STORE[compute]
    d.act, d.slope = L.ACT_NONE, 0.05
    d.inp = L.View(ctypes.c_void_p(r3.data_ptr()), cp, 0)
    d.out0 = L.View(ctypes.c_void_p(v.data_ptr()), cp, 0)
    d.wpacked = ctypes.c_void_p(blob4.data_ptr())
    if esdb:
        d.border_bias = ctypes.c_void_p(tab.data_ptr())
    d.tail_wpacked = ctypes.c_void_p(blob5.data_ptr())
    d.tail_cat = L.View(ctypes.c_void_p(ds.data_ptr()), 32, 0)
    d.tail_cat_c, d.tail_cout, d.tail_mid_act = 96, C, L.ACT_GELU if esdb else L.ACT_LRELU
    d.tail_seg_stride16 = ds[0].numel() * 2 // 16
    d.post_wpacked = ctypes.c_void_p(blobc.data_ptr())
    d.post_out = L.View(ctypes.c_void_p(c1.data_ptr()), 16, 0)
    d.post_cout, d.post_act = f, L.ACT_NONE
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    keep = (r3, ds, blob4, blob5, blobc, tab)
    if not L.lib().esr_conv_tail_supported(ctypes.byref(d)):
        return Case(None, [v, c1], [None, None], None, d=d, st=st, keep=keep)
    # fp64 reference (ESDB: the dense 3x3 + the table row of the pixel's outside sides, exact GELU)
    x = r3b[..., :C].permute(0, 3, 1, 2).double()
    pre = F.conv2d(x, w4e.double().to(DEV), b4.double().to(DEV), padding=1)
    if esdb:
        pre = pre + tab.double()[border_mask(hw)][..., :dc].permute(2, 0, 1)[None]
    r4 = F.gelu(pre) if esdb else F.leaky_relu(pre, 0.05)
    r4q = r4.to(dt).double()                                                       # the tensor the separate launches store
    cat = torch.cat([dsb[j, ..., :dc].permute(0, 3, 1, 2).double() for j in range(3)] + [r4q], 1)
    vref = _rep(torch.einsum("oc,nchw->nohw", _hilo_w(w5, dt).to(DEV), cat) + b5.double().to(DEV)[None, :, None, None], n, period)
    step = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    if esdb:
        # a flipped rounding of r4 / the polynomial's error (1.3e-4 on [-4, 4], 2.13e-4 below: these pre-activations stay inside) move v by |w5| x that much
        extra = float(w5.abs().max()) * (1.2 * step * float(r4.abs().max()) + 4 * 1.3e-4)
    else:
        # r4 sits on rounding boundaries now and then: a flipped r4 value moves v by |w5| x one step of r4
        extra = 1.2 * float(w5.abs().max()) * step * float(r4.abs().max())
    slack = [extra, 2e-4 + extra * float(wc.abs().max()) * 8]

    def launch():
        with ops.kernel_trace() as names:
            ops._launch(L.OP_CONV, d, st.value, "tail")
        torch.cuda.synchronize()
        return names

    def c1_ref(got):
        """bf16: conv1 sees v's fp32 value and hi + lo weights; fp16: the stored v and the weights' high parts"""
        wq = _hilo_w(wc, dt) if compute == "bf16" else wc.to(dt).double()
        return torch.einsum("oc,nchw->nohw", wq.to(DEV), vref if compute == "bf16" else got) + bc.double().to(DEV)[None, :, None, None]

    names = launch()
    case = Case(names, [v, c1], [vref], None, pads=[C, f], launch=launch, c1_ref=c1_ref, slack=slack, keep=keep, d=d, st=st)
    case.refs.append(c1_ref(case.got(0)))
    return case


def s16_conv(compute, cin, cout, k, hw, act, res_mode, tight, n=2, period=None):
    """the 16-bit storage conv on conv_s16_kernel, every epilogue family (tests/test_gpu_h16.py::test_s16_conv_matches_fp64_reference); a plain
    48 -> 48 3x3 from 512 tiles of 16 x 16 is its 4-wave shape (s16_four_waves)"""
    from ntire2022_esr_amd import ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    dt = DT[compute]
    g = torch.Generator().manual_seed(cin + cout + hw[0] + k)
    cp = (cin + 15) // 16 * 16
    xb = torch.randn(period or n, cin, *hw, generator=g).to(dt)
    rb = torch.randn(period or n, cout, *hw, generator=g).to(dt)
    w = torch.randn(cout, cin, k, k, generator=g) * (0.1 if k == 3 else 0.2)
    b = torch.randn(cout, generator=g)
    blob = pack_conv_s16(w, b, compute, cin_phys=cp)
    weff, _ = unpack_conv_s16(blob, cin, cout, k, compute, cin_phys=cp)
    conv = F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=k // 2)
    rd = rb.double().to(DEV)
    ref = ACTS[act](conv + rd) if res_mode == 1 else (ACTS[act](conv) + rd if res_mode == 2 else ACTS[act](conv))
    xin = _rep(F.pad(_nhwc(xb), (0, ((cin + 7) // 8 * 8 if tight else cp) - cin)).to(DEV), n, period)
    rp = _rep(F.pad(_nhwc(rb), (0, (-cout) % 8)).to(DEV), n, period) if res_mode else None
    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w, b, act=act, res=rp, res_mode=res_mode, cin=cin, packed=blob.to(DEV))
    return Case(names, [y], [_rep(ref, n, period)], None, pads=[cout])


def hilo_head(n, cin, cout, hw, period=None, g=None):
    """the head of a bf16 network's long skip: y = conv(x16) stored as a hi + lo pair whose high parts ARE the plain kernel's output
    (tests/test_gpu_h16.py::test_s16_hilo_skip_convs, its first third; extra: what the rest of that test goes on with).  16 input slots and
    512 .. 4095 tiles of 16 x 16: conv_s16_kernel's 4-wave HILO shape."""
    from ntire2022_esr_amd import _lib as L, ops
    from ntire2022_esr_amd.engine import pack_conv_s16, unpack_conv_s16
    g = g or torch.Generator().manual_seed(n * 1000 + cin + hw[0])
    cp = (cin + 15) // 16 * 16
    xb = torch.randn(period or n, cin, *hw, generator=g).to(torch.bfloat16)
    r32 = torch.randn(n if period is None else period, cout, *hw, generator=g) * 3.0
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    blob = pack_conv_s16(w, b, "bf16", cin_phys=cp)
    weff, _ = unpack_conv_s16(blob, cin, cout, 3, "bf16", cin_phys=cp)
    xin = _rep(F.pad(_nhwc(xb), (0, cp - cin)).to(DEV), n, period)
    conv = F.conv2d(xb.double().to(DEV), weff.double().to(DEV), b.double().to(DEV), padding=1)
    plain = ops.conv2d(xin, w, b, cin=cin, packed=blob.to(DEV))
    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w, b, cin=cin, packed=blob.to(DEV), hilo=L.HILO_OUT)
    return Case(names, [y], [_rep(conv, n, period)], None, pair=True, pads=[cout], plain=plain, g=g, x=xb, r32=r32, w=w, b=b, blob=blob, xin=xin, conv=conv)


def _w8_on(on):
    from ntire2022_esr_amd import _lib as L
    L.lib().esr_dbg_wino8(ctypes.c_int(1 if on else 0))


def wino8(cin, cout, n, h, w, act, period=None, blocked_out1=False, blocked_in=False, seed=None):
    """Winograd F(2x2, 3x3) fp32 on wino8_f32_kernel (strips of 4 x 16, from 4096 strips at 33 .. 64 outputs, 8192 below) against the fp64
    convolution, and the same launch with the research switch off: wino_f32_kernel (tests/test_gpu_wino.py::test_wino8_plain; blocked_out1 /
    blocked_in: the 16 / 48 split store with a channel-blocked out1 and the channel-blocked input of ::test_wino8_split_and_blocked_stores,
    ::test_wino8_blocked_input, both outputs returned as NHWC)"""
    from ntire2022_esr_amd import ops
    g = torch.Generator().manual_seed(cin + cout + h if seed is None else seed)
    xb = torch.randn(period or n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)
    ref = _rep(ACTS[act](F.conv2d(xb.double().to(DEV), wt.double().to(DEV), b.double().to(DEV), padding=1)), n, period)
    if blocked_in:
        xd = _rep(xb.view(-1, cin // 8, 8, h, w).permute(0, 1, 3, 4, 2).contiguous().to(DEV), n, period)
    else:
        xd = _rep(_nhwc(xb).to(DEV), n, period)
        if cin % 8:
            xd = F.pad(xd, (0, 8 - cin % 8))

    def launch():
        kw = dict(act=act, cin=cin, wino=True, blocked_in=blocked_in)
        with ops.kernel_trace() as names:
            if blocked_out1:
                cat = torch.zeros((n, h, w, 16), device=DEV)
                remb = torch.full((n, (cout - 16) // 8, h, w, 8), 9.0, device=DEV)
                ops.conv2d(xd, wt, b, split=16, out=cat, out1=remb, blocked_out1=True, **kw)
                y = torch.cat([cat, remb.permute(0, 2, 3, 1, 4).reshape(n, h, w, cout - 16)], dim=-1)
            else:
                y = ops.conv2d(xd, wt, b, **kw)
        return y, names

    _w8_on(True)
    try:
        y8, names = launch()
        _w8_on(False)
        y4, names4 = launch()
    finally:
        _w8_on(True)
    return Case(names, [y8], [ref], None, pads=[None], general=(y4, names4), ref32=ACTS[act](F.conv2d(xb, wt, b, padding=1)) if period is None else None, x=xb, w=wt, b=b)


def conv_f32(n, hw, cin, cout, act, res_mode, period=None):
    """conv_f32_kernel, every epilogue family; 3x3 NHWC with >= 3 output tiles and >= 2 input chunks from 256 tiles of 16 x 32 takes the 8-wave
    shape (tests/test_gpu_conv.py::test_conv_8wave_tall_tiles)"""
    from ntire2022_esr_amd import ops
    g = torch.Generator().manual_seed(n * 7 + hw[0] + act + 3 * res_mode)
    xb = torch.randn(period or n, cin, *hw, generator=g)
    rb = torch.randn(period or n, cout, *hw, generator=g)
    w = torch.randn(cout, cin, 3, 3, generator=g) * 0.1
    b = torch.randn(cout, generator=g)

    def f(x, r, wt, bt):
        c = F.conv2d(x, wt, bt, padding=1)
        return {0: ACTS[act](c), 1: ACTS[act](c + r), 2: ACTS[act](c) + r}[res_mode]

    ref = _rep(f(xb.double().to(DEV), rb.double().to(DEV), w.double().to(DEV), b.double().to(DEV)), n, period)
    xin = _rep(_nhwc(xb).to(DEV), n, period)
    rin = _rep(_nhwc(rb).to(DEV), n, period) if res_mode else None

    def chunk(lo, hi):
        with ops.kernel_trace() as names:
            y1 = ops.conv2d(xin[lo:hi].contiguous(), w, b, act=act, slope=0.05, res=rin[lo:hi].contiguous() if res_mode else None, res_mode=res_mode)
        return [y1], names

    (y,), names = chunk(0, n)
    return Case(names, [y], [ref], chunk, pads=[None], ref32=f(xb, rb, w, b) if period is None else None)


def imdb_tail(n, hw, mid_act, res_mode, cat_c, period=None):
    """esr_conv_desc.tail_* in fp32: IMDBlock's conv4 -> cat -> conv1x1 -> + x in one launch; the concat part is a channel slice of a wider
    buffer.  cat_c = 48 with no / a pre-activation residual is the network's own shape: imdb_tail_kernel, always on 16 x 32 tiles with one
    8-wave block per CU (tests/test_gpu_conv.py::test_conv3x3_with_fused_1x1_tail)"""
    from ntire2022_esr_amd import ops
    g = torch.Generator().manual_seed(n + hw[0] + 5 * mid_act + res_mode + cat_c)
    m = period or n
    xb = torch.randn(m, 48, *hw, generator=g)
    catb = torch.randn(m, 64, *hw, generator=g)                   # channels [8, 8 + cat_c) are the 1x1's other inputs
    rb = torch.randn(m, 64, *hw, generator=g)
    w3 = torch.randn(16, 48, 3, 3, generator=g) * 0.1
    b3 = torch.randn(16, generator=g)
    w1 = torch.randn(64, cat_c + 16, 1, 1, generator=g) * 0.1
    b1 = torch.randn(64, generator=g)

    def f(x, cat, r, cv):
        c4 = ACTS[mid_act](F.conv2d(x, cv(w3), cv(b3), padding=1))
        y1 = F.conv2d(torch.cat([cat[:, 8:8 + cat_c], c4], 1), cv(w1), cv(b1))
        return {0: y1, 1: y1 + r, 2: F.leaky_relu(y1, 0.05) + r}[res_mode]

    ref = _rep(f(xb.double().to(DEV), catb.double().to(DEV), rb.double().to(DEV), lambda t: t.double().to(DEV)), n, period)
    xin, cin_, rin = (_rep(_nhwc(t).to(DEV), n, period) for t in (xb, catb, rb))
    with ops.kernel_trace() as names:
        y = ops.conv2d(xin, w3, b3, act=1 if res_mode == 2 else 0, slope=0.05, res=rin if res_mode else None, res_mode=res_mode,
                       tail_weight=w1, tail_bias=b1, tail_cat=cin_, tail_cat_coff=8, tail_mid_act=mid_act)
    return Case(names, [y], [ref], None, pads=[None], ref32=f(xb, catb, rb, lambda t: t) if period is None else None)


# ---- the thin-batch table ------------------------------------------------------------------------------------------------------------------
# unit / threshold: the tile count the dispatch code tests (s16_select, s16_four_waves: csrc/esr_s16.hip; conv_block_waves: csrc/esr_hip.hip;
# esr_conv2d_wino's `nstrips >= 4 * 8 * W8_MAX_BLOCKS / nhalves`: csrc/esr_wino.hip).  tests/test_thin_batch_table.py asks the library's own
# shape query whether the batch is above it and every chunk below, so a wrong number here fails without a GPU.
#   waves    esr_conv_block_waves' answer for the batch (None: the query does not know the kernel -- the Winograd kernels)
#   chunks   check 4: the batch again as this many consecutive chunks on the general kernel, bit-identical (0: another accumulation order)
#   bound    per output: (relative, absolute) -- |got - ref| <= |ref| * relative * eps(storage) + absolute * max(1, max|ref|), or a callable
def _f(**kw):
    return kw


EPS = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


def _plain_bound(gelu=False):
    return lambda compute, ref: ref.abs() * EPS[compute] * 1.01 + (3e-4 if gelu else 5e-5) * max(1.0, float(ref.abs().max()))


def _hilo_bound(compute, ref):
    return ref.abs() * 2.0 ** -15 + 3e-5 * max(1.0, float(ref.abs().max()))


def _c64m_bound(extra=0.0):
    return lambda compute, ref: ref.abs() * EPS[compute] * 1.01 + 3e-5 * max(1.0, float(ref.abs().max())) + extra


def _rlfb_bound(compute, ref):
    # test_s16_post_chain_rlfb's `close` (its small-image branch: every case here is far below 1e6 outputs)
    return ref.abs() * EPS[compute] * 1.01 + (1e-3 * 32 if compute == "bf16" else 0.5) * EPS[compute] * max(1.0, float(ref.abs().max()))


def _f32_bound(compute, ref):
    return torch.full_like(ref, 2e-5 * max(1.0, float(ref.abs().max())))


_TF = {"bf16": "true", "f16": "false"}

FORMS = [
    # conv48r_kernel: C48R16 (256 <= t32 < 1024, 4 rows per wave on 16 x 16 tiles) and C48R32 (t32 >= 1024, 8 rows per wave)
    *[_f(id=f"conv48r-{nm}-rw{rw}", storages=("bf16", "f16"), unit="t32", threshold=256 if rw == 4 else 1024, chunks=2 if rw == 4 else 5, waves=1,
         run=(lambda compute, n, hw, period, a=args: conv48r(compute, n, hw, *a, period=period)),
         kernel=(lambda compute, nt=nt, ext=ext, rw=rw: f"conv48r_kernel<{_TF[compute]}, {nt}, {ext}, {rw},"), general="conv_s16_kernel<",
         bounds=[_plain_bound(args[2] == 3)], desc=dict(cin=48, cout=args[1], act=args[2], res_in=args[3]))
      for rw in (4, 8) for nm, args, nt, ext in [("plain", (48, 48, 1, False, False), 3, "false"), ("resin", (48, 48, 0, True, False), 3, "true"),
                                                 ("two", (48, 24, 1, False, False), 2, "true")]],
    # ... with the merged BSConvU's border table: ESDB's c4 (two output tiles, GELU, no residual)
    *[_f(id=f"conv48r-bsconv-c4-rw{rw}", storages=("bf16", "f16"), unit="t32", threshold=256 if rw == 4 else 1024, chunks=2 if rw == 4 else 5, waves=1,
         run=(lambda compute, n, hw, period: bsconv48(compute, n, hw, 24, 3, False, period=period)),
         kernel=(lambda compute, rw=rw: f"conv48r_kernel<{_TF[compute]}, 2, true, {rw},"), general="conv_s16_kernel<",
         bounds=[_plain_bound(True)], desc=dict(cin=48, cout=24, act=3, border=True)) for rw in (4, 8)],
    _f(id="conv48rp", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=2, waves=1,
       run=(lambda compute, n, hw, period: rlfb_post(compute, n, hw, 48, 46, 16, 21 + n + hw[0], period=period)),
       kernel=(lambda compute: f"conv48rp_kernel<{_TF[compute]}, false>"), general="conv_s16_kernel<",
       bounds=[_rlfb_bound, _rlfb_bound], desc=dict(cin=48, cout=46, act=1, c3r=True)),
    _f(id="conv48rl", storages=("bf16",), unit="t16", threshold=256, chunks=2, waves=1,
       run=(lambda compute, n, hw, period: lr_hilo(n, 46, hw, 0, 48, period=period)),
       kernel=(lambda compute: "conv48rp_kernel<true, true>"), general="conv_s16_kernel<",
       bounds=[_hilo_bound], desc=dict(cin=46, cout=46, act=0, lr=48)),
    _f(id="conv64m-hilo", storages=("bf16",), unit="t16", threshold=256, chunks=0, waves=1,
       run=(lambda compute, n, hw, period: lr_hilo(n, 50, hw, 0, 64, period=period)),
       kernel=(lambda compute: "conv64m_kernel<true, false, true, 4, false>"), general=None,
       bounds=[_hilo_bound], desc=dict(cin=50, cout=50, act=0, lr=64)),
    # conv48rq_kernel: fp16 only; GELU on the conv and on the post 1x1 (no table: with one the batch runs on conv64m_kernel<.., 3, true>, below)
    _f(id="conv48rq", storages=("f16",), unit="t16", threshold=256, chunks=2, waves=1,
       run=(lambda compute, n, hw, period: conv48rq(hw, n, False, 3, 3, 48, 24, period=period)),
       kernel=(lambda compute: "conv48rq_kernel<false,"), general="conv_s16_kernel<",
       # y: the plain bound with a 16-bit GELU; the 1x1 + GELU on the stored y: the bound of the fp16 GELU post form of test_esdb_r_on_conv64m_matches_fp64_reference
       bounds=[_plain_bound(True), _c64m_bound(4e-4)], desc=dict(cin=48, cout=48, act=3, res_in=True, post=24, post_act=3)),
    _f(id="conv64r", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=2, waves=1,
       run=(lambda compute, n, hw, period: conv64(compute, n, hw, 50, 25, 1, False, period=period)),
       kernel=(lambda compute: f"conv64r_kernel<{_TF[compute]}, 2,"), general="conv_s16_kernel<",
       bounds=[_plain_bound()], desc=dict(cin=50, cout=25, act=1)),
    _f(id="conv64m-plain", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=0, waves=1,
       run=(lambda compute, n, hw, period: conv64m(compute, n, 50, hw, True, n + 50 + hw[0], period=period)),
       kernel=(lambda compute: f"conv64m_kernel<{_TF[compute]}, false, false, 4, false>"), general=None,
       bounds=[_c64m_bound()], desc=dict(cin=50, cout=50, act=1, res_in=True)),
    _f(id="conv64m-post", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=0, waves=1,
       run=(lambda compute, n, hw, period: conv64m(compute, n, 50, hw, True, n * 10 + hw[0] + 50, pc=25, period=period)),
       kernel=(lambda compute: f"conv64m_kernel<{_TF[compute]}, true, false, 4, false>"), general=None,
       bounds=[_c64m_bound(), _c64m_bound(2e-4)], desc=dict(cin=50, cout=50, act=1, res_in=True, post=25, post_act=1)),
    # ESDB's c{j}_r as the merged BSConvU, against the fp64 BSConvU: the only reference that gives table rows 3, 7, 11 .. 15 a meaning
    _f(id="conv64m-esdb", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=0, waves=1,
       run=(lambda compute, n, hw, period: bsconv48(compute, n, hw, 48, 3, True, period=period)),
       kernel=(lambda compute: f"conv64m_kernel<{_TF[compute]}, false, false, 3, true>"), general=None,
       bounds=[_c64m_bound(2.6e-4)], desc=dict(cin=48, cout=48, act=3, res_in=True, border=True)),
    _f(id="conv64m-esdb-post", storages=("f16",), unit="t16", threshold=256, chunks=0, waves=1,
       run=(lambda compute, n, hw, period: bsconv48(compute, n, hw, 48, 3, True, period=period, post=(24, 3))),
       kernel=(lambda compute: "conv64m_kernel<false, true, false, 3, true>"), general=None,
       bounds=[_c64m_bound(2.6e-4), _c64m_bound(4e-4)], desc=dict(cin=48, cout=48, act=3, res_in=True, border=True, post=24, post_act=3)),
    # conv_s16_kernel's 4-wave shapes: the plain 48 -> 48 3x3 from 512 tiles of 16 x 16; the hi + lo head over 16 input slots, 512 .. 4095 tiles
    _f(id="s16-4w", storages=("bf16", "f16"), unit="t16", threshold=512, chunks=0, waves=4,
       run=(lambda compute, n, hw, period: s16_conv(compute, 32, 48, 3, hw, 1, 0, False, n=n, period=period)),
       kernel=(lambda compute: f"conv_s16_kernel<3, 3, 4, {_TF[compute]}, false"), general=None,
       bounds=[_c64m_bound()], desc=dict(cin=32, cout=48, act=1)),          # (test_s16_conv_matches_fp64_reference's _ulp_ok: 3e-5)
    _f(id="hilo-4w", storages=("bf16",), unit="t16", threshold=512, chunks=0, waves=4,
       run=(lambda compute, n, hw, period: hilo_head(n, 9, 48, hw, period=period)),
       kernel=(lambda compute: "conv_s16_kernel<3, 3, 4, true, false, 0, 0, true"), general=None,
       bounds=[_hilo_bound], desc=dict(cin=9, cout=48, act=0, hilo_out=True)),
    # wino8_f32_kernel<ACT, OUT, NCH>: 4 and 6 input chunks; NHWC and blocked out1; NHWC and blocked input
    *[_f(id=f"wino8-{nm}", storages=("f32",), unit="strip", threshold=4096 if a[1] > 32 else 8192, chunks=-1, waves=None,
         run=(lambda compute, n, hw, period, a=a, kw=kw: wino8(a[0], a[1], n, hw[0], hw[1], a[2], period=period, **kw)),
         kernel=(lambda compute, k=k: k), general="wino_f32_kernel<", bounds=[_f32_bound], desc=None)
      for nm, a, kw, k in [("nch6", (48, 64, 1), {}, "wino8_f32_kernel<1, 0, 6>"), ("nch4", (32, 32, 3), {}, "wino8_f32_kernel<-1, 0, 4>"),
                           ("blocked-out1", (48, 64, 1), dict(blocked_out1=True), "wino8_f32_kernel<1, 1, 6>"),
                           ("blocked-in", (48, 64, 1), dict(blocked_out1=True, blocked_in=True), "wino8_f32_kernel<1, 1, 6>")]],
    # conv_f32_kernel's 8-wave shape on 16 x 32 tiles
    *[_f(id=f"conv-f32-tall-{act}{rm}", storages=("f32",), unit="t32", threshold=256, chunks=2, waves=8,
         run=(lambda compute, n, hw, period, act=act, rm=rm: conv_f32(n, hw, 48, 64, act, rm, period=period)),
         kernel=(lambda compute: "conv_f32_kernel<4, 3, false, 8, 0, 0, false>"), general="conv_f32_kernel<4, 3, false, 4, 0, 0, false>",
         bounds=[_f32_bound], desc=dict(cin=48, cout=64, act=act, res_hbm=rm)) for act, rm in [(1, 0), (0, 2), (1, 1)]],
    # imdb_tail_kernel: 16 x 32 tiles at every size (launch_conv_tail, csrc/esr_hip.hip); 256 of them = one per CU, more: the persistent walk
    *[_f(id=f"imdb-tail-{ma}{rm}", storages=("f32",), unit="t32", threshold=256, chunks=0, waves=None,
         run=(lambda compute, n, hw, period, ma=ma, rm=rm: imdb_tail(n, hw, ma, rm, 48, period=period)),
         kernel=(lambda compute, rm=rm: f"imdb_tail_kernel<{'true' if rm == 1 else 'false'}>"), general=None,
         bounds=[_f32_bound], desc=None) for ma, rm in [(0, 1), (1, 0)]],
    # rfdb_tail_kernel, RFDB and ESDB form (rfdb_tail_takes, csrc/esr_s16.hip: 256 tiles of 16 x 16; its query is esr_conv_tail_supported on
    # real views, which the launch itself asserts through the trace)
    *[_f(id=f"block-tail-{'esdb' if esdb else 'rfdb'}", storages=("bf16", "f16"), unit="t16", threshold=256, chunks=0, waves=None,
         run=(lambda compute, n, hw, period, a=a, esdb=esdb: block_tail(compute, n, hw, *a, esdb, period=period)),
         kernel=(lambda compute, esdb=esdb: f"rfdb_tail_kernel<{_TF[compute]}, {'3, true' if esdb else '4, false'}>"), general=None,
         bounds=[lambda compute, ref, case: _c64m_bound(case.extra["slack"][0])(compute, ref),
                 lambda compute, ref, case: _c64m_bound(case.extra["slack"][1])(compute, ref)], desc=None)
      for esdb, a in [(False, (50, 25, 16)), (True, (48, 24, 12))]],
]


def rows():
    """every (form, storage, shape) of the table with its batch size"""
    for form in FORMS:
        for compute in form["storages"]:
            for hw in SHAPES:
                yield form, compute, hw, batch_for(hw, form["unit"], form["threshold"])


def descriptor(form, compute, n, hw):
    """the form's descriptor for esr_conv_block_waves (host-only: the pointers are never read), as tests/test_abi_and_host.py builds it"""
    from ntire2022_esr_amd import _lib as L
    s = form["desc"]
    fake = lambda a: ctypes.c_void_p(a)
    d = L.ConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, hw[0], hw[1], s["cin"], s["cout"], 3
    d.in_layout = d.out_layout = L.NHWC
    d.storage = L.STORE[compute]
    d.compute = L.COMPUTE[compute] if compute != "f32" else 0
    d.act = s.get("act", 0)
    esz, pitch = (4, (s["cin"] + 7) // 8 * 8) if compute == "f32" else (2, (s["cin"] + 15) // 16 * 16)
    d.inp = L.View(fake(0x2000), pitch, 0)
    d.out0 = L.View(fake(0x5000), (s["cout"] + 7) // 8 * 8, 0)
    if s.get("res_in"):
        d.res_mode, d.res = L.RES_PRE_ACT, L.View(fake(0x2000), pitch, 0)
    if s.get("res_hbm"):
        d.res_mode, d.res = s["res_hbm"], L.View(fake(0x1000), (s["cout"] + 7) // 8 * 8, 0)
    if s.get("border"):
        d.border_bias = fake(0x6000)
    if s.get("post"):
        d.post_wpacked, d.post_cout, d.post_act = fake(0x3000), s["post"], s["post_act"]
    if s.get("c3r"):
        d.res_mode, d.res = L.RES_POST_ACT, L.View(fake(0x1000), 48, 0)
        d.post_wpacked, d.post2_wpacked, d.post_cout, d.post2_cout = fake(0x3000), fake(0x4000), 46, 16
        d.out0 = L.View(None, 0, 0)
    if s.get("lr"):
        d.res_mode, d.hilo, d.hilo_stride = L.RES_PRE_ACT, L.HILO_RES | L.HILO_OUT, 1 << 20
        d.res = L.View(fake(0x1000), s["lr"], 0)
    if s.get("hilo_out"):
        d.hilo, d.hilo_stride = L.HILO_OUT, 1 << 20
    return d
