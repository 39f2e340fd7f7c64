"""One fill per one-launch op: THE statement of which field of the C ABI's descriptor (include/esr_hip.h) carries which operand.

The engine's op classes (engine.py: from the ops a fused op replaces, into op.conv / op.chain / op.esa in place) and the single-op wrappers
(ops.py: from tensors) both call these, so a kernel's own tests and the networks run it under one convention; tests/test_launcher_table.py
holds every fill to the descriptors the tests build by hand.

A fill takes the zeroed descriptor `d`, nhw = (n, h, w), the storage code (L.STORE[...]) and, by keyword under their names in the kernel's
formula, the operands as L.View, the weight blobs as addresses and the channel counts as ints.  It writes every field the launcher reads
and nothing else; an operand that is None is left out.  What the two callers derive differently -- views, stored widths, which blob --
arrives as an argument; nothing here knows torch or a Plan."""
from . import _lib as L


def _conv(d, nhw, storage, compute, ksize, cin, cout):
    """the frame of an esr_conv_desc: shape, NHWC in and out, storage and operand type"""
    d.n, d.h, d.w = nhw
    d.cin, d.cout, d.ksize = cin, cout, ksize
    d.in_layout = d.out_layout = L.NHWC
    d.storage, d.compute = storage, compute


def _chain(d, nhw, storage, w, cin, cmid, cout, act, slope, res_mode, x):
    """the frame of an esr_chain_desc: shape, the layers' blobs `w` in order, 16-bit storage = operand type, the input view"""
    d.n, d.h, d.w = nhw
    d.n_layers, d.cin, d.cmid, d.cout = len(w), cin, cmid, cout
    d.act, d.slope, d.res_mode = act, slope, res_mode
    d.storage = d.compute = storage
    d.inp = x
    for i, blob in enumerate(w):
        d.wpacked[i] = blob


def chain(d, nhw, storage, *, x, w, cin, cmid, cout, act, slope, res_mode, post_w, v, v_width, post_act, post2_w, c1, c1_width):
    """esr_conv_chain_s16, RLFB form: t = x; t = act(conv_i(t)); u = act(conv_n(t)) + x (res_mode RES_POST_ACT); v = post_act(post_w . u);
    c1 = post2_w . v.  x -> inp, the 3x3 blobs w[i] -> wpacked[i] (cin -> cmid -> .. -> cout), v -> post_out (post_cout = v_width channels
    stored), c1 -> post2_out (post2_cout = c1_width)."""
    _chain(d, nhw, storage, w, cin, cmid, cout, act, slope, res_mode, x)
    d.post_wpacked, d.post_out, d.post_cout, d.post_act = post_w, v, v_width, post_act
    d.post2_wpacked, d.post2_out, d.post2_cout = post2_w, c1, c1_width


def hfab(d, nhw, storage, *, x, w, cin, cmid, cout, act, slope, y, y_width):
    """esr_conv_chain_s16, HFAB form (res_mode RES_GATE, no 1x1s): t = act(conv_i(t)) for the first three, y = sigmoid(conv_4(t)) * x.
    x -> inp, w[i] -> wpacked[i], y -> post_out (post_cout = y_width channels stored, the pad ones as zeros)."""
    _chain(d, nhw, storage, w, cin, cmid, cout, act, slope, L.RES_GATE, x)
    d.post_out, d.post_cout = y, y_width


def distill_step(d, nhw, storage, *, x, w_d, w_fold, cin, cmid, cout, res, dd, d_width, y, y_width):
    """esr_distill_step_s16: dd = relu(w_d . x), y = relu(w_fold (*) cat[x, dd] (+ x if res)).
    x -> inp (cin channels), w_d -> wpacked[0] (cmid outputs), w_fold (pack_distill_s16) -> wpacked[1] (cout outputs),
    dd -> post_out (post_cout = d_width), y -> post2_out (post2_cout = y_width)."""
    _chain(d, nhw, storage, (w_d, w_fold), cin, cmid, cout, L.ACT_RELU, 0.0, L.RES_PRE_ACT if res else L.RES_NONE, x)
    d.post_out, d.post_cout = dd, d_width
    d.post2_out, d.post2_cout = y, y_width


def refine_cascade(d, nhw, storage, *, d2, w, cin, cmid, cout, slope, d3, d3_width, r4, r4_width):
    """esr_refine_cascade_s16: r2 = lrelu(w[0] (*) d2 + d2), d3 = lrelu(w[1] . r2), r3 = lrelu(w[2] (*) d3 + d3), r4 = lrelu(w[3] (*) r3 + r3).
    d2 -> inp (cin channels), w[i] -> wpacked[i], d3 -> post_out (cmid channels, post_cout = d3_width stored),
    r4 -> post2_out (cout channels, post2_cout = r4_width)."""
    _chain(d, nhw, storage, w, cin, cmid, cout, L.ACT_LRELU, slope, L.RES_PRE_ACT, d2)
    d.post_out, d.post_cout = d3, d3_width
    d.post2_out, d.post2_cout = r4, r4_width


def cx_block(d, nhw, storage, *, v, w0, w1, w2, c, m, cout, slope, out, out_width):
    """esr_cx_block_s16: t = dw7(v, w0), h = lrelu(w1 . t), out = w2 . h + v.
    v -> inp (c channels), w0 (pack_dw7) / w1 / w2 (pack_cx_pw) -> wpacked[0..2], m -> cmid, out -> post_out (post_cout = out_width)."""
    _chain(d, nhw, storage, (w0, w1, w2), c, m, cout, L.ACT_LRELU, slope, L.RES_POST_ACT, v)
    d.post_out, d.post_cout = out, out_width


def dwpw_pair(d, nhw, storage, *, x, w, c, slope, out, out_width):
    """esr_dwpw_pair_s16: u1 = dw3(x, w[0]) + x, h = relu(w[1] . u1), u2 = dw3(h, w[2]) + h, out = lrelu(w[3] . u2 + x).
    x -> inp (cin = cmid = cout = c), w[i] -> wpacked[i] (pack_dw, pack_dwpw_pw, ..), out -> post_out (post_cout = out_width)."""
    _chain(d, nhw, storage, w, c, c, c, L.ACT_LRELU, slope, L.RES_PRE_ACT, x)
    d.post_out, d.post_cout = out, out_width


def resblock_head(d, nhw, storage, *, x, g=None, xs=None, w1, w2, wc, cin, cout, u, c1, c1_width):
    """esr_resblock_head_s16: xs = x + g (g given: res_mode RES_PRE_ACT; else xs = x, not stored), t = relu(w1 (*) xs), u = w2 (*) t, c1 = wc . u.
    x -> inp, g -> res, xs -> out0, u -> out1, c1 -> post_out (post_cout = c1_width); w1 -> wpacked, w2 -> tail_wpacked, wc -> post_wpacked."""
    _conv(d, nhw, storage, storage, 3, cin, cout)
    d.act, d.slope, d.res_mode = L.ACT_RELU, 0.0, (L.RES_NONE if g is None else L.RES_PRE_ACT)
    d.inp, d.out1 = x, u
    if g is not None:
        d.res, d.out0 = g, xs
    d.wpacked, d.tail_wpacked, d.post_wpacked = w1, w2, wc
    d.post_out, d.post_cout = c1, c1_width


def resdb_step(d, nhw, storage, *, x, extras=(), a, w_e, w_c, cin, cout, extra_channels, dists, dists_channels, y):
    """esr_resdb_step: u = prelu(cat(x, extras), a_e), e = w_e . u, dists = e[cout:], t = prelu(e[:cout], a_c), y = x + w_c (*) t.
    x -> inp (cin channels), the up to two extras -> res, tail_cat (tail_cat_c = extra_channels in all), a = pack_prelu(cat(a_e, a_c)) ->
    tail_wpacked, w_e (res rows, then distilled rows) -> post_wpacked, w_c -> wpacked, dists -> post_out (post_cout = dists_channels), y -> out0."""
    _conv(d, nhw, storage, storage, 3, cin, cout)
    d.post_cout, d.tail_cat_c = dists_channels, extra_channels
    d.inp, d.out0, d.post_out = x, y, dists
    for view, field in zip(extras, ("res", "tail_cat")):
        setattr(d, field, view)
    d.wpacked, d.post_wpacked, d.tail_wpacked = w_c, w_e, a


def conv_prelu(d, nhw, storage, *, x, w, a, cin, cout, y):
    """esr_conv_prelu: y = prelu(w (*) x, a).  x -> inp, w -> wpacked, the slopes a (pack_prelu) -> tail_wpacked, y -> out0."""
    _conv(d, nhw, storage, storage, 3, cin, cout)
    d.inp, d.out0 = x, y
    d.wpacked, d.tail_wpacked = w, a


def mdsa_gate(d, nhw, storage, *, f, x, w, cin, cout, y, seg=None):
    """esr_mdsa_gate (res_mode RES_GATE): y = prelu(w_f . cat(f1, f2, f3), a_f) * sigmoid(w_s . x), all of w_f, a_f, w_s in w (pack_mdsa_gate).
    f -> inp: the cin-channel concat, or with seg = (bytes from one dense tensor to the next, 16-channel chunks read of each) f1's view of a
    planar concat (in_seg_stride, in_seg_chunks); x -> res, y -> out0 (cout channels)."""
    _conv(d, nhw, storage, storage, 1, cin, cout)
    d.res_mode = L.RES_GATE
    d.inp, d.res, d.out0 = f, x, y
    if seg is not None:
        d.in_seg_stride, d.in_seg_chunks = seg
    d.wpacked = w


def pa_gate(d, nhw, storage, *, t, w, c, y, y_width, s=None, hilo=0, hilo_stride=0):
    """esr_pa_gate: y = t * sigmoid(w . t) (+ s; res_mode RES_POST_ACT).  t -> inp (c channels), w (pack_pa_gate) -> wpacked, s -> res,
    y -> out0 (cout = y_width channels stored, those >= c as zeros).  hilo: L.HILO_RES / L.HILO_OUT -- s / y is the high half of a hi + lo
    pair whose low half lies hilo_stride bytes behind it."""
    _conv(d, nhw, storage, storage, 1, c, y_width)
    d.inp, d.out0 = t, y
    if s is not None:
        d.res, d.res_mode = s, L.RES_POST_ACT
    d.hilo, d.hilo_stride = hilo, hilo_stride
    d.wpacked = w


def pa_tail(d, *, x, w3, w):
    """esr_pa_tail, on top of pa_gate's fill: t = w3 (*) x takes the place of the stored t.  x -> inp, w3 -> wpacked, the gate's w -> tail_wpacked."""
    d.ksize = 3
    d.inp = x
    d.wpacked, d.tail_wpacked = w3, w


def asym_step(d, nhw, storage, *, x, w_d, w_taps, cin, c, act, slope, res, dd, y, y_width, p=()):
    """esr_asym_step, a(.) = act / slope: dd = a(w_d . x), a_l, a_m = a(first 3-tap convolutions of x), y = a(second ones (+ x if res) + dd + p[0] + p[1]).
    x -> inp (cin channels), w_taps (pack_asym_s16) -> wpacked, w_d -> post_wpacked, dd -> post_out (post_cout = c, post_act = act),
    y -> out0 (cout = y_width channels stored), the up to two earlier maps p -> res, tail_cat."""
    _conv(d, nhw, storage, storage, 3, cin, y_width)
    d.act, d.slope, d.post_act = act, slope, act
    d.res_mode = L.RES_PRE_ACT if res else L.RES_NONE
    d.inp, d.out0, d.post_out, d.post_cout = x, y, dd, c
    for view, field in zip(p, ("res", "tail_cat")):
        if view is not None:
            setattr(d, field, view)
    d.wpacked, d.post_wpacked = w_taps, w_d


PRELU_SRCS = (("inp", "cin"), ("res", "split"), ("tail_cat", "tail_cat_c"), ("out1", "tail_cout"))


def prelu(d, nhw, storage, *, srcs, a, y):
    """esr_prelu: y[c] = prelu(cat(srcs)[c], a[c]).  The up to four sources [(view, channels), ...] -> PRELU_SRCS in the concat's order,
    cout = their sum, a (pack_prelu) -> wpacked, y -> out0."""
    _conv(d, nhw, storage, storage, 1, 0, sum(c for _, c in srcs))
    for (view, c), (field, count) in zip(srcs, PRELU_SRCS):
        setattr(d, field, view)
        setattr(d, count, c)
    d.out0 = y
    d.wpacked = a


def dwconv3x3(d, nhw, storage, *, x, w, c, act, slope, y, res=None, res_mode=L.RES_NONE):
    """esr_dwconv3x3_f32 (`compute` stays 0): y = act(dw3(x, w) + res) or act(dw3(x, w)) + res (res_mode).  x -> inp, w (pack_dw) -> wpacked,
    cin = cout = c, res -> res, y -> out0."""
    _conv(d, nhw, storage, 0, 3, c, c)
    d.act, d.slope, d.res_mode = act, slope, res_mode
    d.inp, d.out0 = x, y
    if res is not None:
        d.res = res
    d.wpacked = w


def dwconv7x7(d, nhw, storage, *, x, w, c, y):
    """esr_dwconv7x7 (`compute` stays 0): y = dw7(x, w).  x -> inp, w (pack_dw7) -> wpacked, cin = cout = c, y -> out0."""
    _conv(d, nhw, storage, 0, 7, c, c)
    d.inp, d.out0 = x, y
    d.wpacked = w


def esa_unshuffle(d, nhw, storage, *, c1, w, f, y, lo):
    """esr_esa_unshuffle_f32 on an esr_esa_desc: y = relu(con_(relu(max_pool2d(pixel_unshuffle(c1, 2), 7, 3)))).  c1 -> x (f channels, h x w),
    w (pack_unshuffle) -> w0, y -> y, the fp32 map of lo = (h_lo, w_lo) pixels with its ring."""
    d.n, d.h, d.w = nhw
    d.f, d.storage = f, storage
    d.h_lo, d.w_lo = lo
    d.x, d.y = c1, y
    d.w0 = w
