"""CPU-only: what every launcher answers to a broken tensor view, as a table.

Each launcher that takes views gets one valid baseline descriptor on a small host buffer, and from it one descriptor per fault:
for every view the launcher checks, the pointer null, the pitch off its granule, the coff off its granule, the slice one granule
past the pitch, and an image (h and w alone: nothing is allocated) that carries this view over the raw-buffer limit; plus a few
descriptors with two faults per conv launcher, which pin the ORDER of the checks (the first one that fires decides between
ESR_ERR_BAD_ARG and ESR_ERR_UNSUPPORTED, and callers see that code).

Every swept descriptor is one the library refuses (-1 / -2), so nothing is ever launched on these host pointers, with or
without a GPU.  The baselines themselves are called only where there is no device: there they pass every check and fail in the
launch (ESR_ERR_LAUNCH), which shows that the fault, not the baseline, is what the sweep's codes answer to.

EXPECTED holds the codes of the commit BEFORE the view checks moved into esr_internal.h (esr_view_fits / esr_view_ok /
esr_fits_raw): that library was loaded in place of this one (ESR_HIP_LIB) and `PYTHONPATH=. python tests/test_view_validation.py` printed
the table.  They are literals on purpose: the test pins behaviour, it does not restate the rule.

Not swept, because the launcher has no such check and the descriptor would be VALID (and launch): a size fault for
esr_conv3x3s2_f32, esr_maxpool7s3_f32, esr_dwconv3x3_f32 and esr_pack_input_s16; "slice past the pitch" for the views whose
pitch must equal ESA_FP with coff 0 (any other coff is the coff fault)."""
import ctypes

import torch

from ntire2022_esr_amd import _lib as L

_BUF = (ctypes.c_float * 256)()
A = ctypes.addressof(_BUF)
RAW_LIMIT = 2147483647
BF16 = L.STORE["bf16"]


def V(c, g, k=0):
    """a valid view over c channels with one spare granule g (so that a misaligned coff still fits); k: a distinct pointer"""
    return L.View(A + 64 * k, c + g, 0)


def _conv(**kw):
    d = L.ConvDesc()
    d.n, d.h, d.w, d.ksize = 1, 4, 4, 3
    d.in_layout = d.out_layout = L.NHWC
    d.wpacked = A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _conv16(**kw):
    return _conv(storage=BF16, compute=L.COMPUTE_BF16, **kw)


def _esa(**kw):
    d = L.EsaDesc()
    d.n, d.h, d.w, d.c, d.f = 1, 16, 16, 48, 16
    d.c1 = d.c3 = d.w0 = d.w1 = A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _fp_view(k=0):
    return L.View(A + 64 * k, L.ESA_FP, 0)


def _esa_posts():
    d = _esa(storage=BF16, h_lo=2, w_lo=2, x=V(48, 8), y=V(48, 8, 1), post_w=A)
    d.post[0].cout, d.post[0].res_mode, d.post[0].out, d.post[0].res = 48, L.RES_PRE_ACT, V(48, 8, 2), V(48, 8, 3)
    d.post[1].cout, d.post[1].out = 16, V(16, 8, 2)
    return d


def _lowres(**kw):
    d = L.EsaLowresDesc()
    d.n, d.h, d.w, d.f = 1, 32, 32, 16
    d.x, d.pooled, d.y = _fp_view(), A, A
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _lowres_s2():
    d = _lowres(w_s2=A, n_layers=1)
    d.layer[0].kind, d.layer[0].w = 0, A
    return d


def _lowres_pool7():
    d = _lowres(n_layers=2)
    d.layer[0].kind, d.layer[0].w, d.layer[0].w_dw = 2, A, A
    d.layer[1].kind, d.layer[1].w = 3, A
    return d


def _bs(storage=0):
    d = L.BsDesc()
    d.n, d.h, d.w, d.cin, d.c = 1, 4, 4, 32, 32
    d.res_mode = L.RES_POST_ACT
    d.storage = storage
    d.inp, d.out, d.res, d.d_out = V(32, 8 if storage else 4), V(32, 4, 1), V(32, 4, 2), V(16, 4, 3)
    d.pw_packed = d.dw_packed = d.d_packed = A
    d.d_cout = 16
    return d


def _chain(gate):
    d = L.ChainDesc()
    d.n, d.h, d.w = 1, 16, 16
    d.storage, d.compute, d.act, d.slope = BF16, L.COMPUTE_BF16, L.ACT_LRELU, 0.05
    d.inp = V(48, 8)
    for i in range(4 if gate else 3):
        d.wpacked[i] = A
    if gate:            # FMEN's HFAB: sigmoid(conv chain) * x
        d.n_layers, d.cin, d.cmid, d.cout, d.res_mode = 4, 48, 16, 48, L.RES_GATE
        d.post_cout, d.post_out = 48, V(48, 8, 1)
    else:               # RLFN's RLFB
        d.n_layers, d.cin, d.cmid, d.cout, d.res_mode = 3, 48, 48, 48, L.RES_POST_ACT
        d.post_wpacked, d.post_cout, d.post_out = A, 48, V(48, 8, 1)
        d.post2_wpacked, d.post2_cout, d.post2_out = A, 16, V(16, 8, 2)
    return d


def _ca():
    d = L.CaDesc()
    d.n, d.h, d.w, d.c, d.cr, d.layout = 1, 4, 4, 48, 4, L.NHWC
    d.x, d.y = V(48, 4), V(48, 4, 1)
    d.w1 = d.w2 = d.stats = A
    return d


def _tail16(esdb):
    """rfdb_tail_kernel's two descriptors: RFDB (64 inputs, 49 .. 64 outputs) and ESDB (48 inputs, border table, GELU, 33 .. 48)"""
    d = _conv16(h=256, w=256, cin=48 if esdb else 64, cout=32, inp=V(48 if esdb else 64, 8), tail_wpacked=A, tail_cat=V(32, 8, 1),
                tail_cat_c=96, tail_seg_stride16=64, tail_cout=48 if esdb else 64, out0=V(48 if esdb else 64, 8, 2),
                post_wpacked=A, post_cout=16, post_out=V(16, 8, 3))
    if esdb:
        d.border_bias, d.tail_mid_act = A, L.ACT_GELU
    return d


# name -> (entry point, baseline builder, [(view attribute path, granule, size limit)])
# granule 0: a view that must be exactly (pitch ESA_FP, coff 0).  Size limit: the bytes per element where the launcher limits the bytes of one
# image of this view (2 / 4), 1 where it limits element offsets, 0 where it limits a count of pixels, tiles or jobs (once per launcher), None
# where it has no limit for this view
LAUNCHERS = {
    "conv_f32": ("esr_conv2d_f32", lambda: _conv(cin=64, cout=64, res_mode=L.RES_POST_ACT, inp=V(64, 4), out0=V(64, 4, 1), res=V(64, 4, 2)),
                 [("inp", 4, 4), ("out0", 4, 1), ("res", 4, 1)]),
    "conv_f32_tail": ("esr_conv2d_f32", lambda: _conv(cin=48, cout=16, inp=V(48, 4), tail_wpacked=A, tail_cat=V(48, 4, 1), tail_cat_c=48,
                                                       tail_cout=64, out0=V(64, 4, 2)),
                      [("inp", 4, 4), ("tail_cat", 4, 1), ("out0", 4, 1)]),
    "conv_f32_post": ("esr_conv2d_f32", lambda: _conv(cin=64, cout=64, inp=V(64, 4), out0=V(64, 4, 1), post_wpacked=A, post_cout=32,
                                                       post_out=V(32, 4, 2)),
                      [("inp", 4, 4), ("out0", 4, 1), ("post_out", 4, 1)]),
    "conv_f32_blocked_out1": ("esr_conv2d_f32", lambda: _conv(cin=64, cout=64, split=16, blocked8=L.BLOCKED_OUT1, inp=V(64, 4),
                                                               out0=V(16, 4, 1), out1=V(48, 8, 2)),
                              [("inp", 4, 4), ("out0", 4, 1), ("out1", 8, 4)]),
    "conv_s16": ("esr_conv2d_f32", lambda: _conv16(cin=48, cout=48, res_mode=L.RES_POST_ACT, inp=V(48, 8), out0=V(48, 8, 1), res=V(48, 8, 2)),
                 [("inp", 8, 2), ("out0", 8, 2), ("res", 8, 2)]),
    "conv_s16_split": ("esr_conv2d_f32", lambda: _conv16(cin=48, cout=48, split=16, inp=V(48, 8), out0=V(16, 8, 1), out1=V(32, 8, 2)),
                       [("inp", 8, 2), ("out0", 8, 2), ("out1", 8, 2)]),
    "conv_s16_post2": ("esr_conv2d_f32", lambda: _conv16(cin=48, cout=48, res_mode=L.RES_POST_ACT, inp=V(48, 8), out0=V(48, 8, 1), res=V(48, 8, 2),
                                                          post_wpacked=A, post_cout=48, post_out=V(48, 8, 3), post2_wpacked=A, post2_cout=16,
                                                          post2_out=V(16, 8, 3)),
                       [("inp", 8, 2), ("out0", 8, 2), ("res", 8, 2), ("post_out", 8, 2), ("post2_out", 8, 2)]),
    "conv_s16_hilo": ("esr_conv2d_f32", lambda: _conv16(cin=48, cout=48, hilo=L.HILO_OUT, hilo_stride=4096, inp=V(48, 8), out0=V(48, 8, 1)),
                      [("inp", 8, 2), ("out0", 8, 2)]),
    "conv_s16_segmented": ("esr_conv2d_f32", lambda: _conv16(cin=96, cout=48, ksize=1, in_seg_stride=4096, in_seg_chunks=2, inp=V(24, 8),
                                                              out0=V(48, 8, 1)),
                           [("inp", 8, 2), ("out0", 8, 2)]),
    "conv_s16_rfdb_tail": ("esr_conv2d_f32", lambda: _tail16(False), [("inp", 8, 2), ("tail_cat", 8, 2), ("out0", 8, 2), ("post_out", 8, 2)]),
    "conv_s16_esdb_tail": ("esr_conv2d_f32", lambda: _tail16(True), [("inp", 8, 2), ("tail_cat", 8, 2), ("out0", 8, 2), ("post_out", 8, 2)]),
    "conv3x3s2": ("esr_conv3x3s2_f32", lambda: _esa(h_lo=7, w_lo=7, x=_fp_view(), y=_fp_view(1)), [("x", 0, None), ("y", 0, None)]),
    "maxpool7s3": ("esr_maxpool7s3_f32", lambda: _esa(h_lo=4, w_lo=4, x=_fp_view(), y=_fp_view(1)), [("x", 0, None), ("y", 0, None)]),
    "maxpool7s7": ("esr_maxpool7s7_f32", lambda: _esa(h_lo=2, w_lo=2, x=_fp_view(), y=_fp_view(1)), [("x", 0, 0), ("y", 0, None)]),
    "esa_apply": ("esr_esa_apply_f32", lambda: _esa(h_lo=2, w_lo=2, x=V(48, 4), y=V(48, 4, 1)), [("x", 4, 0), ("y", 4, None)]),
    "esa_apply_posts": ("esr_esa_apply_f32", _esa_posts,
                        [("x", 8, 0), ("y", 8, None), ("post.0.out", 8, None), ("post.0.res", 8, None), ("post.1.out", 8, None)]),
    "esa_lowres_s2": ("esr_esa_lowres_f32", _lowres_s2, [("x", 0, 0)]),
    "esa_lowres_pool7": ("esr_esa_lowres_f32", _lowres_pool7, [("x", 0, 0)]),
    "dwconv": ("esr_dwconv3x3_f32", lambda: _conv(cin=48, cout=48, res_mode=L.RES_POST_ACT, inp=V(48, 4), out0=V(48, 4, 1), res=V(48, 4, 2)),
               [("inp", 4, None), ("out0", 4, None), ("res", 4, None)]),
    "bsconv": ("esr_bsconv_f32", _bs, [("inp", 4, 4), ("out", 4, 1), ("res", 4, 1), ("d_out", 4, 1)]),
    "bsconv_s16": ("esr_bsconv_f32", lambda: _bs(BF16), [("inp", 8, 4), ("out", 4, 1), ("res", 4, 1), ("d_out", 4, 1)]),
    "chain_rlfb": ("esr_conv_chain_s16", lambda: _chain(False), [("inp", 8, 2), ("post_out", 8, 2), ("post2_out", 8, 2)]),
    "chain_gate": ("esr_conv_chain_s16", lambda: _chain(True), [("inp", 8, 2), ("post_out", 8, None)]),
    "channel_attention": ("esr_channel_attention_f32", _ca, [("x", 4, 0), ("y", 4, None)]),
    "pack_input": ("esr_pack_input_s16", lambda: _conv(cin=3, storage=BF16, inp=L.View(A, 0, 0), out0=V(16, 8, 1)), [("out0", 8, None)]),
}
# pack_input's fp32 NCHW input has a pointer and nothing else to check
POINTER_ONLY = {"pack_input": ["inp"]}
# a post chain may consume the 16-bit conv's result alone: a null out0 is a valid descriptor there
NOT_A_FAULT = {"conv_s16_post2:out0:ptr"}


def _view(d, path):
    for p in path.split("."):
        d = d[int(p)] if p.isdigit() else getattr(d, p)
    return d


def _huge(pitch, elem_bytes):
    """(h, w) of the smallest image of 32768-pixel rows whose pitch * elem_bytes bytes per pixel reach the raw-buffer limit; elem_bytes 0:
    a launcher that limits counts (pixels, tiles, jobs) and not bytes -- the largest image there is"""
    if elem_bytes == 0:
        return 2147483647, 2147483647
    w = 32768
    return -(-RAW_LIMIT // (pitch * elem_bytes * w)), w


def _cases():
    """(id, entry point, descriptor)"""
    for name, (fn, base, views) in LAUNCHERS.items():
        for path in POINTER_ONLY.get(name, []):
            d = base()
            _view(d, path).ptr = None
            yield f"{name}:{path}:ptr", fn, d
        for path, g, eb in views:
            faults = {"ptr": lambda v: setattr(v, "ptr", None), "pitch": lambda v: setattr(v, "pitch", v.pitch + 1),
                      "coff": lambda v: setattr(v, "coff", 1)}
            if g:
                faults["past"] = lambda v, g=g: setattr(v, "coff", 2 * g)
            for what, f in faults.items():
                d = base()
                f(_view(d, path))
                if f"{name}:{path}:{what}" not in NOT_A_FAULT:
                    yield f"{name}:{path}:{what}", fn, d
            if eb is not None:
                d = base()
                if path != views[0][0]:               # widened (still valid), so that the image carries THIS view over the limit and no other
                    _view(d, path).pitch *= 8
                d.h, d.w = _huge(_view(d, path).pitch, eb)
                if name == "maxpool7s7":              # (the pooled size has to follow, or that is the fault)
                    d.h_lo, d.w_lo = (d.h - 5) // 7 + 1, (d.w - 5) // 7 + 1
                yield f"{name}:{path}:size", fn, d
    # two faults: which check fires first
    for name in ("conv_f32", "conv_f32_tail", "conv_f32_post", "conv_f32_blocked_out1", "conv_s16", "conv_s16_split", "conv_s16_post2",
                 "conv_s16_hilo", "conv_s16_segmented", "conv_s16_rfdb_tail"):
        fn, base, views = LAUNCHERS[name]
        last = views[-1][0]
        for path in ("inp", last):                    # a misaligned pitch + an image over every view's limit
            d = base()
            _view(d, path).pitch += 1
            d.h = d.w = 65536
            yield f"{name}:{path}:pitch+size", fn, d
        d = base()                                    # an unsupported shape + a view that does not fit
        d.ksize = 5
        _view(d, last).coff = 2 * views[-1][1]
        yield f"{name}:{last}:ksize+past", fn, d
        d = base()                                    # an unknown layout + a null pointer
        d.out_layout = 7
        _view(d, last).ptr = None
        yield f"{name}:{last}:layout+ptr", fn, d
        d = base()                                    # the first and the last view
        _view(d, "inp").coff = 1
        d.h = d.w = 65536
        _view(d, last).ptr = None
        yield f"{name}:inp+{last}:coff+size+ptr", fn, d


EXPECTED = {
    "conv_f32:inp:ptr": -1,
    "conv_f32:inp:pitch": -1,
    "conv_f32:inp:coff": -1,
    "conv_f32:inp:past": -1,
    "conv_f32:inp:size": -2,
    "conv_f32:out0:ptr": -1,
    "conv_f32:out0:pitch": -1,
    "conv_f32:out0:coff": -1,
    "conv_f32:out0:past": -1,
    "conv_f32:out0:size": -2,
    "conv_f32:res:ptr": -1,
    "conv_f32:res:pitch": -1,
    "conv_f32:res:coff": -1,
    "conv_f32:res:past": -1,
    "conv_f32:res:size": -2,
    "conv_f32_tail:inp:ptr": -1,
    "conv_f32_tail:inp:pitch": -1,
    "conv_f32_tail:inp:coff": -1,
    "conv_f32_tail:inp:past": -1,
    "conv_f32_tail:inp:size": -2,
    "conv_f32_tail:tail_cat:ptr": -1,
    "conv_f32_tail:tail_cat:pitch": -1,
    "conv_f32_tail:tail_cat:coff": -1,
    "conv_f32_tail:tail_cat:past": -1,
    "conv_f32_tail:tail_cat:size": -2,
    "conv_f32_tail:out0:ptr": -1,
    "conv_f32_tail:out0:pitch": -1,
    "conv_f32_tail:out0:coff": -1,
    "conv_f32_tail:out0:past": -1,
    "conv_f32_tail:out0:size": -2,
    "conv_f32_post:inp:ptr": -1,
    "conv_f32_post:inp:pitch": -1,
    "conv_f32_post:inp:coff": -1,
    "conv_f32_post:inp:past": -1,
    "conv_f32_post:inp:size": -2,
    "conv_f32_post:out0:ptr": -1,
    "conv_f32_post:out0:pitch": -1,
    "conv_f32_post:out0:coff": -1,
    "conv_f32_post:out0:past": -1,
    "conv_f32_post:out0:size": -2,
    "conv_f32_post:post_out:ptr": -1,
    "conv_f32_post:post_out:pitch": -1,
    "conv_f32_post:post_out:coff": -1,
    "conv_f32_post:post_out:past": -1,
    "conv_f32_post:post_out:size": -2,
    "conv_f32_blocked_out1:inp:ptr": -1,
    "conv_f32_blocked_out1:inp:pitch": -1,
    "conv_f32_blocked_out1:inp:coff": -1,
    "conv_f32_blocked_out1:inp:past": -1,
    "conv_f32_blocked_out1:inp:size": -2,
    "conv_f32_blocked_out1:out0:ptr": -1,
    "conv_f32_blocked_out1:out0:pitch": -1,
    "conv_f32_blocked_out1:out0:coff": -1,
    "conv_f32_blocked_out1:out0:past": -1,
    "conv_f32_blocked_out1:out0:size": -2,
    "conv_f32_blocked_out1:out1:ptr": -1,
    "conv_f32_blocked_out1:out1:pitch": -1,
    "conv_f32_blocked_out1:out1:coff": -1,
    "conv_f32_blocked_out1:out1:past": -1,
    "conv_f32_blocked_out1:out1:size": -2,
    "conv_s16:inp:ptr": -1,
    "conv_s16:inp:pitch": -1,
    "conv_s16:inp:coff": -1,
    "conv_s16:inp:past": -1,
    "conv_s16:inp:size": -2,
    "conv_s16:out0:ptr": -1,
    "conv_s16:out0:pitch": -1,
    "conv_s16:out0:coff": -1,
    "conv_s16:out0:past": -1,
    "conv_s16:out0:size": -2,
    "conv_s16:res:ptr": -1,
    "conv_s16:res:pitch": -1,
    "conv_s16:res:coff": -1,
    "conv_s16:res:past": -1,
    "conv_s16:res:size": -2,
    "conv_s16_split:inp:ptr": -1,
    "conv_s16_split:inp:pitch": -1,
    "conv_s16_split:inp:coff": -1,
    "conv_s16_split:inp:past": -1,
    "conv_s16_split:inp:size": -2,
    "conv_s16_split:out0:ptr": -1,
    "conv_s16_split:out0:pitch": -1,
    "conv_s16_split:out0:coff": -1,
    "conv_s16_split:out0:past": -1,
    "conv_s16_split:out0:size": -2,
    "conv_s16_split:out1:ptr": -1,
    "conv_s16_split:out1:pitch": -1,
    "conv_s16_split:out1:coff": -1,
    "conv_s16_split:out1:past": -1,
    "conv_s16_split:out1:size": -2,
    "conv_s16_post2:inp:ptr": -1,
    "conv_s16_post2:inp:pitch": -1,
    "conv_s16_post2:inp:coff": -1,
    "conv_s16_post2:inp:past": -1,
    "conv_s16_post2:inp:size": -2,
    "conv_s16_post2:out0:pitch": -1,
    "conv_s16_post2:out0:coff": -1,
    "conv_s16_post2:out0:past": -1,
    "conv_s16_post2:out0:size": -2,
    "conv_s16_post2:res:ptr": -1,
    "conv_s16_post2:res:pitch": -1,
    "conv_s16_post2:res:coff": -1,
    "conv_s16_post2:res:past": -1,
    "conv_s16_post2:res:size": -2,
    "conv_s16_post2:post_out:ptr": -1,
    "conv_s16_post2:post_out:pitch": -1,
    "conv_s16_post2:post_out:coff": -1,
    "conv_s16_post2:post_out:past": -1,
    "conv_s16_post2:post_out:size": -2,
    "conv_s16_post2:post2_out:ptr": -1,
    "conv_s16_post2:post2_out:pitch": -1,
    "conv_s16_post2:post2_out:coff": -1,
    "conv_s16_post2:post2_out:past": -1,
    "conv_s16_post2:post2_out:size": -2,
    "conv_s16_hilo:inp:ptr": -1,
    "conv_s16_hilo:inp:pitch": -1,
    "conv_s16_hilo:inp:coff": -1,
    "conv_s16_hilo:inp:past": -1,
    "conv_s16_hilo:inp:size": -2,
    "conv_s16_hilo:out0:ptr": -1,
    "conv_s16_hilo:out0:pitch": -1,
    "conv_s16_hilo:out0:coff": -1,
    "conv_s16_hilo:out0:past": -1,
    "conv_s16_hilo:out0:size": -2,
    "conv_s16_segmented:inp:ptr": -1,
    "conv_s16_segmented:inp:pitch": -1,
    "conv_s16_segmented:inp:coff": -1,
    "conv_s16_segmented:inp:past": -1,
    "conv_s16_segmented:inp:size": -2,
    "conv_s16_segmented:out0:ptr": -1,
    "conv_s16_segmented:out0:pitch": -1,
    "conv_s16_segmented:out0:coff": -1,
    "conv_s16_segmented:out0:past": -1,
    "conv_s16_segmented:out0:size": -2,
    "conv_s16_rfdb_tail:inp:ptr": -1,
    "conv_s16_rfdb_tail:inp:pitch": -2,
    "conv_s16_rfdb_tail:inp:coff": -2,
    "conv_s16_rfdb_tail:inp:past": -2,
    "conv_s16_rfdb_tail:inp:size": -2,
    "conv_s16_rfdb_tail:tail_cat:ptr": -2,
    "conv_s16_rfdb_tail:tail_cat:pitch": -2,
    "conv_s16_rfdb_tail:tail_cat:coff": -2,
    "conv_s16_rfdb_tail:tail_cat:past": -2,
    "conv_s16_rfdb_tail:tail_cat:size": -2,
    "conv_s16_rfdb_tail:out0:ptr": -2,
    "conv_s16_rfdb_tail:out0:pitch": -2,
    "conv_s16_rfdb_tail:out0:coff": -2,
    "conv_s16_rfdb_tail:out0:past": -2,
    "conv_s16_rfdb_tail:out0:size": -2,
    "conv_s16_rfdb_tail:post_out:ptr": -2,
    "conv_s16_rfdb_tail:post_out:pitch": -2,
    "conv_s16_rfdb_tail:post_out:coff": -2,
    "conv_s16_rfdb_tail:post_out:past": -2,
    "conv_s16_rfdb_tail:post_out:size": -2,
    "conv_s16_esdb_tail:inp:ptr": -1,
    "conv_s16_esdb_tail:inp:pitch": -2,
    "conv_s16_esdb_tail:inp:coff": -2,
    "conv_s16_esdb_tail:inp:past": -2,
    "conv_s16_esdb_tail:inp:size": -2,
    "conv_s16_esdb_tail:tail_cat:ptr": -2,
    "conv_s16_esdb_tail:tail_cat:pitch": -2,
    "conv_s16_esdb_tail:tail_cat:coff": -2,
    "conv_s16_esdb_tail:tail_cat:past": -2,
    "conv_s16_esdb_tail:tail_cat:size": -2,
    "conv_s16_esdb_tail:out0:ptr": -2,
    "conv_s16_esdb_tail:out0:pitch": -2,
    "conv_s16_esdb_tail:out0:coff": -2,
    "conv_s16_esdb_tail:out0:past": -2,
    "conv_s16_esdb_tail:out0:size": -2,
    "conv_s16_esdb_tail:post_out:ptr": -2,
    "conv_s16_esdb_tail:post_out:pitch": -2,
    "conv_s16_esdb_tail:post_out:coff": -2,
    "conv_s16_esdb_tail:post_out:past": -2,
    "conv_s16_esdb_tail:post_out:size": -2,
    "conv3x3s2:x:ptr": -1,
    "conv3x3s2:x:pitch": -1,
    "conv3x3s2:x:coff": -1,
    "conv3x3s2:y:ptr": -1,
    "conv3x3s2:y:pitch": -1,
    "conv3x3s2:y:coff": -1,
    "maxpool7s3:x:ptr": -1,
    "maxpool7s3:x:pitch": -1,
    "maxpool7s3:x:coff": -1,
    "maxpool7s3:y:ptr": -1,
    "maxpool7s3:y:pitch": -1,
    "maxpool7s3:y:coff": -1,
    "maxpool7s7:x:ptr": -1,
    "maxpool7s7:x:pitch": -1,
    "maxpool7s7:x:coff": -1,
    "maxpool7s7:x:size": -2,
    "maxpool7s7:y:ptr": -1,
    "maxpool7s7:y:pitch": -1,
    "maxpool7s7:y:coff": -1,
    "esa_apply:x:ptr": -1,
    "esa_apply:x:pitch": -1,
    "esa_apply:x:coff": -1,
    "esa_apply:x:past": -1,
    "esa_apply:x:size": -2,
    "esa_apply:y:ptr": -1,
    "esa_apply:y:pitch": -1,
    "esa_apply:y:coff": -1,
    "esa_apply:y:past": -1,
    "esa_apply_posts:x:ptr": -1,
    "esa_apply_posts:x:pitch": -1,
    "esa_apply_posts:x:coff": -1,
    "esa_apply_posts:x:past": -1,
    "esa_apply_posts:x:size": -2,
    "esa_apply_posts:y:ptr": -1,
    "esa_apply_posts:y:pitch": -1,
    "esa_apply_posts:y:coff": -1,
    "esa_apply_posts:y:past": -1,
    "esa_apply_posts:post.0.out:ptr": -1,
    "esa_apply_posts:post.0.out:pitch": -1,
    "esa_apply_posts:post.0.out:coff": -1,
    "esa_apply_posts:post.0.out:past": -1,
    "esa_apply_posts:post.0.res:ptr": -1,
    "esa_apply_posts:post.0.res:pitch": -1,
    "esa_apply_posts:post.0.res:coff": -1,
    "esa_apply_posts:post.0.res:past": -1,
    "esa_apply_posts:post.1.out:ptr": -1,
    "esa_apply_posts:post.1.out:pitch": -1,
    "esa_apply_posts:post.1.out:coff": -1,
    "esa_apply_posts:post.1.out:past": -1,
    "esa_lowres_s2:x:ptr": -1,
    "esa_lowres_s2:x:pitch": -1,
    "esa_lowres_s2:x:coff": -1,
    "esa_lowres_s2:x:size": -2,
    "esa_lowres_pool7:x:ptr": -1,
    "esa_lowres_pool7:x:pitch": -1,
    "esa_lowres_pool7:x:coff": -1,
    "esa_lowres_pool7:x:size": -2,
    "dwconv:inp:ptr": -1,
    "dwconv:inp:pitch": -1,
    "dwconv:inp:coff": -1,
    "dwconv:inp:past": -1,
    "dwconv:out0:ptr": -1,
    "dwconv:out0:pitch": -1,
    "dwconv:out0:coff": -1,
    "dwconv:out0:past": -1,
    "dwconv:res:ptr": -1,
    "dwconv:res:pitch": -1,
    "dwconv:res:coff": -1,
    "dwconv:res:past": -1,
    "bsconv:inp:ptr": -1,
    "bsconv:inp:pitch": -1,
    "bsconv:inp:coff": -1,
    "bsconv:inp:past": -1,
    "bsconv:inp:size": -2,
    "bsconv:out:ptr": -1,
    "bsconv:out:pitch": -1,
    "bsconv:out:coff": -1,
    "bsconv:out:past": -1,
    "bsconv:out:size": -2,
    "bsconv:res:ptr": -1,
    "bsconv:res:pitch": -1,
    "bsconv:res:coff": -1,
    "bsconv:res:past": -1,
    "bsconv:res:size": -2,
    "bsconv:d_out:ptr": -1,
    "bsconv:d_out:pitch": -1,
    "bsconv:d_out:coff": -1,
    "bsconv:d_out:past": -1,
    "bsconv:d_out:size": -2,
    "bsconv_s16:inp:ptr": -1,
    "bsconv_s16:inp:pitch": -1,
    "bsconv_s16:inp:coff": -1,
    "bsconv_s16:inp:past": -1,
    "bsconv_s16:inp:size": -2,
    "bsconv_s16:out:ptr": -1,
    "bsconv_s16:out:pitch": -1,
    "bsconv_s16:out:coff": -1,
    "bsconv_s16:out:past": -1,
    "bsconv_s16:out:size": -2,
    "bsconv_s16:res:ptr": -1,
    "bsconv_s16:res:pitch": -1,
    "bsconv_s16:res:coff": -1,
    "bsconv_s16:res:past": -1,
    "bsconv_s16:res:size": -2,
    "bsconv_s16:d_out:ptr": -1,
    "bsconv_s16:d_out:pitch": -1,
    "bsconv_s16:d_out:coff": -1,
    "bsconv_s16:d_out:past": -1,
    "bsconv_s16:d_out:size": -2,
    "chain_rlfb:inp:ptr": -1,
    "chain_rlfb:inp:pitch": -1,
    "chain_rlfb:inp:coff": -1,
    "chain_rlfb:inp:past": -1,
    "chain_rlfb:inp:size": -2,
    "chain_rlfb:post_out:ptr": -1,
    "chain_rlfb:post_out:pitch": -1,
    "chain_rlfb:post_out:coff": -1,
    "chain_rlfb:post_out:past": -1,
    "chain_rlfb:post_out:size": -2,
    "chain_rlfb:post2_out:ptr": -1,
    "chain_rlfb:post2_out:pitch": -1,
    "chain_rlfb:post2_out:coff": -1,
    "chain_rlfb:post2_out:past": -1,
    "chain_rlfb:post2_out:size": -2,
    "chain_gate:inp:ptr": -1,
    "chain_gate:inp:pitch": -1,
    "chain_gate:inp:coff": -1,
    "chain_gate:inp:past": -1,
    "chain_gate:inp:size": -2,
    "chain_gate:post_out:ptr": -1,
    "chain_gate:post_out:pitch": -1,
    "chain_gate:post_out:coff": -1,
    "chain_gate:post_out:past": -1,
    "channel_attention:x:ptr": -1,
    "channel_attention:x:pitch": -1,
    "channel_attention:x:coff": -1,
    "channel_attention:x:past": -1,
    "channel_attention:x:size": -2,
    "channel_attention:y:ptr": -1,
    "channel_attention:y:pitch": -1,
    "channel_attention:y:coff": -1,
    "channel_attention:y:past": -1,
    "pack_input:inp:ptr": -1,
    "pack_input:out0:ptr": -1,
    "pack_input:out0:pitch": -1,
    "pack_input:out0:coff": -1,
    "pack_input:out0:past": -1,
    "conv_f32:inp:pitch+size": -1,
    "conv_f32:res:pitch+size": -1,
    "conv_f32:res:ksize+past": -2,
    "conv_f32:res:layout+ptr": -1,
    "conv_f32:inp+res:coff+size+ptr": -1,
    "conv_f32_tail:inp:pitch+size": -1,
    "conv_f32_tail:out0:pitch+size": -1,
    "conv_f32_tail:out0:ksize+past": -2,
    "conv_f32_tail:out0:layout+ptr": -1,
    "conv_f32_tail:inp+out0:coff+size+ptr": -1,
    "conv_f32_post:inp:pitch+size": -1,
    "conv_f32_post:post_out:pitch+size": -1,
    "conv_f32_post:post_out:ksize+past": -2,
    "conv_f32_post:post_out:layout+ptr": -2,
    "conv_f32_post:inp+post_out:coff+size+ptr": -1,
    "conv_f32_blocked_out1:inp:pitch+size": -1,
    "conv_f32_blocked_out1:out1:pitch+size": -1,
    "conv_f32_blocked_out1:out1:ksize+past": -2,
    "conv_f32_blocked_out1:out1:layout+ptr": -1,
    "conv_f32_blocked_out1:inp+out1:coff+size+ptr": -1,
    "conv_s16:inp:pitch+size": -1,
    "conv_s16:res:pitch+size": -1,
    "conv_s16:res:ksize+past": -2,
    "conv_s16:res:layout+ptr": -1,
    "conv_s16:inp+res:coff+size+ptr": -1,
    "conv_s16_split:inp:pitch+size": -1,
    "conv_s16_split:out1:pitch+size": -1,
    "conv_s16_split:out1:ksize+past": -2,
    "conv_s16_split:out1:layout+ptr": -1,
    "conv_s16_split:inp+out1:coff+size+ptr": -1,
    "conv_s16_post2:inp:pitch+size": -1,
    "conv_s16_post2:post2_out:pitch+size": -2,
    "conv_s16_post2:post2_out:ksize+past": -2,
    "conv_s16_post2:post2_out:layout+ptr": -1,
    "conv_s16_post2:inp+post2_out:coff+size+ptr": -1,
    "conv_s16_hilo:inp:pitch+size": -1,
    "conv_s16_hilo:out0:pitch+size": -1,
    "conv_s16_hilo:out0:ksize+past": -2,
    "conv_s16_hilo:out0:layout+ptr": -1,
    "conv_s16_hilo:inp+out0:coff+size+ptr": -1,
    "conv_s16_segmented:inp:pitch+size": -1,
    "conv_s16_segmented:out0:pitch+size": -1,
    "conv_s16_segmented:out0:ksize+past": -2,
    "conv_s16_segmented:out0:layout+ptr": -1,
    "conv_s16_segmented:inp+out0:coff+size+ptr": -1,
    "conv_s16_rfdb_tail:inp:pitch+size": -2,
    "conv_s16_rfdb_tail:post_out:pitch+size": -2,
    "conv_s16_rfdb_tail:post_out:ksize+past": -2,
    "conv_s16_rfdb_tail:post_out:layout+ptr": -2,
    "conv_s16_rfdb_tail:inp+post_out:coff+size+ptr": -2,
}


def _call(fn, d):
    return getattr(L.lib(), fn)(ctypes.byref(d), None)


def test_table_is_complete():
    """every launcher of the list, every view it checks, every fault: the table is generated from LAUNCHERS, and EXPECTED has a code for
    exactly its cases"""
    ids = [i for i, _, _ in _cases()]
    assert len(ids) == len(set(ids))
    assert set(ids) == set(EXPECTED), set(ids) ^ set(EXPECTED)
    for name, (_, _, views) in LAUNCHERS.items():
        for path, g, _ in views:
            for what in ("ptr", "pitch", "coff") + (("past",) if g else ()):
                assert f"{name}:{path}:{what}" in EXPECTED or f"{name}:{path}:{what}" in NOT_A_FAULT
    assert all(code in (-1, -2) for code in EXPECTED.values())           # refused: never a launch on host pointers


def test_every_broken_view_is_refused_with_the_recorded_code():
    assert all(code in (-1, -2) for code in EXPECTED.values())
    got = {i: _call(fn, d) for i, fn, d in _cases() if EXPECTED.get(i) in (-1, -2)}
    assert got == EXPECTED, {i: (got.get(i), EXPECTED.get(i)) for i in set(got) | set(EXPECTED) if got.get(i) != EXPECTED.get(i)}


def test_baselines_are_valid():
    """without a device every baseline passes every check and fails in the launch (or the LDS opt-in, or the memset, in front of it); only
    there: with a GPU the launch would run, on these host pointers"""
    if torch.cuda.device_count() == 0:
        got = {name: _call(fn, base()) for name, (fn, base, _) in LAUNCHERS.items()}
        assert got == dict.fromkeys(LAUNCHERS, -3), {k: v for k, v in got.items() if v != -3}


if __name__ == "__main__":
    for i, fn, d in _cases():
        print(f'    "{i}": {_call(fn, d)},')
