"""Single-op entry points over the C ABI (used by the parity tests and by callers that
want one fused convolution rather than a whole network).  Tensors are torch CUDA tensors;
only their data_ptr()/stream cross the boundary."""
import contextlib
import ctypes

import torch

from . import _lib as L
from . import descs
from .engine import (pack_asym_s16, pack_conv, pack_conv_s16, pack_cx_pw, pack_distill_s16, pack_dw, pack_dw7, pack_dwpw_pw, pack_mdsa_gate, pack_pa_gate,
                     pack_post_s16, pack_prelu, pack_unshuffle, pack_wino)


def _view(t, coff=0):
    """NHWC tensor [N,H,W,pitch] -> esr_view at channel offset coff; None, an absent operand, stays None"""
    return None if t is None else L.View(ctypes.c_void_p(t.data_ptr()), t.shape[-1], coff)


_STORE_OF = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}


def _provided(t, what, like, shape, cmin, gran):
    """A caller-provided output is checked as the tensor the op would allocate in its place: device and dtype of `like`, contiguous,
    leading dims `shape`, a pixel pitch of at least `cmin` channels in multiples of the storage granule `gran`.  Returns t."""
    if not isinstance(t, torch.Tensor) or t.device != like.device:
        raise L.EsrError(f"{what}: must be a tensor on {like.device}")
    if t.dtype != like.dtype:
        raise L.EsrError(f"{what}: dtype {t.dtype}, the op stores {like.dtype}")
    if not t.is_contiguous() or tuple(t.shape[:-1]) != tuple(shape):
        raise L.EsrError(f"{what}: must be a contiguous [{', '.join(str(v) for v in shape)}, pitch] tensor, got {tuple(t.shape)}")
    if t.shape[-1] % gran or t.shape[-1] < cmin:
        raise L.EsrError(f"{what}: pitch {t.shape[-1]} must be a multiple of {gran} and hold {cmin} channels")
    return t


def _zeros_or(t, what, like, shape, cmin, gran, pitch=None):
    """the output an op stores into: the caller's `t`, checked (_provided), or fresh zeros [*shape, pitch] (default pitch: cmin) like `like`"""
    if t is not None:
        return _provided(t, what, like, shape, cmin, gran)
    return torch.zeros(tuple(shape) + (cmin if pitch is None else pitch,), dtype=like.dtype, device=like.device)


def _s16_store(x, what):
    """the shared opening of the one-launch 16-bit ops: x on the GPU, its storage type by name, 16-bit storage only"""
    if not x.is_cuda:
        raise L.EsrError(f"{what}: tensors must live on the GPU; there is no CPU fallback")
    st = _STORE_OF[x.dtype]
    if st == "f32":
        raise L.EsrError(f"{what}: 16-bit storage only")
    return st


def _any_store(x, what):
    """the shared opening of the ops that take every storage: x on the GPU -> (its storage type by name, the channels of a 16-byte granule)"""
    if not x.is_cuda:
        raise L.EsrError(f"{what}: tensors must live on the GPU; there is no CPU fallback")
    st = _STORE_OF[x.dtype]
    return st, 4 if st == "f32" else 8


_TRACE = None       # kernel_trace(): the list that collects device symbols


@contextlib.contextmanager
def kernel_trace():
    """TEST-ONLY diagnostics (tests/test_gpu_bounds.py); the engine and the models never enter it.  Inside the block every op of this module
    that has an esr_op kind runs as a one-op list through esr_run_ops_profiled -- which dispatches to the same launcher the direct call
    enters -- and the device symbol(s) it launched ("conv64m_kernel<true, false, false, 4, false>", ...; esr_prof_kernel_symbol) are
    appended to the list the block yields: how a test asserts WHICH kernel a launcher selected.  Same launches, same results; two HIP
    events and one stream synchronisation per op on top.  The list is a module global: one thread at a time, not re-entrant across
    threads."""
    global _TRACE
    prev, _TRACE = _TRACE, []
    try:
        yield _TRACE
    finally:
        _TRACE = prev


def _launch(kind, d, stream, what=None, *named):
    """one C ABI call of the launcher of op `kind` (L.LAUNCHERS) on the descriptor d -- also one a caller filled in by hand (the tests do, for
    entry points without a wrapper here); under kernel_trace() as a one-op list through the profiler, which records the device symbol.
    what: the name in the error's text (default: the entry point's).
    The call form from before the table, _launch(fn, what, d, stream, kind, field), is still taken, so that callers written against it keep
    working; the entry point and field it names must be the row's."""
    lib = L.lib()
    if isinstance(kind, str):
        (named_fn, what, d, stream), (kind, named_field) = (kind, d, stream, what), named
        assert (named_fn, named_field) == L.LAUNCHERS[kind][:2], (named_fn, named_field, kind)
    fn, field, _ = L.LAUNCHERS[kind]
    what = what or fn
    if _TRACE is None:
        L.check(getattr(lib, fn)(ctypes.byref(d), ctypes.c_void_p(stream)), what)
        return
    op = L.Op()
    op.kind = kind
    setattr(op, field, d)
    prof = ctypes.c_void_p()
    L.check(lib.esr_prof_create(1, 1, ctypes.byref(prof)), "esr_prof_create")
    try:
        L.check(lib.esr_run_ops_profiled(ctypes.byref(op), 1, ctypes.c_void_p(stream), prof), what)
        buf = ctypes.create_string_buffer(256)
        L.check(lib.esr_prof_kernel_symbol(prof, 0, buf, 256), "esr_prof_kernel_symbol")
        _TRACE.append(buf.value.decode())
    finally:
        # the profiler's events are recorded on THIS stream (0: the default stream)
        (torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()).synchronize()
        lib.esr_prof_destroy(prof)


def _run(kind, d, x, refusal):
    """the shared end of a wrapper: the predicate of the kind's row, where it has one, refuses with EsrError(refusal); else one launch on the
    current stream of x's device"""
    predicate = L.LAUNCHERS[kind][2]
    if predicate is not None and not getattr(L.lib(), predicate)(ctypes.byref(d)):
        raise L.EsrError(refusal)
    _launch(kind, d, torch.cuda.current_stream(x.device).cuda_stream)


def conv2d(x, weight, bias, *, act=L.ACT_NONE, slope=0.05, res=None, res_mode=L.RES_NONE,
           in_nchw=False, shuffle_out=False, out=None, out_coff=0, in_coff=0, cin=None,
           split=0, out1=None, out1_coff=0, res_coff=0, packed=None, cin_map=None, store=None,
           tail_weight=None, tail_bias=None, tail_cat=None, tail_cat_coff=0, tail_mid_act=L.ACT_NONE,
           post_weight=None, post_bias=None, post_act=L.ACT_NONE, post2_weight=None, post2_bias=None, store_main=True,
           border=None, blocked_in=False, blocked_out1=False, wino=False, hilo=0, post_out=None, post2_out=None):
    """Fused conv (k=1|3, stride 1, same padding) on the current stream.

    x       NHWC [N,H,W,pitch] (channels [in_coff, in_coff+cin) are read) or NCHW fp32 if in_nchw.  The dtype of an NHWC
            x is the storage type of the op: float32 -> exact fp32 MFMA; bfloat16 / float16 -> conv_s16_kernel (16-bit
            operands as stored, fp32 accumulate, one rounding at the store); res / out / out1 have the same dtype.
    store   NCHW input only: "bf16" | "f16" makes the NHWC output 16-bit (the head of a 16-bit network)
    returns NHWC [N,H,W,cout] (or `out`), or NCHW fp32 [N,cout/16,4H,4W] if shuffle_out
    post_*  esr_conv_desc.post_*: post_weight [pc, cout(, 1, 1)] applied to this conv's activated output; returns (y, post).
            16-bit storage: applied to the finished fp32 result (residual included); post2_weight [pc2, pc] chains a second 1x1
            on the first (returns (y, post, post2)); store_main=False does not store y (returns None in its place)
    post_out / post2_out   caller-provided NHWC [N,H,W,pitch] tensors for the two 1x1 results (default: freshly allocated zeros of pitch
            round_up(channels, granule)); same dtype and device as the op's storage, pitch a multiple of the granule (4 fp32 / 8 16-bit)
            that holds the channels, written from channel 0; EsrError otherwise
    border  esr_conv_desc.border_bias: fp32 [16, round_up(cout, 16)] table added by outside-mask (16-bit storage only)
    blocked_in / blocked_out1   esr_conv_desc.blocked8: x / out1 is a channel-blocked fp32 tensor [N, C/8, H, W, 8]
    hilo    esr_conv_desc.hilo (bf16, 3x3, 33..64 output channels): L.HILO_IN -- x is a contiguous [2, N, H, W, P] pair (value = x[0] + x[1]:
            high parts, low parts); L.HILO_RES -- so is res; L.HILO_OUT -- so will y be ([2, N, H, W, round_up(cout, 16)]); all pairs of one
            call must have the same x.stride(0)
    wino    fp32 3x3: also pass Winograd F(2x2, 3x3) weights (esr_conv_desc.wino_wpacked); raises if the shape does not qualify
    tail_*  fused 1x1 (esr_conv_desc.tail_*): tail_weight [cout1, cat_c + 16(, 1, 1)] over concat(tail_cat slice,
            mid_act(this 3x3 conv)); act / res / out then apply to the 1x1, whose output is returned
    """
    if not x.is_cuda:
        raise L.EsrError("conv2d: tensors must live on the GPU; there is no CPU fallback")
    lib = L.lib()
    w4 = weight if weight.dim() == 4 else weight[:, :, None, None]
    cout, wcin, k, _ = w4.shape
    st = _STORE_OF[x.dtype] if not in_nchw else (store or "f32")
    s16 = st != "f32" and not in_nchw
    if packed is None:
        packed = (pack_conv_s16(weight, bias, st, cin_map=cin_map) if s16 else pack_conv(weight, bias, cin_map=cin_map)).to(x.device)
    odt = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[st]
    gran = 4 if st == "f32" else 8
    d = L.ConvDesc()
    d.storage = L.STORE[st]
    d.compute = L.COMPUTE[st] if s16 else 0
    hilo_strides = []
    if in_nchw:
        n, c, h, w = x.shape
        d.in_layout, cin = L.NCHW_IN, c
        d.inp = L.View(ctypes.c_void_p(x.data_ptr()), 0, 0)
    elif blocked_in:
        if x.dim() != 5 or x.shape[-1] != 8 or x.dtype != torch.float32 or not x.is_contiguous():
            raise L.EsrError("conv2d: a blocked input is a contiguous fp32 [N, C/8, H, W, 8] tensor")
        n, pl, h, w, _ = x.shape
        cin = wcin if cin is None else cin
        d.in_layout = L.NHWC
        d.inp = L.View(ctypes.c_void_p(x.data_ptr()), pl * 8, in_coff)
        d.blocked8 |= L.BLOCKED_IN
    elif hilo & L.HILO_IN:
        if x.dim() != 5 or x.shape[0] != 2 or not x.is_contiguous():
            raise L.EsrError("conv2d: a hi + lo input is a contiguous [2, N, H, W, P] pair")
        _, n, h, w, _ = x.shape
        cin = wcin if cin is None else cin
        d.in_layout = L.NHWC
        d.inp = _view(x[0], in_coff)
        _hilo_pair(x, "input", hilo_strides)
    elif x.dim() == 5:
        # planar concat [S, N, H, W, P]: S dense tensors one stride apart (esr_conv_desc.in_seg_stride / in_seg_chunks)
        if not s16 or not x.is_contiguous() or x.shape[-1] % 16:
            raise L.EsrError("conv2d: a segmented input is a contiguous 16-bit [S, N, H, W, P] tensor with P a multiple of 16")
        nseg, n, h, w, pp = x.shape
        cin = wcin if cin is None else cin
        d.in_layout = L.NHWC
        d.inp = L.View(ctypes.c_void_p(x.data_ptr()), pp, 0)
        d.in_seg_stride, d.in_seg_chunks = x.stride(0) * x.element_size(), pp // 16
    else:
        n, h, w, _ = x.shape
        cin = wcin if cin is None else cin
        d.in_layout = L.NHWC
        d.inp = _view(x, in_coff)
    d.n, d.h, d.w, d.cin, d.cout, d.ksize = n, h, w, cin, cout, k
    keep = None
    if tail_weight is not None:
        tw = tail_weight if tail_weight.dim() == 4 else tail_weight[:, :, None, None]
        keep = pack_conv(tw, tail_bias).to(x.device)
        d.tail_wpacked = ctypes.c_void_p(keep.data_ptr())
        d.tail_cat = _view(tail_cat, tail_cat_coff)
        d.tail_cat_c, d.tail_cout, d.tail_mid_act = tw.shape[1] - 16, tw.shape[0], tail_mid_act
        cout = tw.shape[0]                      # what the epilogue stores
    d.act, d.slope, d.res_mode, d.split = act, slope, res_mode, split
    if border is not None:
        if border.dtype != torch.float32 or not border.is_contiguous() or tuple(border.shape) != (16, (cout + 15) // 16 * 16):
            raise L.EsrError("conv2d: border must be a contiguous fp32 [16, round_up(cout, 16)] tensor")
        d.border_bias = ctypes.c_void_p(border.data_ptr())
    if shuffle_out:
        y = torch.empty((n, cout // 16, 4 * h, 4 * w), dtype=torch.float32, device=x.device) if out is None else out
        d.out_layout = L.NCHW_SHUFFLE4
        d.out0 = L.View(ctypes.c_void_p(y.data_ptr()), 0, 0)
    else:
        d.out_layout = L.NHWC
        if not store_main:
            y = None
        else:
            if out is None:
                c_store = (min(split, cout) if split else cout)
                y = torch.zeros(((2,) if hilo & L.HILO_OUT else ()) + (n, h, w, (c_store + gran - 1) // gran * gran if not hilo & L.HILO_OUT else (cout + 15) // 16 * 16),
                                dtype=odt, device=x.device)
            else:
                y = out
            if hilo & L.HILO_OUT:
                if y.dim() != 5 or y.shape[0] != 2 or not y.is_contiguous():
                    raise L.EsrError("conv2d: a hi + lo output is a contiguous [2, N, H, W, P] pair")
                d.out0 = _view(y[0], out_coff)
                _hilo_pair(y, "output", hilo_strides)
            else:
                d.out0 = _view(y, out_coff)
        if out1 is not None:
            if blocked_out1:
                if out1.dim() != 5 or out1.shape[-1] != 8 or out1.dtype != torch.float32 or not out1.is_contiguous():
                    raise L.EsrError("conv2d: a blocked out1 is a contiguous fp32 [N, C/8, H, W, 8] tensor")
                d.out1 = L.View(ctypes.c_void_p(out1.data_ptr()), out1.shape[1] * 8, out1_coff)
                d.blocked8 |= L.BLOCKED_OUT1
            else:
                d.out1 = _view(out1, out1_coff)
    if res is not None and hilo & L.HILO_RES:
        if res.dim() != 5 or res.shape[0] != 2 or not res.is_contiguous():
            raise L.EsrError("conv2d: a hi + lo residual is a contiguous [2, N, H, W, P] pair")
        d.res = _view(res[0], res_coff)
        _hilo_pair(res, "residual", hilo_strides)
    elif res is not None:
        d.res = _view(res, res_coff)
    d.hilo = hilo
    if hilo_strides:
        # ONE stride field serves every pair of the descriptor (esr_conv_desc.hilo_stride): pairs of different geometry would make the
        # kernel address a low tensor at the wrong place
        if len(set(hilo_strides)) != 1:
            raise L.EsrError(f"conv2d: the hi + lo pairs of one call must have the same stride between their halves, got {sorted(set(hilo_strides))}")
        d.hilo_stride = hilo_strides[0]
    d.wpacked = ctypes.c_void_p(packed.data_ptr())
    if wino:
        keepw = pack_wino(w4, bias, cin_map=cin_map).to(x.device)
        if not lib.esr_wino_supported(ctypes.byref(d)):
            raise L.EsrError("conv2d: this descriptor does not qualify for the Winograd kernel (esr_wino_supported)")
        d.wino_wpacked = ctypes.c_void_p(keepw.data_ptr())
    yp = yp2 = None
    if post_weight is not None:
        pw = post_weight if post_weight.dim() == 4 else post_weight[:, :, None, None]
        keep2 = (pack_post_s16(pw, post_bias, st) if s16 else pack_conv(pw, post_bias)).to(x.device)
        pcs = (pw.shape[0] + gran - 1) // gran * gran
        like = torch.empty(0, dtype=odt, device=x.device)
        yp = _zeros_or(post_out, "conv2d: post_out", like, (n, h, w), pcs, gran)
        d.post_wpacked, d.post_out = ctypes.c_void_p(keep2.data_ptr()), _view(yp)
        d.post_cout, d.post_act = pw.shape[0], post_act
        if post2_weight is not None:
            keep3 = pack_post_s16(post2_weight, post2_bias, st).to(x.device)
            pcs2 = (post2_weight.shape[0] + 7) // 8 * 8
            yp2 = _zeros_or(post2_out, "conv2d: post2_out", like, (n, h, w), pcs2, 8)
            d.post2_wpacked, d.post2_out, d.post2_cout = ctypes.c_void_p(keep3.data_ptr()), _view(yp2), post2_weight.shape[0]
    stream = torch.cuda.current_stream(x.device).cuda_stream
    if (post_out is not None and post_weight is None) or (post2_out is not None and post2_weight is None):
        raise L.EsrError("conv2d: post_out / post2_out without the post weights")
    _launch(L.OP_CONV, d, stream)
    if yp is None:
        return y
    return (y, yp) if yp2 is None else (y, yp, yp2)


def conv_chain(x, weights, biases, post_weight=None, post_bias=None, post2_weight=None, post2_bias=None, *, act=L.ACT_LRELU, slope=0.05,
               res_mode=L.RES_POST_ACT, post_act=L.ACT_NONE, cin=None, out=None, v_out=None, c1_out=None):
    """esr_conv_chain_s16 (ABI v11): a residual block's chain of 3x3 convolutions in ONE launch on a 16-bit NHWC tensor x [N, H, W, P]
    (RLFB.forward, team04_rlfn.py:109-122): t = x; t = act(conv_i(t)) for all but the last 3x3; u = act(conv_n(t)) + x;
    v = post_act(post_weight . u + post_bias) -> stored; c1 = post2_weight . v_fp32 + post2_bias -> stored.  Returns (v, c1).
    weights: list of OIHW fp32 3x3 weights, biases: list of fp32 biases (or None).
    res_mode=L.RES_GATE is FMEN's HFAB (team03_fmen.py:60-73; four 3x3s, no post weights): t = act(conv_i(t)) for the first three,
    y = sigmoid(conv_4(t)) * x, returned as an NHWC tensor of x's pitch (or stored into `out`, same geometry); `cin` channels of x are read.
    `out` is checked like every caller-provided output (x's dtype and device, contiguous [N, H, W, pitch >= x's pitch in multiples of 8]):
    a tensor that fails the check used to reach the kernel unchecked and now raises EsrError.
    v_out / c1_out (RLFB form): caller-provided NHWC [N, H, W, pitch] tensors of x's dtype and device for v (pitch a multiple of 16 holding
    the first 1x1's channels) and c1 (a multiple of 8 holding the second's); default: freshly allocated zeros.  EsrError otherwise."""
    st = _s16_store(x, "conv_chain")
    n, h, w, pitch = x.shape
    keep = [pack_conv_s16(wt, b, st, cin_phys=(wt.shape[1] + 15) // 16 * 16).to(x.device) for wt, b in zip(weights, biases)]
    common = dict(x=_view(x), w=[k.data_ptr() for k in keep], cin=weights[0].shape[1] if cin is None else cin, cmid=weights[0].shape[0],
                  cout=weights[-1].shape[0], act=act, slope=slope)
    d = L.ChainDesc()
    if res_mode == L.RES_GATE:
        y = _zeros_or(out, "conv_chain: out", x, (n, h, w), pitch, 8)
        # (the pad channels of the last chunk too, as the per-layer store: zeros)
        descs.hfab(d, (n, h, w), L.STORE[st], **common, y=_view(y), y_width=min((common["cout"] + 15) // 16 * 16, y.shape[-1]))
        outs = y
    else:
        pw = post_weight if post_weight.dim() == 4 else post_weight[:, :, None, None]
        keep += [pack_post_s16(pw, post_bias, st).to(x.device), pack_post_s16(post2_weight, post2_bias, st).to(x.device)]
        v = _zeros_or(v_out, "conv_chain: v_out", x, (n, h, w), (pw.shape[0] + 15) // 16 * 16, 16)
        c1 = _zeros_or(c1_out, "conv_chain: c1_out", x, (n, h, w), (post2_weight.shape[0] + 7) // 8 * 8, 8)
        descs.chain(d, (n, h, w), L.STORE[st], **common, res_mode=res_mode, post_w=keep[-2].data_ptr(), v=_view(v), v_width=pw.shape[0],
                    post_act=post_act, post2_w=keep[-1].data_ptr(), c1=_view(c1), c1_width=post2_weight.shape[0])
        outs = v, c1
    _run(L.OP_CONV_CHAIN, d, x, "conv_chain: no kernel for this shape (esr_conv_chain_supported)")
    return outs


def distill_step(x, w_d, b_d, w_r, b_r, w_b, b_b, *, res=False, cin=None, in_coff=0, d_out=None, d_coff=0, d_channels=None,
                 out=None, out_coff=0, out_channels=None):
    """esr_distill_step_s16: one distillation step of BMDN's block (team37_bmdn.py:155-171) in ONE launch on a 16-bit NHWC tensor x
    [N, H, W, P]: d = relu(w_d . x + b_d) (1x1), y = relu(conv3x3(x, w_r, b_r) + conv3x3(d, w_b, b_b) (+ x if res)) with d as stored and
    zero-padded.  Returns (d, y).  `cin` channels of x from `in_coff` are read (default: w_d's inputs).
    d_out / out: caller-provided NHWC tensors of x's dtype and device (pitch a multiple of 8) that receive d / y from channel d_coff /
    out_coff; default: freshly allocated zeros of pitch round_up(channels, 8).  d_channels / out_channels: esr_chain_desc.post_cout /
    post2_cout, the stored widths (default: the logical ones; up to round_up(.., 16): the pad channels are written as zeros)."""
    st = _s16_store(x, "distill_step")
    n, h, w, _ = x.shape
    w1 = w_d if w_d.dim() == 4 else w_d[:, :, None, None]
    keep = [pack_conv_s16(w1, b_d, st, cin_phys=(w1.shape[1] + 15) // 16 * 16).to(x.device), pack_distill_s16(w_r, b_r, w_b, b_b, st).to(x.device)]
    dc = w1.shape[0] if d_channels is None else d_channels
    oc = w_r.shape[0] if out_channels is None else out_channels
    dd = _zeros_or(d_out, "distill_step: d_out", x, (n, h, w), (dc + 7) // 8 * 8, 8)
    y = _zeros_or(out, "distill_step: out", x, (n, h, w), (oc + 7) // 8 * 8, 8)
    d = L.ChainDesc()
    descs.distill_step(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), w_d=keep[0].data_ptr(), w_fold=keep[1].data_ptr(),
                       cin=w1.shape[1] if cin is None else cin, cmid=w1.shape[0], cout=w_r.shape[0], res=res, dd=_view(dd, d_coff), d_width=dc,
                       y=_view(y, out_coff), y_width=oc)
    _run(L.OP_DISTILL_STEP, d, x, "distill_step: no kernel for this shape (esr_distill_step_supported)")
    return dd, y


def asym_step(x, w_d, b_d, w_l1, b_l1, w_l2, b_l2, w_m1, b_m1, w_m2, b_m2, *, res=False, p1=None, p2=None, act=L.ACT_LRELU, slope=0.05, cin=None,
              in_coff=0, p1_coff=0, p2_coff=0, d_out=None, d_coff=0, out=None, out_coff=0, out_channels=None):
    """esr_asym_step: one step of ARFDN's block (team14_arfdn/block.py:233-254) in ONE launch on a 16-bit NHWC tensor x [N, H, W, P], with
    a(v) = the activation `act` / `slope`: d = a(w_d . x + b_d) (1x1), a_l = a(conv(x, w_l1 [c, cin, 3, 1])), a_m = a(conv(x, w_m1 [c, cin, 1, 3])),
    y = a(conv(a_l, w_l2 [c, c, 1, 3]) + conv(a_m, w_m2 [c, c, 3, 1]) (+ x if res) + d + p1 + p2) with d, a_l and a_m rounded to x's dtype
    and a_l / a_m zero-padded.  Returns (d, y).  `cin` channels of x from `in_coff` are read (default: w_d's inputs); p1 / p2: NHWC tensors
    of x's dtype whose c channels from p1_coff / p2_coff are added (None: absent).
    d_out / out: caller-provided NHWC tensors (pitch a multiple of 8) that receive d / y from channel d_coff / out_coff; default: freshly
    allocated zeros of pitch round_up(channels, 8).  out_channels: esr_conv_desc.cout, y's stored width (default c; up to
    round_up(c, 16): the pad channels are written as zeros)."""
    st = _s16_store(x, "asym_step")
    n, h, w, _ = x.shape
    w1 = w_d if w_d.dim() == 4 else w_d[:, :, None, None]
    c = w1.shape[0]
    oc = c if out_channels is None else out_channels
    keep = [pack_asym_s16(w_l1, b_l1, w_m1, b_m1, w_l2, b_l2, w_m2, b_m2, st).to(x.device),
            pack_conv_s16(w1, b_d, st, cin_phys=(w1.shape[1] + 15) // 16 * 16).to(x.device)]
    dd = _zeros_or(d_out, "asym_step: d_out", x, (n, h, w), (c + 7) // 8 * 8, 8)
    y = _zeros_or(out, "asym_step: out", x, (n, h, w), (oc + 7) // 8 * 8, 8)
    d = L.ConvDesc()
    descs.asym_step(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), w_d=keep[1].data_ptr(), w_taps=keep[0].data_ptr(),
                    cin=w1.shape[1] if cin is None else cin, c=c, act=act, slope=slope, res=res, dd=_view(dd, d_coff), y=_view(y, out_coff), y_width=oc,
                    p=(_view(p1, p1_coff), _view(p2, p2_coff)))
    _run(L.OP_ASYM_STEP, d, x, "asym_step: no kernel for this shape (esr_asym_step_supported)")
    return dd, y


def prelu(srcs, slopes, *, out=None, out_coff=0):
    """esr_prelu: a per-channel nn.PReLU over the concat of up to four NHWC views in ONE streaming launch, fp32 / bf16 / fp16 tensors on the
    GPU: y[c] = v >= 0 ? v : slopes[c] * v, the product rounded once to the tensors' dtype.  srcs: [(tensor [N, H, W, P], first channel, channels),
    ...] (a bare tensor: all its channels) in the concat's order; slopes: fp32 [sum of the channels], any sign and size.
    out: a caller-provided NHWC tensor (pitch a multiple of the 16-byte granule) that receives y from channel out_coff, none of the sources;
    default: freshly allocated zeros of pitch round_up(channels, granule).  Returns y."""
    srcs = [(s, 0, s.shape[-1]) if isinstance(s, torch.Tensor) else tuple(s) for s in srcs]
    x = srcs[0][0]
    st, gran = _any_store(x, "prelu")
    if not 1 <= len(srcs) <= 4 or any(t.dtype != x.dtype or t.device != x.device or not t.is_contiguous() or tuple(t.shape[:3]) != tuple(x.shape[:3])
                                      for t, _, _ in srcs):
        raise L.EsrError("prelu: one to four contiguous NHWC tensors of one dtype, device and N x H x W")
    n, h, w, _ = x.shape
    ctot = sum(c for _, _, c in srcs)
    keep = pack_prelu(slopes).to(x.device)
    y = _zeros_or(out, "prelu: out", x, (n, h, w), (ctot + gran - 1) // gran * gran, gran)
    d = L.ConvDesc()
    descs.prelu(d, (n, h, w), L.STORE[st], srcs=[(_view(t, coff), c) for t, coff, c in srcs], a=keep.data_ptr(), y=_view(y, out_coff))
    _run(L.OP_PRELU, d, x, "prelu: esr_prelu does not take this descriptor (esr_prelu_supported)")
    return y


def resdb_step(x, a_e, w_e, b_e, a_c, w_c, b_c, *, extras=(), x_coff=0, d_out=None, d_coff=0, out=None, out_coff=0):
    """esr_resdb_step: one step of ResDN's block (team43_resdn.py:93-106) in ONE launch on 16-bit NHWC tensors: u = prelu(cat(x, extras), a_e),
    e = w_e . u + b_e (1x1, [48 + 16 nd, 48 + 16 nx, 1, 1]), dists = e[48:], t = prelu(e[:48], a_c) zero-padded, y = x + conv3x3(t, w_c) + b_c, with
    u, e[:48], t, dists and y rounded once to x's dtype.  x: [N, H, W, P] whose 48 channels from x_coff are read; extras: up to two
    (tensor, first channel) pairs of 16 channels each.  Returns (dists, y).  d_out / out: caller-provided NHWC tensors that receive dists / y
    from channel d_coff / out_coff; default: freshly allocated zeros."""
    st = _s16_store(x, "resdb_step")
    refusal = "resdb_step: no kernel for this shape (esr_resdb_step_supported: n = 48, d = 16, 1..3 distilled outputs, 0..2 extra inputs)"
    n, h, w, _ = x.shape
    nd, nx = w_e.shape[0] - 48, len(extras)
    w1 = w_e if w_e.dim() == 4 else w_e[:, :, None, None]
    if nd < 1 or w1.shape[1] != 48 + 16 * nx or a_e.numel() != 48 + 16 * nx or a_c.numel() != 48:
        raise L.EsrError(refusal)
    keep = [pack_conv_s16(w_c, b_c, st).to(x.device), pack_conv_s16(w1, b_e, st).to(x.device),
            pack_prelu(torch.cat([a_e.float().reshape(-1), a_c.float().reshape(-1)])).to(x.device)]
    dd = _zeros_or(d_out, "resdb_step: d_out", x, (n, h, w), nd, 8)
    y = _zeros_or(out, "resdb_step: out", x, (n, h, w), 48, 8)
    d = L.ConvDesc()
    descs.resdb_step(d, (n, h, w), L.STORE[st], x=_view(x, x_coff), extras=[_view(t, coff) for t, coff in extras], a=keep[2].data_ptr(),
                     w_e=keep[1].data_ptr(), w_c=keep[0].data_ptr(), cin=48, cout=48, extra_channels=16 * nx, dists=_view(dd, d_coff), dists_channels=nd,
                     y=_view(y, out_coff))
    _run(L.OP_RESDB_STEP, d, x, refusal)
    return dd, y


def conv_prelu(x, w, b, a, *, x_coff=0, out=None, out_coff=0):
    """esr_conv_prelu: a dense 64 -> 64 3x3 (zero padding) with the per-channel nn.PReLU behind it in ONE launch on 16-bit NHWC tensors:
    y[c] = prelu(conv3x3(x, w)[c] + b[c], a[c]) with prelu(v, a) = v >= 0 ? v : a v, fp32 accumulation, rounded once to x's dtype.  x: [N, H, W, P]
    whose 64 channels from x_coff are read; w: [64, 64, 3, 3], packed as the stand-alone convolution packs it; a: 64 fp32 slopes of any sign
    and size.  out: a caller-provided NHWC tensor that receives y from channel out_coff and shares no byte with x's channels; default:
    freshly allocated zeros.  Returns y."""
    st = _s16_store(x, "conv_prelu")
    refusal = "conv_prelu: no kernel for this shape (esr_conv_prelu_supported: 64 -> 64, 3x3, 16-bit storage)"
    n, h, wd, _ = x.shape
    if tuple(w.shape) != (64, 64, 3, 3) or a.numel() != 64:
        raise L.EsrError(refusal)
    keep = [pack_conv_s16(w, b, st).to(x.device), pack_prelu(a).to(x.device)]
    y = _zeros_or(out, "conv_prelu: out", x, (n, h, wd), 64, 8)
    d = L.ConvDesc()
    descs.conv_prelu(d, (n, h, wd), L.STORE[st], x=_view(x, x_coff), w=keep[0].data_ptr(), a=keep[1].data_ptr(), cin=64, cout=64, y=_view(y, out_coff))
    _run(L.OP_CONV_PRELU, d, x, refusal)
    return y


def mdsa_gate(f, x, w_f, b_f, a_f, w_s, b_s, *, f_coff=0, x_coff=0, out=None, out_coff=0):
    """esr_mdsa_gate: the end of an MDSA block (team24_mdgn.py:26-28) in ONE streaming launch on 16-bit NHWC tensors:
    y = prelu(w_f . cat(f1, f2, f3) + b_f, a_f) * sigmoid(w_s . x + b_s), the weights of the 192 -> 64 1x1 as hi + lo pairs, everything else
    fp32, one rounding to the tensors' dtype.  f: ONE tensor [N, H, W, P] whose 192 channels from f_coff are cat(f1, f2, f3), or a stacked
    tensor [3, N, H, W, P] whose three dense tensors hold f1, f2, f3 in their 64 channels from f_coff (what a plan's planar concat is).
    x: [N, H, W, Q], 64 channels from x_coff.  out: a caller-provided NHWC tensor that receives y from channel out_coff, another tensor than
    f and x; default: freshly allocated zeros.  Returns y."""
    st = _s16_store(x, "mdsa_gate")
    n, h, w, _ = x.shape
    planar = f.dim() == 5
    if not f.is_cuda or f.dtype != x.dtype or not f.is_contiguous() or not x.is_contiguous() or tuple(f.shape[-4:-1]) != (n, h, w) or (planar and f.shape[0] != 3):
        raise L.EsrError("mdsa_gate: f [N, H, W, P] or [3, N, H, W, P] and x [N, H, W, Q], contiguous, one dtype and device")
    keep = pack_mdsa_gate(w_f, b_f, a_f, w_s, b_s, st).to(x.device)
    y = _zeros_or(out, "mdsa_gate: out", x, (n, h, w), 64, 8)
    d = L.ConvDesc()
    descs.mdsa_gate(d, (n, h, w), L.STORE[st], f=_view(f, f_coff), x=_view(x, x_coff), w=keep.data_ptr(), cin=192, cout=64, y=_view(y, out_coff),
                    seg=(f.stride(0) * f.element_size(), 4) if planar else None)
    _run(L.OP_MDSA_GATE, d, x, "mdsa_gate: esr_mdsa_gate does not take this descriptor (esr_mdsa_gate_supported)")
    return y


def resblock_head(x, w1, b1, w2, b2, wc, bc, *, g=None, in_coff=0, g_coff=0, x_out=None, x_coff=0, u_out=None, u_coff=0,
                  c1_out=None, c1_coff=0, c1_channels=None):
    """esr_resblock_head_s16: the head of ESAN's residual block (team34_esan.py:71-76, :49) in ONE launch on 16-bit NHWC tensors of 32
    channels: xs = x + g (g given; else xs = x and nothing is stored for it), t = relu(conv3x3(xs, w1, b1)), u = conv3x3(t, w2, b2) with t
    as rounded and zero-padded, c1 = wc . u + bc on u as stored.  Returns (xs or None, u, c1).
    x_out / u_out / c1_out: caller-provided NHWC tensors of x's dtype and device (pitch a multiple of 8) that receive xs / u / c1 from channel
    x_coff / u_coff / c1_coff; default: freshly allocated zeros (c1: pitch 16, the ESA map).  c1_channels: esr_conv_desc.post_cout, the
    stored width (default: the logical one; round_up(.., 8) channels are written, the pad ones as zeros)."""
    st = _s16_store(x, "resblock_head")
    n, h, w, _ = x.shape
    wc4 = wc if wc.dim() == 4 else wc[:, :, None, None]
    c, f = w1.shape[1], (wc4.shape[0] if c1_channels is None else c1_channels)
    keep = [pack_conv_s16(w1, b1, st).to(x.device), pack_conv_s16(w2, b2, st).to(x.device), pack_conv_s16(wc4, bc, st).to(x.device)]
    xs = None if g is None else _zeros_or(x_out, "resblock_head: x_out", x, (n, h, w), c, 8)
    u = _zeros_or(u_out, "resblock_head: u_out", x, (n, h, w), c, 8)
    c1 = _zeros_or(c1_out, "resblock_head: c1_out", x, (n, h, w), (f + 7) // 8 * 8, 8, pitch=L.ESA_FP)
    d = L.ConvDesc()
    descs.resblock_head(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), g=_view(g, g_coff), xs=_view(xs, x_coff), w1=keep[0].data_ptr(),
                        w2=keep[1].data_ptr(), wc=keep[2].data_ptr(), cin=c, cout=w2.shape[0], u=_view(u, u_coff), c1=_view(c1, c1_coff), c1_width=f)
    _run(L.OP_RESBLOCK_HEAD, d, x, "resblock_head: no kernel for this shape (esr_resblock_head_supported)")
    return xs, u, c1


def refine_cascade(d2, w2r, b2r, w3d, b3d, w3r, b3r, w4, b4, *, slope=0.05, in_coff=0, d3_out=None, d3_coff=0, r4_out=None, r4_coff=0,
                   store=None):
    """esr_refine_cascade_s16: the narrowing refinement path of FasterRFDN's block (team25_frfdn/block.py:115-122) in ONE launch on a 16-bit
    NHWC tensor d2 [N, H, W, P] (32 channels from in_coff): r2 = lrelu(conv3x3(d2, w2r, b2r) + d2), d3 = lrelu(w3d . r2 + b3d),
    r3 = lrelu(conv3x3(d3, w3r, b3r) + d3), r4 = lrelu(conv3x3(r3, w4, b4) + r3), every tensor as rounded to the storage type and
    zero-padded.  Returns (d3, r4), 16 channels each.
    d3_out / r4_out: caller-provided NHWC tensors of d2's dtype and device (pitch a multiple of 8) that receive d3 / r4 from channel d3_coff /
    r4_coff -- they may be one tensor (offsets 0 and 16 of a pitch-32 concat segment), never d2's; default: freshly allocated zeros of
    pitch 16.  store: "bf16" | "f16", if given it must be d2's storage type."""
    st = _s16_store(d2, "refine_cascade")
    if store is not None and store != st:
        raise L.EsrError(f"refine_cascade: store {store!r}, d2 is stored as {st}")
    n, h, w, _ = d2.shape
    w1 = w3d if w3d.dim() == 4 else w3d[:, :, None, None]
    cmid, cout = w1.shape[0], w4.shape[0]
    keep = [pack_conv_s16(wt, b, st).to(d2.device) for wt, b in ((w2r, b2r), (w1, b3d), (w3r, b3r), (w4, b4))]
    d3 = _zeros_or(d3_out, "refine_cascade: d3_out", d2, (n, h, w), (cmid + 7) // 8 * 8, 8)
    r4 = _zeros_or(r4_out, "refine_cascade: r4_out", d2, (n, h, w), (cout + 7) // 8 * 8, 8)
    d = L.ChainDesc()
    descs.refine_cascade(d, (n, h, w), L.STORE[st], d2=_view(d2, in_coff), w=[k.data_ptr() for k in keep], cin=w2r.shape[1], cmid=cmid, cout=cout,
                         slope=slope, d3=_view(d3, d3_coff), d3_width=cmid, r4=_view(r4, r4_coff), r4_width=cout)
    _run(L.OP_REFINE_CASCADE, d, d2, "refine_cascade: no kernel for this shape (esr_refine_cascade_supported)")
    return d3, r4


def dwconv7x7(x, weight, bias, *, in_coff=0, out=None, out_coff=0, packed=None):
    """esr_dwconv7x7: depthwise nn.Conv2d(C, C, 7, 1, 3, groups=C) with zero padding and bias on an NHWC tensor x [N, H, W, P] (C channels
    from in_coff) in fp32, bf16 or fp16 storage: fp32 sums in (ky, kx) ascending order, the bias last, one rounding.  weight [C, 1, 7, 7].
    out: a caller-provided NHWC tensor of x's dtype and device (another tensor than x) that receives the result from channel out_coff;
    default: freshly allocated zeros of pitch round_up(C, granule).  The pad channels up to the granule (4 fp32 / 8 16-bit) are stored as zeros."""
    st, gran = _any_store(x, "dwconv7x7")
    n, h, w, _ = x.shape
    c = weight.shape[0]
    keep = pack_dw7(weight, bias).to(x.device) if packed is None else packed
    y = _zeros_or(out, "dwconv7x7: out", x, (n, h, w), (c + gran - 1) // gran * gran, gran)
    d = L.ConvDesc()
    descs.dwconv7x7(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), w=keep.data_ptr(), c=c, y=_view(y, out_coff))
    _run(L.OP_DWCONV7, d, x, "dwconv7x7: no kernel for this shape (esr_dwconv7x7_supported)")
    return y


def cx_block(v, w0, b0, w1, b1, w2, b2, *, slope=0.05, in_coff=0, out=None, out_coff=0, out_channels=None, store=None):
    """esr_cx_block_s16: a ConvNeXt block (team38_rfdnext/rfdn_block.py:132-144) in ONE launch on a 16-bit NHWC tensor v [N, H, W, P] (C
    channels from in_coff): t = dw7(v, w0, b0), h = lrelu(w1 . t + b1), out = w2 . h + b2 + v, each of t, h and out rounded once to the
    storage type, v zero-padded.  w0 [C, 1, 7, 7], w1 [M, C(, 1, 1)], w2 [C, M(, 1, 1)]; 33 <= C <= 64, 129 <= M <= 256.
    out: a caller-provided NHWC tensor of v's dtype and device, never v itself, that receives the result from channel out_coff; default:
    freshly allocated zeros of pitch round_up(C, 8).  out_channels: the channels stored (default round_up(C, 8); those >= C are zeros).
    store: "bf16" | "f16", if given it must be v's storage type."""
    st = _s16_store(v, "cx_block")
    if store is not None and store != st:
        raise L.EsrError(f"cx_block: store {store!r}, v is stored as {st}")
    n, h, w, _ = v.shape
    cout = w2.shape[0]
    keep = [pack_dw7(w0, b0).to(v.device)] + [p.to(v.device) for p in pack_cx_pw(w1, b1, w2, b2, st)]
    width = (cout + 7) // 8 * 8 if out_channels is None else out_channels
    y = _zeros_or(out, "cx_block: out", v, (n, h, w), width, 8)
    d = L.ChainDesc()
    descs.cx_block(d, (n, h, w), L.STORE[st], v=_view(v, in_coff), w0=keep[0].data_ptr(), w1=keep[1].data_ptr(), w2=keep[2].data_ptr(), c=w0.shape[0],
                   m=w1.shape[0], cout=cout, slope=slope, out=_view(y, out_coff), out_width=width)
    _run(L.OP_CX_BLOCK, d, v, "cx_block: no kernel for this shape (esr_cx_block_supported)")
    return y


def dwconv3x3(x, weight, bias, *, act=L.ACT_NONE, slope=0.05, res=None, res_mode=L.RES_NONE, in_coff=0, res_coff=0, out=None, out_coff=0):
    """esr_dwconv3x3_f32: depthwise nn.Conv2d(C, C, 3, 1, 1, groups=C) with zero padding and bias on an NHWC tensor x [N, H, W, P] (C channels
    from in_coff) in fp32, bf16 or fp16 storage, + res before / behind the activation (res_mode).  weight [C, 1, 3, 3].
    out: a caller-provided NHWC tensor of x's dtype and device (another tensor than x) that receives round_up(C, 4) channels from out_coff;
    default: freshly allocated zeros of pitch round_up(C, granule)."""
    st, gran = _any_store(x, "dwconv3x3")
    n, h, w, _ = x.shape
    c = weight.shape[0]
    keep = pack_dw(weight, bias).to(x.device)
    y = _zeros_or(out, "dwconv3x3: out", x, (n, h, w), (c + gran - 1) // gran * gran, gran)
    d = L.ConvDesc()
    descs.dwconv3x3(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), w=keep.data_ptr(), c=c, act=act, slope=slope, y=_view(y, out_coff),
                    res=_view(res, res_coff), res_mode=res_mode)
    _run(L.OP_DWCONV, d, x, None)
    return y


def dwpw_pair(x, wda, bda, wa, ba, wdb, bdb, wb, bb, *, slope=0.05, in_coff=0, out=None, out_coff=0, out_channels=None, store=None):
    """esr_dwpw_pair_s16: the refinement path of team 35's RFDB (team35_rfdn/rmsrb1.py:22-27, :199-210) in ONE launch on a 16-bit NHWC tensor
    x [N, H, W, P] (C channels from in_coff): u1 = dw3(x, wda, bda) + x, h = relu(wa . u1 + ba), u2 = dw3(h, wdb, bdb) + h,
    out = lrelu(wb . u2 + bb + x), each of u1, h, u2 and out rounded once to the storage type, x and h zero-padded.  wda / wdb [C, 1, 3, 3],
    wa / wb [C, C(, 1, 1)]; 33 <= C <= 64.
    out: a caller-provided NHWC tensor of x's dtype and device, never x itself, that receives the result from channel out_coff; default:
    freshly allocated zeros of pitch round_up(C, 8).  out_channels: the channels stored (default round_up(C, 8); those >= C are zeros).
    store: "bf16" | "f16", if given it must be x's storage type."""
    st = _s16_store(x, "dwpw_pair")
    if store is not None and store != st:
        raise L.EsrError(f"dwpw_pair: store {store!r}, x is stored as {st}")
    refusal = "dwpw_pair: no kernel for this shape (esr_dwpw_pair_supported)"
    n, h, w, _ = x.shape
    c = wda.shape[0]
    if not L.lib().esr_packed_cx_pw1_bytes(c, c):
        raise L.EsrError(refusal)
    keep = [pack_dw(wda, bda).to(x.device), pack_dwpw_pw(wa, ba, st).to(x.device), pack_dw(wdb, bdb).to(x.device), pack_dwpw_pw(wb, bb, st).to(x.device)]
    width = (c + 7) // 8 * 8 if out_channels is None else out_channels
    y = _zeros_or(out, "dwpw_pair: out", x, (n, h, w), width, 8)
    d = L.ChainDesc()
    descs.dwpw_pair(d, (n, h, w), L.STORE[st], x=_view(x, in_coff), w=[k.data_ptr() for k in keep], c=c, slope=slope, out=_view(y, out_coff), out_width=width)
    _run(L.OP_DWPW_PAIR, d, x, refusal)
    return y


def _pa(what, t, weight, bias, s, pair_out, in_coff, s_coff, out, out_coff, out_channels):
    """the descriptor esr_pa_gate and esr_pa_tail share -> (desc, y, the blob to keep alive)"""
    st, gran = _any_store(t, what)
    n, h, w, _ = t.shape
    c = weight.shape[0]
    width = (c + gran - 1) // gran * gran if out_channels is None else out_channels
    hilo, strides = 0, set()
    if s is not None:
        pair = s.dim() == 5
        if s.device != t.device or s.dtype != t.dtype or not s.is_contiguous() or tuple(s.shape[:-1]) != ((2,) if pair else ()) + (n, h, w):
            raise L.EsrError(f"{what}: s must be a contiguous [{'2, ' if pair else ''}{n}, {h}, {w}, pitch] tensor of t's dtype on t's device")
        if pair:
            hilo |= L.HILO_RES
            strides.add(s[1].data_ptr() - s[0].data_ptr())
    if not L.lib().esr_packed_pa_gate_bytes(c, L.STORE[st]) or tuple(weight.shape[:2]) != (c, c):
        raise L.EsrError(f"{what}: no kernel for this shape (a square 1x1 of 33 .. 64 channels)")
    keep = pack_pa_gate(weight, bias, st).to(t.device)
    y = _zeros_or(out, f"{what}: out", t, ((2,) if pair_out else ()) + (n, h, w), width, gran)
    if pair_out:
        hilo |= L.HILO_OUT
        strides.add(y[1].data_ptr() - y[0].data_ptr())
    if len(strides) > 1:
        raise L.EsrError(f"{what}: a pair s and a pair result must have one pitch")
    d = L.ConvDesc()
    descs.pa_gate(d, (n, h, w), L.STORE[st], t=_view(t, in_coff), w=keep.data_ptr(), c=c, y=_view(y, out_coff), y_width=width, s=_view(s, s_coff),
                  hilo=hilo, hilo_stride=strides.pop() if strides else 0)
    return d, y, keep


def pa_gate(t, weight, bias, *, s=None, pair_out=False, in_coff=0, s_coff=0, out=None, out_coff=0, out_channels=None):
    """esr_pa_gate: y = t * sigmoid(weight . t + bias) (+ s) -- a pixel attention (team10_repafdn/block.py:151-166) and the tensor added behind
    it -- in ONE launch on an NHWC tensor t [N, H, W, P] (C channels from in_coff) in fp32, bf16 or fp16 storage.  weight [C, C(, 1, 1)],
    33 <= C <= 64; the product and the sum are fp32, one rounding at the store.
    s: None, an NHWC tensor [N, H, W, Ps] of t's dtype (C channels from s_coff), or -- 16-bit storage -- a hi + lo pair [2, N, H, W, Ps]
    (s = hi + lo in fp32).  pair_out (16-bit storage): y is returned as such a pair [2, N, H, W, Py], hi = rnd(v), lo = rnd(v - hi); with a
    pair s as well the two must have one pitch (the C ABI has one stride for both).
    out: a caller-provided tensor of t's dtype and device, never t or s, that receives the result from channel out_coff; default: freshly
    allocated zeros of pitch round_up(C, granule).  out_channels: the channels stored (default round_up(C, granule), granule 4 fp32 / 8
    16-bit; those >= C are zeros)."""
    d, y, keep = _pa("pa_gate", t, weight, bias, s, pair_out, in_coff, s_coff, out, out_coff, out_channels)
    _run(L.OP_PA_GATE, d, t, "pa_gate: no kernel for this shape (esr_pa_gate_supported)")
    return y


def pa_tail(x, w3, b3, weight, bias, *, s=None, pair_out=False, in_coff=0, s_coff=0, out=None, out_coff=0, out_channels=None):
    """esr_pa_tail: t = conv3x3(x, w3, b3) (zero padding), y = t * sigmoid(weight . rnd(t) + bias) (+ s) in ONE launch on a 16-bit NHWC
    tensor x [N, H, W, P] (C channels from in_coff): t stays in fp32 and is never stored, only the gate's matrix operand is t rounded to the
    storage type.  w3 [C, C, 3, 3], weight [C, C(, 1, 1)], 33 <= C <= 64.  s, pair_out, out, out_coff, out_channels: as ops.pa_gate; out is
    never x (neighbouring tiles read its halo) or s."""
    _s16_store(x, "pa_tail")
    d, y, keep = _pa("pa_tail", x, weight, bias, s, pair_out, in_coff, s_coff, out, out_coff, out_channels)
    c = d.cin
    if tuple(w3.shape) != (c, c, 3, 3):
        raise L.EsrError(f"pa_tail: w3 must be [{c}, {c}, 3, 3]")
    keep3 = pack_conv_s16(w3, b3, _STORE_OF[x.dtype], cin_phys=(c + 15) // 16 * 16).to(x.device)
    descs.pa_tail(d, x=_view(x, in_coff), w3=keep3.data_ptr(), w=keep.data_ptr())
    _run(L.OP_PA_TAIL, d, x, "pa_tail: no kernel for this shape (esr_pa_tail_supported)")
    return y


def esa_unshuffle(c1, weight, bias, *, out=None):
    """esr_esa_unshuffle_f32: c3 = relu(con_(relu(max_pool2d(pixel_unshuffle(c1, 2), 7, 3)))) (team35_rfdn/rmsrb1.py:140-144) in one launch.
    c1: the conv1 map [N, H, W, 16] in fp32, bf16 or fp16 storage (f channels, the rest ignored), H, W >= 14; weight [f, 4 f, 1, 1] and bias
    of con_ = nn.Conv2d(4 f, f, 1, padding 1).  Returns the fp32 map [N, h3 + 2, w3 + 2, 16], h3 = (H // 2 - 7) // 3 + 1: the ring is
    relu(bias), the pad channels f .. 15 are zeros.  out: a caller-provided contiguous fp32 tensor of that shape on c1's device."""
    st, _ = _any_store(c1, "esa_unshuffle")
    n, h, w, _ = c1.shape
    if h < 14 or w < 14:
        raise L.EsrError("esa_unshuffle: H, W >= 14 (one 7x7 pooling window of the half-resolution map)")
    lo = (h // 2 - 7) // 3 + 3, (w // 2 - 7) // 3 + 3
    keep = pack_unshuffle(weight, bias).to(c1.device)
    like = torch.empty(0, dtype=torch.float32, device=c1.device)
    y = _zeros_or(out, "esa_unshuffle: out", like, (n,) + lo, L.ESA_FP, 4)
    d = L.EsaDesc()
    descs.esa_unshuffle(d, (n, h, w), L.STORE[st], c1=_view(c1), w=keep.data_ptr(), f=weight.shape[0], y=_view(y), lo=lo)
    _run(L.OP_ESA_UNSHUFFLE, d, c1, None)
    return y


def _hilo_pair(t, what, strides):
    """checks a hi + lo pair [2, N, H, W, P] (bf16, P a multiple of 16) and records the byte stride between its halves"""
    if t.dtype != torch.bfloat16 or t.shape[-1] % 16:
        raise L.EsrError(f"conv2d: a hi + lo {what} is a bf16 pair with a pixel pitch that is a multiple of 16 channels")
    strides.append(t.stride(0) * t.element_size())


def tensor2uint_device(img_sr, data_range, nonfinite=None, *, out=None):
    """utils_image.tensor2uint on the GPU: [1,C,H,W] (or [C,H,W]) fp32 -> HWC uint8 tensor on the same device.
    nonfinite: optional 1-element int32 DEVICE tensor (caller-zeroed) that the kernel ORs 1 into when the image holds an Inf / NaN
    (esr_tensor2uint_u8_chk) -- the harness's overflow check without a full-size isfinite pass.
    out: caller-provided contiguous uint8 [H, W, C] tensor on the same device (default: a fresh one); EsrError otherwise."""
    if not img_sr.is_cuda:
        raise L.EsrError("tensor2uint_device: tensor must live on the GPU")
    t = img_sr.detach()
    if t.dim() == 4:
        assert t.shape[0] == 1, "one image at a time, like the reference's run()"
        t = t[0]
    t = t.contiguous().float()
    c, h, w = t.shape
    if out is None:
        out = torch.empty((h, w, c), dtype=torch.uint8, device=t.device)
    elif out.dtype != torch.uint8 or out.device != t.device or tuple(out.shape) != (h, w, c) or not out.is_contiguous():
        raise L.EsrError(f"tensor2uint_device: out must be a contiguous uint8 [{h}, {w}, {c}] tensor on {t.device}")
    stream = torch.cuda.current_stream(t.device).cuda_stream
    if nonfinite is not None:
        assert nonfinite.is_cuda and nonfinite.dtype == torch.int32 and nonfinite.numel() == 1
        L.check(L.lib().esr_tensor2uint_u8_chk(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()), c, h, w, ctypes.c_float(data_range),
                                               ctypes.c_void_p(nonfinite.data_ptr()), ctypes.c_void_p(stream)), "esr_tensor2uint_u8_chk")
        return out
    L.check(L.lib().esr_tensor2uint_u8(ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()), c, h, w,
                                       ctypes.c_float(data_range), ctypes.c_void_p(stream)), "esr_tensor2uint_u8")
    return out


def ssim_sum_device(a_u8, b_u8, border=0, *, partials=None):
    """calculate_ssim's numerator on the GPU (utils/utils_image.py:509-554, esr_ssim_u8): the SSIM map of two HWC (or HW) uint8 CUDA
    tensors summed over the 'valid' region of the border-cropped image and all channels, as a 0-dim float64 DEVICE tensor (no host
    synchronisation), and the number of map elements it was summed over.  ssim = sum / count.
    partials: caller-provided float64 [esr_ssim_partials(h, w, c, border)] tensor on the same device for the per-block sums (every entry is
    written; default: a fresh one); EsrError otherwise."""
    if a_u8.shape != b_u8.shape:
        raise ValueError('Input images must have the same dimensions.')
    a, b = a_u8.contiguous(), b_u8.contiguous()
    h, w = a.shape[:2]
    c = a.shape[2] if a.dim() == 3 else 1
    if a.dim() not in (2, 3) or c not in (1, 3):
        raise ValueError('Wrong input image dimensions.')
    n = int(L.lib().esr_ssim_partials(h, w, c, border))
    if n == 0:
        raise L.EsrError(f"ssim_device: a {h}x{w} image cropped by {border} is smaller than the 11x11 window")
    if partials is None:
        partials = torch.empty(n, dtype=torch.float64, device=a.device)
    elif partials.dtype != torch.float64 or partials.device != a.device or tuple(partials.shape) != (n,) or not partials.is_contiguous():
        raise L.EsrError(f"ssim_sum_device: partials must be a contiguous float64 [{n}] tensor on {a.device}")
    stream = torch.cuda.current_stream(a.device).cuda_stream
    L.check(L.lib().esr_ssim_u8(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), h, w, c, border,
                                ctypes.c_void_p(partials.data_ptr()), n, ctypes.c_void_p(stream)), "esr_ssim_u8")
    return partials.sum(), (h - 2 * border - 10) * (w - 2 * border - 10) * c


def ssim_device(a_u8, b_u8, border=0):
    """calculate_ssim for two uint8 CUDA tensors: one scalar D2H.  Parity: pinned to image_util.calculate_ssim (the reference's needs
    cv2, absent in the authoring container: PARITY-UNPINNED against the reference itself)."""
    s, count = ssim_sum_device(a_u8, b_u8, border)
    return float(s.item()) / count


def sqerr_device(a_u8, b_u8, border=0, *, out=None):
    """sum over the border-cropped region of (a - b)^2 for two HWC uint8 CUDA tensors as a 1-element int64 DEVICE tensor:
    no host synchronisation (the harness pipeline reads it when the image retires).
    out: caller-provided 1-element int64 tensor on the same device (default: a fresh one); EsrError otherwise."""
    a, b = a_u8.contiguous(), b_u8.contiguous()
    h, w = a.shape[:2]
    c = a.shape[2] if a.dim() == 3 else 1
    if out is None:
        acc = torch.empty(1, dtype=torch.int64, device=a.device)
    elif out.dtype != torch.int64 or out.device != a.device or out.numel() != 1:
        raise L.EsrError(f"sqerr_device: out must be a 1-element int64 tensor on {a.device}")
    else:
        acc = out
    stream = torch.cuda.current_stream(a.device).cuda_stream
    L.check(L.lib().esr_sqerr_u8(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), h, w, c, border,
                                 ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(stream)), "esr_sqerr_u8")
    return acc


def psnr_device(a_u8, b_u8, border=0):
    """calculate_psnr for two HWC uint8 CUDA tensors: exact integer squared-error sum on the device, one scalar D2H."""
    import math
    if a_u8.shape != b_u8.shape:
        raise ValueError('Input images must have the same dimensions.')
    a, b = a_u8.contiguous(), b_u8.contiguous()
    h, w = a.shape[:2]
    c = a.shape[2] if a.dim() == 3 else 1
    acc = torch.empty(1, dtype=torch.int64, device=a.device)
    stream = torch.cuda.current_stream(a.device).cuda_stream
    L.check(L.lib().esr_sqerr_u8(ctypes.c_void_p(a.data_ptr()), ctypes.c_void_p(b.data_ptr()), h, w, c, border,
                                 ctypes.c_void_p(acc.data_ptr()), ctypes.c_void_p(stream)), "esr_sqerr_u8")
    se = int(acc.item())
    count = (h - 2 * border) * (w - 2 * border) * c
    if se == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(se / count))


def bsconv(x, pw_weight, pw_bias, dw_weight, dw_bias, *, act=L.ACT_NONE, slope=0.05, res=None, res_mode=L.RES_NONE,
           in_coff=0, cin=None, d_weight=None, d_bias=None, d_act=L.ACT_NONE, out=None, d_out=None):
    """BSConvU in one launch (esr_bsconv_f32): act(dw3x3(pw1x1(x)) [+ res]); returns y, or (y, distilled) when the
    distillation 1x1 `d_weight` [d_cout, cin] is given.  x: NHWC [N,H,W,pitch] fp32 / bfloat16 / float16 (the storage
    type of the op: res and the outputs have the same dtype); pw_weight [c, cin]; dw_weight [c,1,3,3].
    out / d_out: caller-provided NHWC [N,H,W,pitch] tensors for y / the distilled output (x's dtype and device, pitch a multiple of 4 that
    holds the channels, written from channel 0; EsrError otherwise); default: freshly allocated zeros."""
    from .engine import pack_dw
    if not x.is_cuda:
        raise L.EsrError("bsconv: tensors must live on the GPU; there is no CPU fallback")
    lib = L.lib()
    st = _STORE_OF[x.dtype]
    n, h, w, _ = x.shape
    c, wcin = pw_weight.shape[0], pw_weight.shape[1]
    cin = wcin if cin is None else cin

    def pk(wt, b):
        w4 = wt.reshape(wt.shape[0], wcin, 1, 1)
        return (pack_conv(w4, b) if st == "f32" else pack_conv_s16(w4, b, st)).to(x.device)

    keep = [pk(pw_weight, pw_bias), pack_dw(dw_weight, dw_bias).to(x.device)]
    d = L.BsDesc()
    d.storage = L.STORE[st]
    d.n, d.h, d.w, d.cin, d.c = n, h, w, cin, c
    d.act, d.slope, d.res_mode = act, slope, res_mode
    d.inp = _view(x, in_coff)
    y = _zeros_or(out, "bsconv: out", x, (n, h, w), (c + 3) // 4 * 4, 4)
    d.out = _view(y)
    if d_out is not None and d_weight is None:
        raise L.EsrError("bsconv: d_out without d_weight")
    if res is not None:
        d.res = _view(res)
    d.pw_packed, d.dw_packed = ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr())
    yd = None
    if d_weight is not None:
        dco = d_weight.shape[0]
        keep.append(pk(d_weight, d_bias))
        yd = _zeros_or(d_out, "bsconv: d_out", x, (n, h, w), (dco + 3) // 4 * 4, 4)
        d.d_packed, d.d_cout, d.d_act, d.d_out = ctypes.c_void_p(keep[2].data_ptr()), dco, d_act, _view(yd)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _launch(L.OP_BSCONV, d, stream)
    return y if yd is None else (y, yd)


def channel_attention(x, w1, b1, w2, b2, *, contrast=False, nchw=False, out=None, coff=0, out_coff=0):
    """CALayer / CCALayer (esr_channel_attention_f32): y = x * sigmoid(W2 . relu(W1 . s + b1) + b2) with s = mean over H, W
    (contrast=False, models/basicblock.py:333-348) or std + mean (contrast=True, models/team05_efdn/plainblock.py:106-122).
    x: NHWC [N,H,W,pitch] (fp32 / bf16 / fp16) or, with nchw=True, NCHW fp32 [N,C,H,W]; w1 [cr, c(,1,1)], w2 [c, cr(,1,1)].
    coff / out_coff (NHWC): first channel of the slice of x that is read / of `out` that is written (multiples of 4; the slice is
    round_up(c, 4) channels wide and must fit the pitch: the library returns ESR_ERR_BAD_ARG otherwise).  `out`: caller-provided tensor of
    x's dtype, device and leading dims (NHWC: any pitch that is a multiple of 4 and holds the slice; NCHW: x's shape); default zeros_like(x)."""
    from .engine import pack_dense
    if not x.is_cuda:
        raise L.EsrError("channel_attention: tensors must live on the GPU; there is no CPU fallback")
    cr, c = w1.shape[0], w1.shape[1]
    c4 = (c + 3) // 4 * 4
    if nchw:
        n, _, h, w = x.shape
    else:
        n, h, w, _ = x.shape
    keep = [pack_dense(w1.reshape(cr, c, 1, 1), b1, c, cr).to(x.device), pack_dense(w2.reshape(c, cr, 1, 1), b2, cr, c4).to(x.device)]
    if nchw and (coff or out_coff):
        raise L.EsrError("channel_attention: channel offsets are for NHWC views")
    if out is None:
        y = torch.zeros_like(x)
    elif nchw:
        if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
            raise L.EsrError("channel_attention: an NCHW `out` has x's shape, dtype and device")
        y = out
    else:
        y = _provided(out, "channel_attention: out", x, (n, h, w), out_coff + c4, 4)
    stats = torch.empty(n * 2 * c4, dtype=torch.float64, device=x.device)
    d = L.CaDesc()
    d.n, d.h, d.w, d.c, d.cr, d.contrast = n, h, w, c, cr, int(contrast)
    d.layout = L.NCHW_IN if nchw else L.NHWC
    d.storage = L.STORE[_STORE_OF[x.dtype]]
    d.x = L.View(ctypes.c_void_p(x.data_ptr()), 0 if nchw else x.shape[-1], coff)
    d.y = L.View(ctypes.c_void_p(y.data_ptr()), 0 if nchw else y.shape[-1], out_coff)
    d.w1, d.w2, d.stats = keep[0].data_ptr(), keep[1].data_ptr(), stats.data_ptr()
    stream = torch.cuda.current_stream(x.device).cuda_stream
    L.check(L.lib().esr_channel_attention_f32(ctypes.byref(d), ctypes.c_void_p(stream)), "esr_channel_attention_f32")
    return y


def esa_apply(x, c1, c3, wf, bf, w4, b4, *, out=None, post=None, skip_y=False, post_out=None, x_coff=0, out_coff=0):
    """ESA's full-resolution tail in one launch (esr_esa_apply_f32): y = x * sigmoid(conv4(bilinear(c3 -> HxW) + conv_f(c1)))
    (models/rfdn_baseline/block.py:124-129).  x: NHWC [N,H,W,pitch] (fp32 / bf16 / fp16 storage), c channels = w4.shape[0];
    c1: NHWC [N,H,W,16] of the same dtype (conv1's output, f = wf.shape[0] <= 16 channels, pads zero); c3: fp32 NHWC [N,h_lo,w_lo,16];
    wf [f,f(,1,1)], w4 [c,f(,1,1)].
    W >= 8: the kernels carry a 16-pixel group's column over at most two image rows; a narrower image raises EsrError (esr_esa_apply_f32
    returns ESR_ERR_UNSUPPORTED) before anything is launched, in every storage type.
    x_coff / out_coff: x is read from channel x_coff of its pitch, y written from channel out_coff of `out`'s (multiples of 4 for fp32, 8 for
    16-bit storage); nothing outside [out_coff, out_coff + round_up(c, granule)) of a pixel is written.
    post (16-bit storage): one or two dicts(weight [cout, cin(,1,1)], bias, act, slope, res) -- 1x1 convolutions evaluated in the same
    launch (esr_esa_desc.post[]): the first on y as stored (+ res, NHWC of x's dtype), the second on the first's fp32 result.  Returns
    (y, [out0(, out1)]) then; skip_y: y is not stored.
    post_out: a list with one caller-provided NHWC [N,H,W,pitch] tensor per post (x's dtype and device, pitch a multiple of 8 that holds the
    post's channels, written from channel 0; EsrError otherwise); default: freshly allocated zeros."""
    from .engine import pack_apply_post, pack_dense
    if not x.is_cuda:
        raise L.EsrError("esa_apply: tensors must live on the GPU; there is no CPU fallback")
    n, h, w, pitch = x.shape
    c, f = w4.shape[0], wf.shape[0]
    cp4 = (c + 3) // 4 * 4
    keep = [pack_dense(wf.reshape(f, f, 1, 1), bf, 16, 16).to(x.device), pack_dense(w4.reshape(c, f, 1, 1), b4, 16, cp4).to(x.device)]
    y = torch.zeros_like(x) if out is None else out
    d = L.EsaDesc()
    d.n, d.h, d.w, d.c, d.f, d.h_lo, d.w_lo = n, h, w, c, f, c3.shape[1], c3.shape[2]
    d.storage = L.STORE[_STORE_OF[x.dtype]]
    d.x, d.y = _view(x, x_coff), _view(y, out_coff)
    d.c1, d.c3, d.w0, d.w1 = c1.data_ptr(), c3.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr()
    outs = []
    if post_out is not None and (not post or len(post_out) != len(post)):
        raise L.EsrError("esa_apply: post_out needs one tensor per post")
    if post:
        p0, p1 = post[0], (post[1] if len(post) > 1 else None)
        keep.append(pack_apply_post(p0["weight"], p0.get("bias"), None if p1 is None else p1["weight"], None if p1 is None else p1.get("bias"),
                                    _STORE_OF[x.dtype]).to(x.device))
        d.post_w = keep[-1].data_ptr()
        d.skip_y = 1 if skip_y else 0
        for k, t in enumerate(post):
            co = t["weight"].shape[0]
            o = _zeros_or(None if post_out is None else post_out[k], f"esa_apply: post_out[{k}]", x, (n, h, w), (co + 7) // 8 * 8, 8)
            outs.append(o)
            pp = d.post[k]
            pp.cout, pp.act, pp.slope = co, t.get("act", L.ACT_NONE), t.get("slope", 0.05)
            pp.out = _view(o)
            if t.get("res") is not None:
                pp.res_mode, pp.res = L.RES_PRE_ACT, _view(t["res"])
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _launch(L.OP_ESA_APPLY, d, stream)
    return (y, outs) if post else y


# ---- torch.library operators over the kernels --------------------------------------------------------------------------------
# The "thin PyTorch-ROCm custom-op layer" of BASELINE.json's north star at KERNEL granularity (engine.py registers the whole-network
# op esr::sr_forward): every hot kernel family is a registered operator with a fake (shape) implementation, so FakeTensor tracing /
# torch.compile / export see opaque ops instead of ctypes calls.  Real implementations = the functions above; tensors are NHWC views
# as the C ABI sees them.  These replace nn.Conv2d + activation (+ residual) (models/basicblock.py:61-98), BSConvU
# (models/team18_bsrn.py:44-88), the ESA tail (models/rfdn_baseline/block.py:124-129) and CALayer / CCALayer
# (models/basicblock.py:333-348, models/team05_efdn/plainblock.py:106-122).
from typing import Optional  # noqa: E402

Tensor = torch.Tensor


def _pad_c(c, dtype):
    g = 4 if dtype == torch.float32 else 8
    return (c + g - 1) // g * g


@torch.library.custom_op("esr::conv2d", mutates_args=())
def conv2d_op(x: Tensor, weight: Tensor, bias: Optional[Tensor], act: int, slope: float, res: Optional[Tensor], res_mode: int,
              winograd: bool) -> Tensor:
    """act(conv(x) [+ res]) on NHWC x [N,H,W,pitch >= cin]; weight OIHW (k = 1 | 3); returns NHWC [N,H,W,pad(cout)].
    winograd: fp32 3x3 as Winograd F(2x2,3x3) when the shape qualifies (esr_wino_supported), else the direct kernel."""
    d = L.ConvDesc()
    d.ksize, d.in_layout, d.out_layout, d.cin, d.cout = weight.shape[2], L.NHWC, L.NHWC, weight.shape[1], weight.shape[0]
    d.inp = L.View(None, x.shape[-1], 0)
    d.res_mode = res_mode
    use_wino = bool(winograd) and x.dtype == torch.float32 and bool(L.lib().esr_wino_supported(ctypes.byref(d)))
    return conv2d(x, weight, bias, act=act, slope=slope, res=res, res_mode=res_mode, wino=use_wino)


@conv2d_op.register_fake
def _conv2d_fake(x, weight, bias, act, slope, res, res_mode, winograd):
    if x.dim() != 4 or weight.dim() != 4 or weight.shape[2] not in (1, 3) or weight.shape[1] > x.shape[-1]:
        raise L.EsrError("esr::conv2d: NHWC x [N,H,W,pitch >= cin], OIHW weight with k in {1, 3}")
    return x.new_empty((x.shape[0], x.shape[1], x.shape[2], _pad_c(weight.shape[0], x.dtype)))


@torch.library.custom_op("esr::bsconv", mutates_args=())
def bsconv_op(x: Tensor, pw_weight: Tensor, pw_bias: Optional[Tensor], dw_weight: Tensor, dw_bias: Optional[Tensor], act: int,
              slope: float, res: Optional[Tensor], res_mode: int) -> Tensor:
    """BSConvU in one launch: act(dw3x3(pw1x1(x)) [+ res]); NHWC in / out"""
    return bsconv(x, pw_weight, pw_bias, dw_weight, dw_bias, act=act, slope=slope, res=res, res_mode=res_mode)


@bsconv_op.register_fake
def _bsconv_fake(x, pw_weight, pw_bias, dw_weight, dw_bias, act, slope, res, res_mode):
    return x.new_empty((x.shape[0], x.shape[1], x.shape[2], (pw_weight.shape[0] + 3) // 4 * 4))


@torch.library.custom_op("esr::esa_apply", mutates_args=())
def esa_apply_op(x: Tensor, c1: Tensor, c3: Tensor, wf: Tensor, bf: Optional[Tensor], w4: Tensor, b4: Optional[Tensor]) -> Tensor:
    """x * sigmoid(conv4(bilinear(c3) + conv_f(c1))): ESA's full-resolution tail"""
    return esa_apply(x, c1, c3, wf, bf, w4, b4)


@esa_apply_op.register_fake
def _esa_apply_fake(x, c1, c3, wf, bf, w4, b4):
    return torch.empty_like(x)


@torch.library.custom_op("esr::channel_attention", mutates_args=())
def channel_attention_op(x: Tensor, w1: Tensor, b1: Optional[Tensor], w2: Tensor, b2: Optional[Tensor], contrast: bool,
                         nchw: bool) -> Tensor:
    """CALayer (contrast = False) / CCALayer (True): x * sigmoid(W2 . relu(W1 . s + b1) + b2)"""
    return channel_attention(x, w1, b1, w2, b2, contrast=contrast, nchw=nchw)


@channel_attention_op.register_fake
def _channel_attention_fake(x, w1, b1, w2, b2, contrast, nchw):
    return torch.empty_like(x)
