"""Host-side engine shared by the four networks: weight packing, workspace, op lists.

A network's forward is a flat `esr_op` list (include/esr_hip.h) built once per
(N, H, W, device) and replayed by ONE C call (`esr_run_ops`) on the caller's
current HIP stream -- so the reference's `start.record(); forward(); end.record()`
bracket (test_demo.py:429-432) times exactly the device work, and nothing here
synchronises the host.  PyTorch only provides device memory (caching allocator)
and the stream handle.
"""
import collections
import ctypes
import itertools
import threading
import types
import weakref
from dataclasses import dataclass

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import descs


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _host(t):
    """a tensor (or None) as a contiguous CPU float32 tensor"""
    return None if t is None else t.detach().to("cpu", torch.float32).contiguous()


def _pack_args(weight=None, bias=None, cin=None, cin_map=None, cin_phys=None, compute=None, flat=False):
    """The packers' shared opening -> namespace(w, b, cm, cm_p, cin_phys, compute): weight and bias on the host (_host; a 2-D weight as
    [out, in, 1, 1], `flat`: any weight as [out, -1]); `cin_map[s]` = logical input channel carried by physical slot s, or -1 for a zero pad
    slot (padded concat buffers) -> its int32 array `cm`, the pointer `cm_p` into it (the namespace keeps the array alive across the C call)
    and `cin_phys` = its length (no map: `cin_phys`, else the weight's inputs, else `cin`); `compute` by name -> its L.COMPUTE code."""
    w = _host(weight)
    if w is not None and flat:
        w = w.reshape(w.shape[0], -1)
    elif w is not None and w.dim() == 2:
        w = w[:, :, None, None].contiguous()
    cm = cm_p = None
    if cin_map is not None:
        cm = np.ascontiguousarray(np.asarray(cin_map, dtype=np.int32))
        cin_phys, cm_p = len(cm), cm.ctypes.data_as(ctypes.c_void_p)
    elif cin_phys is None:
        cin_phys = cin if w is None else w.shape[1]
    return types.SimpleNamespace(w=w, b=_host(bias), cm=cm, cm_p=cm_p, cin_phys=cin_phys,
                                 compute=L.COMPUTE[compute] if isinstance(compute, str) else compute)


def pack_conv(weight, bias, cin_map=None, cin_phys=None):
    """OIHW (or [out,in] for nn.Linear) fp32 weights + bias -> packed blob (CPU float32 tensor).

    Host-side, no GPU needed.  `cin_map[s]` = logical input channel carried by physical
    slot s, or -1 for a zero pad slot (padded concat buffers)."""
    lib = L.lib()
    a = _pack_args(weight, bias, cin_map=cin_map, cin_phys=cin_phys)
    cout, cin, k, k2 = a.w.shape
    assert k == k2 and k in (1, 3), "only 1x1 / 3x3 kernels are on the hot path"
    nbytes = lib.esr_packed_conv_bytes(a.cin_phys, cout, k)
    if nbytes == 0:
        raise L.EsrError(f"esr_packed_conv_bytes rejected cin_phys={a.cin_phys} cout={cout} k={k}")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_conv_f32(_ptr(a.w), _ptr(a.b), cin, cout, k, a.cm_p, a.cin_phys, _ptr(out), nbytes), "esr_pack_conv_f32")
    return out


def pack_wino(weight, bias, cin_map=None, cin_phys=None):
    """OIHW fp32 3x3 weights + bias -> the Winograd F(2x2, 3x3) blob of esr_pack_wino_f32 (U = G g G^T, computed in fp64 and
    rounded once, in wino_f32_kernel's A-operand order).  Host-side, no GPU needed."""
    lib = L.lib()
    a = _pack_args(weight, bias, cin_map=cin_map, cin_phys=cin_phys)
    cout, cin, k, k2 = a.w.shape
    assert k == 3 and k2 == 3
    nbytes = lib.esr_packed_wino_bytes(a.cin_phys, cout)
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_wino_f32(_ptr(a.w), _ptr(a.b), cin, cout, a.cm_p, a.cin_phys, _ptr(out), nbytes), "esr_pack_wino_f32")
    return out


def unpack_wino(blob, cin, cout, cin_map=None, cin_phys=None):
    """U [cout, cin, 16] and bias of a pack_wino blob (tests)."""
    blob = _host(blob)
    a = _pack_args(cin=cin, cin_map=cin_map, cin_phys=cin_phys)
    u = torch.empty(cout, cin, 16)
    b = torch.empty(cout)
    L.check(L.lib().esr_unpack_wino_f32(_ptr(blob), blob.numel() * 4, cin, cout, a.cm_p, a.cin_phys, _ptr(u), _ptr(b)), "esr_unpack_wino_f32")
    return u, b


def pack_conv_s16(weight, bias, compute, cin_map=None, cin_phys=None):
    """OIHW (or [out,in]) fp32 weights -> the 16-bit-storage blob of esr_pack_conv_s16 (bf16 or fp16; 3x3 taps rounded
    with error diffusion, 1x1 as hi + lo) + fp32 bias."""
    lib = L.lib()
    a = _pack_args(weight, bias, cin_map=cin_map, cin_phys=cin_phys, compute=compute)
    cout, cin, k, _ = a.w.shape
    assert k in (1, 3)
    nbytes = lib.esr_packed_conv_s16_bytes(a.cin_phys, cout, k)
    out = torch.empty((nbytes + 3) // 4, dtype=torch.float32)
    L.check(lib.esr_pack_conv_s16(_ptr(a.w), _ptr(a.b), cin, cout, k, a.cm_p, a.cin_phys, a.compute, _ptr(out), nbytes), "esr_pack_conv_s16")
    return out


def pack_head_s16(weight, bias, compute):
    """Weights of the network's first 3x3 (NCHW fp32 input, cin <= 4) for the 16-bit head: the input arrives as 16-bit slots
    [x_hi | x_lo | x_hi] (esr_pack_input_s16), the weights as [w_hi | w_hi | w_lo] with w = w_hi + w_lo in the storage type, so
    the products w_hi x_hi + w_hi x_lo + w_lo x_hi keep ~fp32 accuracy on the 16-bit matrix cores."""
    dt = torch.bfloat16 if compute == "bf16" else torch.float16
    w = weight.detach().float().cpu()
    hi = w.to(dt).float()
    lo = w - hi
    return pack_conv_s16(torch.cat([hi, hi, lo], dim=1), bias, compute)


def pack_post_s16(weight, bias, compute):
    """[cout, cin(, 1, 1)] fp32 weights of a 1x1 evaluated in a 16-bit conv's epilogue (esr_conv_desc.post_* / post2_*) ->
    esr_pack_post_s16 blob (MFMA images of the weights' 16-bit high and low parts + fp32 bias)."""
    lib = L.lib()
    a = _pack_args(weight, bias, compute=compute, flat=True)
    cout, cin = a.w.shape
    nbytes = lib.esr_packed_post_s16_bytes(cin, cout)
    out = torch.empty((nbytes + 3) // 4, dtype=torch.float32)
    L.check(lib.esr_pack_post_s16(_ptr(a.w), _ptr(a.b), cin, cout, a.compute, _ptr(out), nbytes), "esr_pack_post_s16")
    return out


def pack_tail_s16(weight, bias, nseg, seg_c, mid_c, compute):
    """[cout, nseg * seg_c + mid_c(, 1, 1)] fp32 weights of the 1x1 of a 16-bit tail (esr_conv_desc.tail_*, ABI v12: RFDB's c5 over
    cat(d1, d2, d3, r4)) -> esr_pack_tail_s16 blob (hi / lo fragment images for v_mfma_f32_32x32x16 + fp32 bias)."""
    lib = L.lib()
    a = _pack_args(weight, bias, compute=compute, flat=True)
    cout, kin = a.w.shape
    if kin != nseg * seg_c + mid_c:
        raise L.EsrError("pack_tail_s16: the 1x1 takes nseg * seg_c + mid_c inputs")
    nbytes = lib.esr_packed_tail_s16_bytes(nseg, seg_c, mid_c, cout)
    if not nbytes:
        raise L.EsrError("pack_tail_s16: unsupported shape")
    out = torch.empty((nbytes + 3) // 4, dtype=torch.float32)
    L.check(lib.esr_pack_tail_s16(_ptr(a.w), _ptr(a.b), nseg, seg_c, mid_c, cout, a.compute, _ptr(out), nbytes), "esr_pack_tail_s16")
    return out


def distill_cin_map(cin, cmid):
    """physical K slot -> logical input channel of a distillation step's folded 3x3 (esr_distill_step_s16, wpacked[1]): the chunks of `in`
    (slot s < cin: channel s), then the chunks of d (slot round_up(cin, 16) + j, j < cmid: logical channel cin + j); -1 = a zero pad row"""
    ci, cm = (cin + 15) // 16 * 16, (cmid + 15) // 16 * 16
    return [s if s < cin else -1 for s in range(ci)] + [cin + j if j < cmid else -1 for j in range(cm)]


def pack_distill_s16(w_r, b_r, w_b, b_b, compute):
    """The two 3x3s of a BMDB distillation step, c_r over r [cout, cin, 3, 3] and c_b over d [cout, cmid, 3, 3] (team37_bmdn.py:157-159), folded
    in fp32 into ONE 3x3 over cat[r, d] -- weights cat([W_r, W_b], 1), bias b_r + b_b -- and packed as an esr_pack_conv_s16 image whose K order
    is [in chunks | d chunks] inside every tap pair (distill_cin_map; pad rows zero): esr_distill_step_s16's wpacked[1]."""
    w_r, w_b = w_r.detach().to("cpu", torch.float32), w_b.detach().to("cpu", torch.float32)
    if w_r.dim() != 4 or w_b.dim() != 4 or w_r.shape[0] != w_b.shape[0] or tuple(w_r.shape[2:]) != (3, 3) or tuple(w_b.shape[2:]) != (3, 3):
        raise L.EsrError("pack_distill_s16: two 3x3 weights with the same output channels")
    zero = torch.zeros(w_r.shape[0])
    b = (zero if b_r is None else b_r.detach().to("cpu", torch.float32)) + (zero if b_b is None else b_b.detach().to("cpu", torch.float32))
    return pack_conv_s16(torch.cat([w_r, w_b], dim=1), b, compute, cin_map=distill_cin_map(w_r.shape[1], w_b.shape[1]))


def pack_apply_post(w0, b0, w1, b1, store):
    """Weights of the 1x1 chain riding in esr_esa_apply_f32's launch (esr_esa_desc.post_w): w0 [cout0, cin(, 1, 1)] applied to the
    apply result, w1 [cout1, cout0(, 1, 1)] (or None) applied to w0's result -> esr_pack_apply_post blob."""
    lib = L.lib()
    a0 = _pack_args(w0, b0, flat=True)
    a1 = _pack_args(w1, None if w1 is None else b1, flat=True)
    cout0, cin = a0.w.shape
    cout1 = 0 if w1 is None else a1.w.shape[0]
    if w1 is not None and a1.w.shape[1] != cout0:
        raise L.EsrError("pack_apply_post: w1 must take w0's outputs")
    st = L.STORE[store]
    nbytes = lib.esr_packed_apply_post_bytes(cin, cout0, cout1, st)
    if not nbytes:
        raise L.EsrError("pack_apply_post: unsupported shape / storage")
    out = torch.empty((nbytes + 3) // 4, dtype=torch.float32)
    L.check(lib.esr_pack_apply_post(_ptr(a0.w), _ptr(a0.b), _ptr(a1.w), _ptr(a1.b), cin, cout0, cout1, st, _ptr(out), nbytes), "esr_pack_apply_post")
    return out


def unpack_conv_s16(blob, cin, cout, k, compute, cin_map=None, cin_phys=None):
    """EFFECTIVE fp32 weights (what the 16-bit kernel multiplies by) + bias of a pack_conv_s16 blob."""
    blob = blob.detach().to("cpu").contiguous()
    a = _pack_args(cin=cin, cin_map=cin_map, cin_phys=cin_phys, compute=compute)
    w = torch.empty(cout, cin, k, k)
    b = torch.empty(cout)
    L.check(L.lib().esr_unpack_conv_s16(_ptr(blob), blob.numel() * blob.element_size(), cin, cout, k, a.cm_p, a.cin_phys, a.compute, _ptr(w), _ptr(b)),
            "esr_unpack_conv_s16")
    return w, b


def pack_dense(weight, bias, cin_p, cout_p):
    """Plain [tap][cin_p][cout_p] + bias[cout_p] layout of the small ESA kernels (esr_pack_dense_f32)."""
    lib = L.lib()
    a = _pack_args(weight, bias)
    cout, cin, k, _ = a.w.shape
    nbytes = lib.esr_packed_dense_bytes(cin_p, cout_p, k)
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_dense_f32(_ptr(a.w), _ptr(a.b), cin, cout, k, cin_p, cout_p, _ptr(out), nbytes), "esr_pack_dense_f32")
    return out


def pack_dw(weight, bias):
    """Depthwise [C,1,3,3] weights + bias -> [tap][cp] + bias[cp] (esr_pack_dw_f32)."""
    lib = L.lib()
    a = _pack_args(weight, bias)
    c = a.w.shape[0]
    nbytes = lib.esr_packed_dw_bytes(c)
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_dw_f32(_ptr(a.w), _ptr(a.b), c, _ptr(out), nbytes), "esr_pack_dw_f32")
    return out


def pack_dw7(weight, bias):
    """Depthwise [C,1,7,7] weights + bias -> [tap][cp] + bias[cp], cp = round_up(C, 8) (esr_pack_dw7_f32)."""
    lib = L.lib()
    a = _pack_args(weight, bias)
    c = a.w.shape[0]
    assert tuple(a.w.shape[1:]) == (1, 7, 7)
    nbytes = lib.esr_packed_dw7_bytes(c)
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_dw7_f32(_ptr(a.w), _ptr(a.b), c, _ptr(out), nbytes), "esr_pack_dw7_f32")
    return out


def unpack_dw7(blob, c):
    """[C,1,7,7] weights and bias of a pack_dw7 blob (tests)."""
    blob = _host(blob)
    cp = (c + 7) // 8 * 8
    img = blob[:49 * cp].reshape(49, cp)
    return img[:, :c].t().reshape(c, 1, 7, 7).contiguous(), blob[49 * cp:49 * cp + c].clone()


def pack_cx_pw(w1, b1, w2, b2, compute):
    """The two 1x1s of a ConvNeXt block for esr_cx_block_s16: w1 [cmid, cin(, 1, 1)] -> esr_pack_cx_pw1_s16 blob, w2 [cout, cmid(, 1, 1)] ->
    esr_pack_cx_pw2_s16 blob whose K order is the one in which cx_block_kernel's first GEMM leaves the hidden channels in a lane.  Both are
    rounded once to the storage type; the biases stay fp32.  Returns (blob1, blob2)."""
    lib = L.lib()
    a1 = _pack_args(w1, b1, compute=compute, flat=True)
    a2 = _pack_args(w2, b2, compute=compute, flat=True)
    cmid, cin = a1.w.shape
    cout, cmid2 = a2.w.shape
    if cmid2 != cmid:
        raise L.EsrError("pack_cx_pw: w2 must take w1's outputs")
    n1, n2 = lib.esr_packed_cx_pw1_bytes(cin, cmid), lib.esr_packed_cx_pw2_bytes(cmid, cout)
    if not n1 or not n2:
        raise L.EsrError("pack_cx_pw: unsupported shape")
    o1, o2 = torch.empty(n1 // 4, dtype=torch.float32), torch.empty(n2 // 4, dtype=torch.float32)
    L.check(lib.esr_pack_cx_pw1_s16(_ptr(a1.w), _ptr(a1.b), cin, cmid, a1.compute, _ptr(o1), n1), "esr_pack_cx_pw1_s16")
    L.check(lib.esr_pack_cx_pw2_s16(_ptr(a2.w), _ptr(a2.b), cmid, cout, a2.compute, _ptr(o2), n2), "esr_pack_cx_pw2_s16")
    return o1, o2


def cx_pw_fragments(blob1, blob2, cmid, compute):
    """The MFMA fragment images of a pack_cx_pw pair as float64 arrays (tests): A1 [2 nhp, 2, 64, 8] and b1 [32 nhp] of the first 1x1 --
    fragment (output tile, K step), lane, element --, A2 [nhp, 4, 64, 8] and b2 [64] of the second, nhp = ceil(cmid / 32)."""
    nhp = (cmid + 31) // 32
    dt = torch.bfloat16 if compute == "bf16" else torch.float16
    out = []
    for blob, shape, nb in ((blob1, (2 * nhp, 2, 64, 8), 32 * nhp), (blob2, (nhp, 4, 64, 8), 64)):
        raw = blob.detach().to("cpu").contiguous().view(torch.uint8)
        img = raw[:nhp * 4096].view(dt).to(torch.float64).reshape(shape).numpy()
        bias = raw[nhp * 4096:nhp * 4096 + 4 * nb].view(torch.float32).to(torch.float64).numpy()
        out += [img, bias]
    return tuple(out)


def pack_dwpw_pw(weight, bias, compute):
    """A C -> C 1x1 of team 35's refinement path for esr_dwpw_pair_s16: w [C, C(, 1, 1)] -> the esr_pack_cx_pw1_s16 blob with cin = cmid = C
    (MFMA A fragments in natural K order, rounded once to the storage type; the bias stays fp32)."""
    lib = L.lib()
    a = _pack_args(weight, bias, compute=compute, flat=True)
    cout, cin = a.w.shape
    nbytes = lib.esr_packed_cx_pw1_bytes(cin, cout) if cin == cout else 0
    if not nbytes:
        raise L.EsrError("pack_dwpw_pw: a square 1x1 of at most 64 channels")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_cx_pw1_s16(_ptr(a.w), _ptr(a.b), cin, cout, a.compute, _ptr(out), nbytes), "esr_pack_cx_pw1_s16")
    return out


def dwpw_pw_effective(blob, c, compute):
    """EFFECTIVE weights [C, C] (what dwpw_pair_kernel multiplies by) and bias [C] of a pack_dwpw_pw blob, as float64 tensors (tests)."""
    nt = (c + 31) // 32 * 2
    dt = torch.bfloat16 if compute == "bf16" else torch.float16
    raw = blob.detach().to("cpu").contiguous().view(torch.uint8)
    img = raw[:nt * 2048].view(dt).to(torch.float64).reshape(nt, 2, 4, 16, 8)        # (mt, ks, kq, row, j)
    w = img.permute(0, 3, 1, 2, 4).reshape(nt * 16, 64)                              # row mt * 16 + r, column ks * 32 + kq * 8 + j
    b = raw[nt * 2048:nt * 2048 + 4 * 16 * nt].view(torch.float32).to(torch.float64)
    return w[:c, :c].clone(), b[:c].clone()


def pack_pa_gate(weight, bias, store):
    """The C -> C 1x1 of a pixel attention for esr_pa_gate: w [C, C(, 1, 1)] -> the esr_pack_pa_gate blob of storage `store` ("f32": fp32 MFMA
    A fragments; "bf16" / "f16": a hi + lo pair of 16-bit images, w = hi + lo), its K axis in the order in which pa_gate_kernel holds a pixel's
    channels; the bias stays fp32."""
    lib = L.lib()
    a = _pack_args(weight, bias, flat=True)
    cout, cin = a.w.shape
    nbytes = lib.esr_packed_pa_gate_bytes(cin, L.STORE[store]) if cin == cout else 0
    if not nbytes:
        raise L.EsrError("pack_pa_gate: a square 1x1 of at most 64 channels")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_pa_gate(_ptr(a.w), _ptr(a.b), cin, L.STORE[store], _ptr(out), nbytes), "esr_pack_pa_gate")
    return out


def pa_gate_effective(blob, c, store):
    """EFFECTIVE weights [C, C] (what pa_gate_kernel multiplies by: hi + lo in 16-bit storage) and bias [C] of a pack_pa_gate blob, as float64
    tensors (tests)."""
    raw = blob.detach().to("cpu").contiguous().view(torch.uint8)
    if store == "f32":
        nimg = 4 * 16 * 64 * 4
        w = raw[:nimg].view(torch.float32).to(torch.float64).reshape(4, 4, 4, 4, 16).permute(0, 4, 1, 3, 2).reshape(64, 64)   # (mt, j, i, kq, row)
    else:
        dt = torch.bfloat16 if store == "bf16" else torch.float16
        half = 4 * 2 * 64 * 16
        nimg = 2 * half
        img = raw[:nimg].view(dt).to(torch.float64).reshape(2, 4, 2, 4, 16, 2, 4)                # (hi | lo, mt, ks, kq, row, e / 4, e % 4)
        w = (img[0] + img[1]).permute(0, 3, 1, 4, 2, 5).reshape(64, 64)
    b = raw[nimg:nimg + 256].view(torch.float32).to(torch.float64)
    return w[:c, :c].clone(), b[:c].clone()


def pack_asym_s16(w_l1, b_l1, w_m1, b_m1, w_l2, b_l2, w_m2, b_m2, compute):
    """The four 3-tap convolutions of an ARFDB step -- c_l1 [c, cin, 3, 1], c_m1 [c, cin, 1, 3], c_l2 [c, c, 1, 3], c_m2 [c, c, 3, 1]
    (team14_arfdn/block.py:203-206) -- as esr_asym_step's wpacked: each weight rounded once to the compute type in the fragment order of a
    K dimension of 32 channels x three taps, then the biases b_l1, b_m1 and b_l2 + b_m2 in fp32 (esr_pack_asym_s16)."""
    lib = L.lib()
    ws = [_host(w) for w in (w_l1, w_m1, w_l2, w_m2)]
    bs = [_host(b) for b in (b_l1, b_m1, b_l2, b_m2)]
    c, cin = ws[0].shape[:2]
    shapes = [(c, cin, 3, 1), (c, cin, 1, 3), (c, c, 1, 3), (c, c, 3, 1)]
    if any(w.dim() != 4 or tuple(w.shape) != sh for w, sh in zip(ws, shapes)) or any(b is not None and tuple(b.shape) != (c,) for b in bs):
        raise L.EsrError("pack_asym_s16: weights [c, cin, 3, 1], [c, cin, 1, 3], [c, c, 1, 3], [c, c, 3, 1] and biases [c]")
    nbytes = lib.esr_packed_asym_s16_bytes(cin, c)
    if not nbytes:
        raise L.EsrError(f"esr_packed_asym_s16_bytes rejected cin={cin} c={c}")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    args = [x for w, b in zip(ws[:2], bs[:2]) for x in (_ptr(w), _ptr(b))] + [x for w, b in zip(ws[2:], bs[2:]) for x in (_ptr(w), _ptr(b))]
    L.check(lib.esr_pack_asym_s16(*args, cin, c, L.COMPUTE[compute], _ptr(out), nbytes), "esr_pack_asym_s16")
    return out


def unpack_asym_s16(blob, cin, c, compute):
    """EFFECTIVE weights of a pack_asym_s16 blob in the reference's shapes -- (w_l1, w_m1, w_l2, w_m2) -- and the bias rows (b_l1, b_m1,
    b_l2 + b_m2), fp32 (tests)."""
    blob = _host(blob)
    ws = [torch.zeros(c, cin, 3), torch.zeros(c, cin, 3), torch.zeros(c, c, 3), torch.zeros(c, c, 3)]
    b = torch.zeros(3, c)
    L.check(L.lib().esr_unpack_asym_s16(_ptr(blob), blob.numel() * 4, cin, c, L.COMPUTE[compute], *(_ptr(w) for w in ws), _ptr(b)), "esr_unpack_asym_s16")
    return (ws[0].reshape(c, cin, 3, 1), ws[1].reshape(c, cin, 1, 3), ws[2].reshape(c, c, 1, 3), ws[3].reshape(c, c, 3, 1)), (b[0], b[1], b[2])


def pack_prelu(slopes):
    """The slopes of one nn.PReLU(c), or of several one behind the other ([c] fp32), as esr_prelu's wpacked: c fp32 values in output-channel
    order, zeros up to a multiple of 8 (esr_pack_prelu).  Slopes are never rounded, whatever the storage."""
    a = _host(slopes).reshape(-1)
    c = a.numel()
    nbytes = L.lib().esr_packed_prelu_bytes(c)
    if not nbytes:
        raise L.EsrError(f"esr_packed_prelu_bytes rejected c={c}")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(L.lib().esr_pack_prelu(_ptr(a), c, _ptr(out), nbytes), "esr_pack_prelu")
    return out


def unpack_prelu(blob, c):
    """the c slopes of a pack_prelu blob (tests)"""
    blob = _host(blob)
    a = torch.zeros(c)
    L.check(L.lib().esr_unpack_prelu(_ptr(blob), blob.numel() * 4, c, _ptr(a)), "esr_unpack_prelu")
    return a


def pack_mdsa_gate(w_f, b_f, a_f, w_s, b_s, store):
    """The end of an MDSA block for esr_mdsa_gate: conv_fuse.0 [64, 192(, 1, 1)] as a hi + lo pair of 16-bit images (w = hi + lo), then its
    bias, conv_fuse.1's 64 slopes, sa.0's weight [1, 64(, 1, 1)] and bias in fp32, never rounded (esr_pack_mdsa_gate; 16-bit storage only)."""
    lib = L.lib()
    wf, ws = _host(w_f), _host(w_s)
    wf, ws = wf.reshape(wf.shape[0], -1), ws.reshape(-1)
    bf, af, bs = (None if b_f is None else _host(b_f).reshape(-1)), _host(a_f).reshape(-1), (None if b_s is None else _host(b_s).reshape(-1))
    nbytes = lib.esr_packed_mdsa_gate_bytes(L.STORE[store])
    if not nbytes or tuple(wf.shape) != (64, 192) or ws.numel() != 64 or af.numel() != 64 or (bf is not None and bf.numel() != 64) or \
            (bs is not None and bs.numel() != 1):
        raise L.EsrError("pack_mdsa_gate: W_f [64, 192], b_f [64], a_f [64], w_s [64], b_s [1] in 16-bit storage")
    out = torch.empty(nbytes // 4, dtype=torch.float32)
    L.check(lib.esr_pack_mdsa_gate(_ptr(wf), _ptr(bf), _ptr(af), _ptr(ws), _ptr(bs), L.STORE[store], _ptr(out), nbytes), "esr_pack_mdsa_gate")
    return out


def unpack_mdsa_gate(blob, store):
    """EFFECTIVE (W_f [64, 192] = hi + lo, b_f [64], a_f [64], w_s [64], b_s [1]) of a pack_mdsa_gate blob, fp32 (tests)"""
    blob = _host(blob)
    wf, bf, af, ws, bs = torch.zeros(64, 192), torch.zeros(64), torch.zeros(64), torch.zeros(64), torch.zeros(1)
    L.check(L.lib().esr_unpack_mdsa_gate(_ptr(blob), blob.numel() * 4, L.STORE[store], _ptr(wf), _ptr(bf), _ptr(af), _ptr(ws), _ptr(bs)),
            "esr_unpack_mdsa_gate")
    return wf, bf, af, ws, bs


def pack_unshuffle(weight, bias):
    """`con_` of team 35's ESA, nn.Conv2d(4 f, f, 1, padding 1), for esr_esa_unshuffle_f32: the esr_pack_dense_f32 blob [4 f][16] + bias[16]
    (the pad outputs f .. 15: zero columns, zero bias)."""
    w = _host(weight)
    assert w.dim() == 4 and tuple(w.shape[2:]) == (1, 1) and w.shape[1] == 4 * w.shape[0] and w.shape[0] <= L.ESA_FP
    return pack_dense(w, bias, w.shape[1], L.ESA_FP)


def unpack_unshuffle(blob, f):
    """[f, 4 f, 1, 1] weights and bias of a pack_unshuffle blob (tests)."""
    blob = _host(blob)
    img = blob[:4 * f * L.ESA_FP].reshape(4 * f, L.ESA_FP)
    return img[:, :f].t().reshape(f, 4 * f, 1, 1).contiguous(), blob[4 * f * L.ESA_FP:4 * f * L.ESA_FP + f].clone()


def fold_center(w_r, b_r, w_d, b_d):
    """A 3x3 and a 1x1 over the same input as ONE 3x3: W_r + the 1x1 on the centre tap, b_r + b_d, both summed in fp32
    (RFDNeXt: rc_1 = c1_r(x) + c1_d(x))."""
    w = w_r.detach().to("cpu", torch.float32).clone()
    w[:, :, 1, 1] += w_d.detach().to("cpu", torch.float32).reshape(w.shape[0], w.shape[1])
    zero = torch.zeros(w.shape[0])
    b = (zero if b_r is None else b_r.detach().to("cpu", torch.float32)) + (zero if b_d is None else b_d.detach().to("cpu", torch.float32))
    return w, b


def unpack_conv(blob, cin, cout, k, cin_map=None, cin_phys=None):
    blob = _host(blob)
    a = _pack_args(cin=cin, cin_map=cin_map, cin_phys=cin_phys)
    w = torch.empty(cout, cin, k, k)
    b = torch.empty(cout)
    L.check(L.lib().esr_unpack_conv_f32(_ptr(blob), blob.numel() * 4, cin, cout, k, a.cm_p, a.cin_phys, _ptr(w), _ptr(b)), "esr_unpack_conv_f32")
    return w, b


class Buffer:
    """An NHWC activation buffer inside the workspace: [n][h][w][pitch] elements of `esize` bytes
    (4 = fp32; 2 = bf16 / fp16 for the full-resolution buffers of a 16-bit-storage plan)."""

    def __init__(self, name, pitch, offset_bytes, h=None, w=None, esize=4, arena=0, blocked=False):
        self.name, self.pitch, self.offset, self.h, self.w, self.esize = name, pitch, offset_bytes, h, w, esize
        self.arena = arena     # 0: full-resolution buffers (the plan's storage type), 1: low-resolution fp32 maps -- kept apart, see Plan
        self.blocked = blocked # fp32 only: stored [n][pitch / 8][h][w][8] (esr_conv_desc.blocked8) -- same bytes, other order

    def __getitem__(self, sl):
        """buf[a:b] -> channel slice view (coff=a, channels=b-a)."""
        a = 0 if sl.start is None else sl.start
        b = self.pitch if sl.stop is None else sl.stop
        return (self, a, b - a)


class Planar:
    """A channel concat kept as `nseg` dense tensors [n][h][w][seg_pitch] that lie `stride` bytes apart (16-bit plans): every
    producer writes whole lines into its own tensor (`seg(j)`), the consuming 1x1 walks the segments
    (esr_conv_desc.in_seg_stride / in_seg_chunks).  Physical channel slot s of the consumer = slot s % seg_pitch of segment
    s // seg_pitch -- the same slot order as a dense [.., nseg * seg_pitch] buffer, so the weight blobs do not change."""

    def __init__(self, segs):
        self.segs = segs
        self.pitch = segs[0].pitch
        self.stride = segs[1].offset - segs[0].offset if len(segs) > 1 else 0

    def seg(self, j):
        return self.segs[j]


INPUT = "__input__"
OUTPUT = "__output__"


def _same_view(a, b):
    """True when two op operands (Buffer | (Buffer, coff, channels) | Planar | INPUT / OUTPUT | None) name the same bytes."""
    if a is b:
        return True
    if a is None or b is None or isinstance(a, str) or isinstance(b, str) or isinstance(a, Planar) or isinstance(b, Planar):
        return False
    a = (a, 0, a.pitch) if isinstance(a, Buffer) else a
    b = (b, 0, b.pitch) if isinstance(b, Buffer) else b
    return a[0] is b[0] and a[1] == b[1] and a[2] == b[2]


def _stored_channels(v, logical, chunk):
    """channels of operand `v` a kernel actually moves: the whole pitch of a Buffer (pad slots included), the chunk-rounded width
    of a channel slice, `logical` for the network input / output"""
    if isinstance(v, Buffer):
        return v.pitch
    if isinstance(v, Planar):
        return v.pitch * len(v.segs)
    if isinstance(v, tuple):
        return (v[2] + chunk - 1) // chunk * chunk
    return logical


def _stored_width(dst, c, whole=True):
    """channels a launch stores for the `c` logical channels of destination `dst`: the pad channels of the last K chunk too where `dst` is
    a WHOLE dense buffer (`whole`: Conv.encode asks this for 16-bit storage and low-resolution maps only).
    16-bit storage: the pad channels are zeros (zero weight rows, zero bias) -- a 24-of-32-channel store leaves every 64-byte run partial,
    and partial-line stores cost up to 2.3x a full one (tools/dbg/s16_1x1_probe.py).  Slices of shared buffers keep their width.
    A low-resolution fp32 map that is a whole dense buffer likewise, in every storage type, for another reason: the fp16 ESA apply
    kernel rounds s = bilinear(c3) + conv_f(c1) of all 16 slots to fp16 before conv4's zero weight rows meet it, so a stale fp32
    value beyond 65504 in a pad slot of c3 would become Inf and 0 * Inf = NaN (tests/test_gpu_stale_workspace.py found it in
    EFDN's per-op branch); the fused branch (esr_esa_lowres_f32) has always stored the zeros."""
    if whole and isinstance(dst, Buffer):
        return min((c + 15) // 16 * 16, dst.pitch)
    return c


def _tf(flag):
    """a bool as the kernels' template argument"""
    return "true" if flag else "false"


def _addr(buf, base):
    """base = (workspace address, bytes reserved for the low-resolution arena in front of the full-resolution one)"""
    ws, lo_cap = base
    return ws + (buf.offset if buf.arena == 1 else lo_cap + buf.offset)


def _view(v, base):
    """the esr_view of an op operand (Buffer | (Buffer, coff, channels)); None, an absent operand, stays None"""
    if v is None:
        return None
    if isinstance(v, Buffer):
        v = (v, 0, v.pitch)
    buf, coff, _ = v
    return L.View(ctypes.c_void_p(_addr(buf, base)), buf.pitch, coff)


def _blocked(v):
    return v is not None and v is not INPUT and v is not OUTPUT and not isinstance(v, Planar) and (v if isinstance(v, Buffer) else v[0]).blocked


# Kinds of the weight blobs an op reads, most of them the suffix of the blob's name `<path><suffix>`.  The op that reads a blob names it, its kind
# and the leaves it is made from (_Op.blobs); HipSRModel._repack walks the ops of one small plan and builds each with the kind's packer (_PACKERS).
# What is not a leaf's own image (folded, scaled, sliced, replicated weights, border tables) a network packs in _extra_pack, under the name its ops read.
BASE = ""          # the image under the leaf's own name that _repack builds for every registered leaf (pack_conv / pack_dense / pack_dw), or a network's own blob
S16 = "#s16"       # esr_pack_conv_s16 image (conv_s16_kernel; BSConvU pointwise / distillation 1x1s)
POST = "#post"     # esr_pack_post_s16 image of a 1x1 in a 16-bit conv's epilogue (Post)
HEAD = "#head"     # a 16-bit plan's head conv reads `<path>#head#s16` (pack_head_s16; Plan.conv)
APOST = "#apost"   # pack_apply_post image of the 1x1 riding in an ESA apply launch, under its name (Apply)
DENSE = "#dense"   # esr_pack_dense_f32 blob of a layer of the fused ESA branch (EsaLayer)
DENSE_CAT = "#dense (cat)"  # the `#dense` blob of a kind-3 layer: a 3x3 over the pair's concat, the two halves' inputs at rows 0 and 16
WINO = "#wino"     # esr_pack_wino_f32 blob of an fp32 3x3 (Winograd F(2x2, 3x3)): built with the leaf's own image, looked up by Conv.encode where it exists
DWPAD = "#pad16"   # pack_dw image of a depthwise 3x3 of fewer than 16 channels, zero-padded to 16 (Dw: low-resolution maps stored whole)
DW7 = "dw7"        # pack_dw7 image of a depthwise 7x7, under the leaf's own name (Dw7)
UNSHUFFLE = "unshuffle"  # pack_unshuffle image of team 35's con_, under the leaf's own name (Unshuffle)
CX1 = "#cx1"       # esr_pack_cx_pw1_s16 image of a ConvNeXt block's first 1x1 (CxBlock; pack_cx_pw)
CX2 = "#cx2"       # esr_pack_cx_pw2_s16 image of its second 1x1
DWPW = "#dwpw"     # pack_dwpw_pw image of a 1x1 of team 35's refinement path (DwPwPair)
PAG = "#pag"       # pack_pa_gate image of a pixel attention's 1x1 in the plan's storage (PaGate)
ASYM = "#asym"     # pack_asym_s16 image of an ARFDB step's four 3-tap convolutions, under the name of c{j}_l1 (AsymStep)
RSTEP = "#step"    # pack_prelu image of a ResDB step's slopes, cat(a_e, a_c), under the name of the expansion's nn.PReLU (ResdbStep)
PRELU = "#prelu"   # pack_prelu image of the slopes in front of a convolution, under the name of the nn.PReLU (Prelu)
MGATE = "#mgate"   # pack_mdsa_gate image of the end of an MDSA block, under the name of the fuse 1x1 conv_fuse.0 (MdsaGate)
FOLD = "#fold"     # pack_distill_s16 image of a distillation step's two 3x3s, under the name of the one over the step's input (Distill)


def _cost(name, kernel, cin, cout, k, flops, rd, wr, stored=None, fexec=None):
    """one entry of HipSRModel.op_costs"""
    return dict(name=name, kernel=kernel, cin=cin, cout=cout, k=k, flops=flops, flops_exec=flops if fexec is None else fexec,
                read_bytes=rd, write_bytes=wr, stored_bytes=(rd + wr) if stored is None else max(stored, 0.0))


@dataclass
class Post:
    """A 1x1 convolution in the launch of another op: conv `post` / `post2`, bsconv `distill`, esa_apply `post` (esr_esa_desc.post[])."""
    w: str
    dst: object
    cout: int
    act: int = L.ACT_NONE
    slope: float = 0.05
    res: object = None         # esa_apply: a view added before the activation
    post2: "Post" = None       # conv: a second 1x1 of this one's result


@dataclass
class Tail:
    """The 1x1 behind a conv's 3x3 in the same launch (esr_conv_desc.tail_*): it reads cat(`cat`, the 3x3's result)."""
    w: str
    cat: object                # view (or Planar) of the concat's other channels
    cat_c: int                 # ... their physical channel count
    cat_c_alg: int             # ... their logical one
    cout: int
    mid_act: int = L.ACT_NONE  # activation of the 3x3's result


@dataclass
class EsaLayer:
    """A layer of the fused ESA branch (esr_esa_layer): kind 0 = dense 3x3 `w`, 1 = pointwise `w` + depthwise `w_dw`, 2 = the parallel pair of
    dense 3x3s `w` and `w_dw`, 3 = the dense 3x3 `w` over the pair's 2f-channel concat (EFDN)."""
    kind: int
    act: int
    w: str
    w_dw: str = None


class _Op:
    """What every op kind provides: OP, its esr_op kind (a row of L.LAUNCHERS), encode(op, plan, base, weights) fills its esr_op
    (Plan.finalize), cost(plan, desc) is its HipSRModel.op_costs entry (desc: the finalized esr_op or None), counted_convs(plan) the nn.Conv2d
    calls of the reference it stands for (HipSRModel._counted_convs), blobs(plan) the weight blobs its encode reads as `weights[name]`:
    [(name, kind, source leaf paths), ...] -- what HipSRModel._repack builds for the op (_PACKERS[kind]) or expects from the network's _extra_pack."""

    def desc(self, op):
        """marks `op` as this kind -> the descriptor in it that the kind's launcher reads"""
        op.kind = self.OP
        return getattr(op, L.LAUNCHERS[self.OP][1])

    def counted_convs(self, plan):
        return []

    reads = ()             # ((the field that holds a leaf's path, kind), ...): the blobs of an op that reads one image per field

    def blobs(self, plan):
        return [_blob(getattr(self, field), kind) for field, kind in self.reads]


def _blob(leaf, kind=BASE, *more):
    """the _Op.blobs entry of the `kind` image of `leaf` (and the leaves `more`), named `<leaf><kind>`, or `<leaf>` where the kind is no suffix"""
    return (leaf + kind if kind.startswith("#") else leaf, kind, (leaf,) + more)


@dataclass
class Pack(_Op):
    """16-bit plans: the NCHW fp32 input packed to 16-bit hi / lo slots (esr_pack_input_s16) for the head convolution"""
    dst: Buffer
    cin: int
    kind, OP = "pack", L.OP_PACK_INPUT
    src = INPUT

    def encode(self, op, plan, base, weights):
        d = self.desc(op)
        d.n, d.h, d.w, d.cin, d.storage = plan.n, plan.h, plan.w, self.cin, L.STORE[plan.store]
        d.out0 = _view(self.dst, base)

    def cost(self, plan, desc):             # the network input read once (fp32 NCHW), its 16 16-bit slots per pixel written once
        npix = plan.npix
        return _cost("pack_input", "pack_input_kernel", self.cin, 16, 0, 0.0, float(npix * self.cin * 4), float(npix * 16 * 2),
                     float(npix * (self.cin * 4 + 32)))


@dataclass
class Conv(_Op):
    """A k x k convolution (esr_conv2d_*).  src / dst / res / dst1: INPUT | OUTPUT | Buffer | (Buffer, coff, channels) | Planar."""
    w: str
    src: object
    dst: object                # None: only the post chain reads the result
    cin: int
    cout: int
    k: int = 3
    act: int = L.ACT_NONE
    slope: float = 0.05
    res: object = None
    res_mode: int = L.RES_NONE
    dst1: object = None
    split: int = 0             # channels [0, split) go to dst, the rest to dst1
    hw: tuple = None           # spatial dims if not full-resolution
    counted: bool = True       # False: not an nn.Conv2d call of the reference (complexity counters)
    tail: Tail = None          # the 3x3 result (cout <= 16) feeds a fused 1x1; dst / res / act / split then belong to the 1x1
    post: Post = None          # a 1x1 of the activated output, stored by the same launch
    cin_alg: int = None        # logical input channels when `cin` counts the pad slots of a padded concat (None: cin)
    border: str = None         # name of an esr_conv_desc.border_bias table
    bs_of: str = None          # this dense 3x3 is that BSConvU (merged weights): its algorithmic flops and counter terms are the BSConvU's
    head: int = None           # set by Plan.conv on a 16-bit plan's head: the logical input channels
    hilo: int = 0              # L.HILO_IN | HILO_RES | HILO_OUT: src / res / dst are Plan.pair() hi + lo pairs (esr_conv_desc.hilo)
    kind, OP = "conv", L.OP_CONV

    def __post_init__(self):
        if self.cin_alg is None:
            self.cin_alg = self.cin

    def s16(self, plan):
        """runs on conv_s16_kernel with the `w + S16` blob: every full-resolution NHWC conv of a 16-bit plan"""
        return plan.esize == 2 and self.hw is None and self.src is not INPUT

    def blobs(self, plan):
        s16 = self.s16(plan)                              # (a head: Plan.conv appended HEAD to the leaf's name)
        out = [(self.w + S16, HEAD, (self.w.removesuffix(HEAD),))] if (s16 and self.head) else [_blob(self.w, S16 if s16 else BASE)]
        psfx = POST if (plan.esize == 2 and self.hw is None) else BASE      # the 1x1s evaluated in the conv's epilogue
        posts = [p for p in (self.post, self.post and self.post.post2) if p is not None]
        return out + [_blob(w) for w in (self.border, self.tail and self.tail.w) if w is not None] + [_blob(p.w, psfx) for p in posts]

    def encode(self, op, plan, base, weights):
        st = L.STORE[plan.store]
        lowres = self.hw is not None
        d = self.desc(op)
        d.n, d.h, d.w = plan.n, plan.h, plan.w
        if lowres:
            d.h, d.w = self.hw
        src, res, dst = self.src, self.res, self.dst
        if self.hilo:                                         # hi + lo pairs (Plan.pair): the descriptor's views are the high-part tensors
            pairs = [v for bit, v in ((L.HILO_IN, src), (L.HILO_RES, res), (L.HILO_OUT, dst)) if self.hilo & bit]
            assert all(isinstance(v, Planar) and len(v.segs) == 2 for v in pairs), "hilo: Plan.pair() buffers"
            strides = {v.stride for v in pairs}
            assert len(strides) == 1, "hilo: pairs of one shape"   # one stride for all pairs of the descriptor
            d.hilo_stride = strides.pop()
            src, res, dst = (v.seg(0) if self.hilo & bit else v for bit, v in ((L.HILO_IN, src), (L.HILO_RES, res), (L.HILO_OUT, dst)))
        d.cin, d.cout, d.ksize = (3 * self.head if self.head else self.cin), self.cout, self.k
        d.act, d.slope, d.res_mode = self.act, self.slope, self.res_mode
        d.split = self.split
        d.in_layout = L.NCHW_IN if src is INPUT else L.NHWC
        if isinstance(src, Planar):
            d.inp = _view(src.seg(0), base)
            d.in_seg_stride, d.in_seg_chunks = src.stride, (src.pitch + 15) // 16      # (a tight pitch -- 56 for nf = 50 -- still reads whole K chunks)
        elif src is not INPUT:
            d.inp = _view(src, base)
        d.out_layout = L.NCHW_SHUFFLE4 if dst is OUTPUT else L.NHWC
        if dst is not OUTPUT and dst is not None:             # (None: consumed by the post chain only, out0.ptr == NULL)
            d.out0 = _view(dst, base)
        if self.dst1 is not None:
            d.out1 = _view(self.dst1, base)
        assert self.tail is not None or (not _blocked(dst) and not _blocked(res)), \
            "blocked buffers: input of a Winograd conv / the fused tail, dst1 of a split store, dst / res of the fused tail"
        d.blocked8 = (L.BLOCKED_IN if _blocked(src) else 0) | (L.BLOCKED_OUT1 if _blocked(self.dst1) else 0) | \
            (L.BLOCKED_OUT0 if _blocked(dst) else 0) | (L.BLOCKED_RES if _blocked(res) else 0)
        if res is not None:
            d.res = _view(res, base)
        d.hilo = self.hilo
        d.storage = 0 if lowres else st                       # ESA low-resolution maps: fp32

        width = lambda dst, c: _stored_width(dst, c, st or lowres)
        if dst is not OUTPUT and dst is not None and not self.split:
            d.cout = width(dst, self.cout)
        if self.s16(plan):
            d.wpacked = ctypes.c_void_p(weights[self.w + S16].data_ptr())     # conv_s16_kernel
            d.compute = st
        else:
            d.wpacked = ctypes.c_void_p(weights[self.w].data_ptr())
            wn = weights.get(self.w + WINO)
            if wn is not None and self.tail is None and self.post is None and L.lib().esr_wino_supported(ctypes.byref(d)):
                d.wino_wpacked = ctypes.c_void_p(wn.data_ptr())      # Winograd F(2x2, 3x3): wino_f32_kernel
        if self.border is not None:
            d.border_bias = ctypes.c_void_p(weights[self.border].data_ptr())
        t = self.tail
        if t is not None:
            d.tail_wpacked = ctypes.c_void_p(weights[t.w].data_ptr())
            d.tail_cat_c, d.tail_mid_act = t.cat_c, t.mid_act
            if isinstance(t.cat, Planar):                     # 16-bit tail (ABI v12): three dense tensors one stride apart; the 3x3's own width
                d.tail_cat = _view(t.cat.seg(0), base)
                d.tail_seg_stride16 = t.cat.stride // 16
                d.cout = self.cout
                d.tail_cout = width(dst, t.cout)
            else:
                d.tail_cat = _view(t.cat, base)
                d.tail_cout = t.cout
        t = self.post
        if t is not None:
            psfx = POST if (st and not lowres) else ""       # 16-bit storage: esr_pack_post_s16 images
            d.post_wpacked = ctypes.c_void_p(weights[t.w + psfx].data_ptr())
            d.post_out = _view(t.dst, base)
            d.post_cout, d.post_act = width(t.dst, t.cout) if psfx else t.cout, t.act
            t2 = t.post2
            if t2 is not None:
                d.post2_wpacked = ctypes.c_void_p(weights[t2.w + psfx].data_ptr())
                d.post2_out = _view(t2.dst, base)
                d.post2_cout = t2.cout
            if psfx and self.tail is not None:
                if not L.lib().esr_conv_tail_supported(ctypes.byref(d)):
                    raise L.EsrError(f"{self.w}: no fused tail kernel for this shape (the plan should have built separate ops)")
            elif psfx and not L.lib().esr_conv_post_supported(ctypes.byref(d)):
                raise L.EsrError(f"{self.w}: no fused post-chain kernel for this shape (the plan should have built separate ops)")

    def cost(self, plan, desc):
        es = plan.esize
        hw = self.hw
        npix = plan.npix if hw is None else plan.n * hw[0] * hw[1]
        e_act = es if hw is None else 4                       # low-resolution maps are fp32
        nt = (self.cout + 15) // 16
        nw = L.lib().esr_conv_block_waves(ctypes.byref(desc.conv)) if desc is not None else 0
        kern = f"conv_f32_kernel<NT={nt},KS={self.k},NCHW_IN={int(self.src is INPUT)},NW={nw}>"
        if self.s16(plan):
            kern = f"conv_s16_kernel<NT={nt},KS={self.k},NW={nw or 8},{plan.store}>"
        blk = isinstance(self.dst1, Buffer) and self.dst1.blocked
        if blk:
            kern = kern[:-1] + ",BLK>"                        # the instantiation with the channel-blocked split store
        wino = desc is not None and bool(desc.conv.wino_wpacked) and bool(L.lib().esr_wino_supported(ctypes.byref(desc.conv)))
        if wino:
            # the device symbol as rocprofv3 prints it: wino_f32_kernel<ACT, RES, Y1BLK> (esr_wino.hip: esr_conv2d_wino)
            rm = self.res_mode if self.res is not None else L.RES_NONE
            at = self.act if (self.act == L.ACT_LRELU or (self.act == L.ACT_NONE and rm != L.RES_POST_ACT)) else -1
            kern = f"wino_f32_kernel<{at}, {rm}, {2 if self.dst is OUTPUT else int(blk)}>"
        e_in = 4 if self.src is INPUT else e_act
        e_out = 4 if self.dst is OUTPUT else e_act
        ca, co, k = self.cin_alg, self.cout, self.k
        # a residual that IS the conv's input (RFDB's c1_r..c3_r, RLFB's c3_r: the kernel adds the centre tap of the staged tile)
        # is not read again: VERDICT r05 weak #2
        res_read = self.res is not None and not _same_view(self.res, self.src)
        wb = 4.0 * ca * co * k ** 2                           # weight bytes (part of both the algorithmic and the stored figure)
        rd = npix * (ca * e_in + (co * e_act if res_read else 0)) + wb
        if self.head:
            rd += npix * (16 * 2 - ca * e_in)                 # the head reads the packed 16-slot copy (esr_pack_input_s16), not the fp32 input
        wr = float(npix * co * e_out) if self.dst is not None else 0.0
        hl = self.hilo                                        # hi + lo tensors: twice the 16-bit bytes
        rd += npix * e_act * ((ca if hl & L.HILO_IN else 0) + (co if (hl & L.HILO_RES and res_read) else 0))
        wr += npix * e_act * co if hl & L.HILO_OUT else 0.0
        if hl:
            kern = kern[:-1] + ",HILO>"
        flops = 2.0 * npix * ca * co * k * k
        if self.bs_of is not None:                            # the BSConvU it stands for: pointwise GEMM + depthwise 3x3
            flops = 2.0 * npix * (ca * co + 9 * co)
            wb = 4.0 * (ca * co + 10 * co)
            rd = npix * (ca * e_in + (co * e_act if res_read else 0)) + wb
            if self.head:
                rd += npix * (16 * 2 - ca * e_in)
        tl = self.tail
        if tl is not None:                                    # 3x3 -> 1x1 in one kernel: both GEMMs' flops, the 1x1's traffic
            kern = f"conv_f32_kernel<NT={nt},KS=3,NCHW_IN=0,NW=4,TAIL={(tl.cout + 15) // 16}>"
            if plan.esize == 2:
                kern = f"rfdb_tail_kernel<{plan.store}>"
            if (self.cin + 7) // 8 == 6 and tl.cat_c == 48 and tl.cout == 64 and self.res_mode in (L.RES_NONE, L.RES_PRE_ACT):
                kern = f"imdb_tail_kernel<FOLD={int(self.res is not None)}>"       # esr_hip.hip: imdb_tail_shape()
            k1 = tl.cat_c_alg + co                            # (logical channels of the concat: 16-bit tail: three dense 32-slot tensors of dc)
            flops += 2.0 * npix * k1 * tl.cout
            wb = 4.0 * (ca * co * 9 + k1 * tl.cout)
            rd = npix * e_act * (ca + tl.cat_c_alg + (tl.cout if res_read else 0)) + wb
            wr = float(npix * e_act * tl.cout)
        pt = self.post
        if pt is not None:                                    # + the 1x1 of the activated output, stored by the same launch
            if nw == 8:
                kern = kern[:-1] + f",POST={(pt.cout + 15) // 16}>"
            post_in = co if tl is None else tl.cout           # (behind a tail: the 1x1 of the tail's result)
            flops += 2.0 * npix * post_in * pt.cout
            wr += npix * e_act * pt.cout
            if pt.post2 is not None:
                kern = kern[:-1] + f"+{(pt.post2.cout + 15) // 16}>"
                flops += 2.0 * npix * pt.cout * pt.post2.cout
                wr += npix * e_act * pt.post2.cout
        # STORED bytes: what the launch moves when pad channels travel (pitch 64 for nf = 50, 32 for dc = 25): whole pitches of
        # Buffers, chunk-rounded slices -- next to the algorithmic bytes above, so the padding waste is a reported number
        chunk = 8 if es == 4 else 16
        hl_in, hl_res, hl_out = (2 if hl & L.HILO_IN else 1), (2 if hl & L.HILO_RES else 1), (2 if hl & L.HILO_OUT else 1)
        sc = lambda v, logical: _stored_channels(v.seg(0) if (isinstance(v, Planar) and hl) else v, logical, chunk)
        st = 16 * 2 * npix if self.head else npix * e_in * hl_in * sc(self.src, ca)
        if tl is not None:
            st += npix * e_act * sc(tl.cat, tl.cat_c)
        if res_read:
            st += npix * e_act * hl_res * sc(self.res, co if tl is None else tl.cout)
        if self.dst is not None:
            st += npix * e_out * hl_out * sc(self.dst, self.split if self.dst1 is not None else (co if tl is None else tl.cout))
        if self.dst1 is not None:
            st += npix * e_act * sc(self.dst1, co - self.split)
        if pt is not None:
            st += npix * e_act * sc(pt.dst, pt.cout)
            if pt.post2 is not None:
                st += npix * e_act * sc(pt.post2.dst, pt.post2.cout)
            wb += 4.0 * co * pt.cout + (4.0 * pt.cout * pt.post2.cout if pt.post2 is not None else 0.0)
        # flops = ALGORITHMIC (direct-convolution) flops; flops_exec = what the matrix cores execute: Winograd F(2x2,3x3) does 16
        # multiplications per 2x2 outputs where the direct form does 36
        fexec = flops * (16.0 / 36.0) if wino else flops
        if hl & L.HILO_IN:
            fexec = 2.0 * flops                               # both halves of a hi + lo input meet the weights
        return _cost(self.w, kern, self.cin, co, k, flops, rd, wr, float(st) + wb, fexec)

    def counted_convs(self, plan):
        if not self.counted:
            return []
        npix = plan.npix if self.hw is None else plan.n * self.hw[0] * self.hw[1]
        conv = (self.cin_alg, self.cout, self.k, npix, self.act)
        t = self.tail
        if t is not None:                                     # two nn.Conv2d calls of the reference in one launch
            return [conv[:4] + (t.mid_act,), (t.cat_c + self.cout, t.cout, 1, npix, self.act)]
        t = self.post
        if t is not None:
            r = [conv, (self.cout, t.cout, 1, npix, t.act)]
            if t.post2 is not None:
                r.append((t.cout, t.post2.cout, 1, npix, L.ACT_NONE))
            return r
        return [conv]


@dataclass
class Dw(_Op):
    """depthwise 3x3 + bias (+act): the dw half of BSConvU"""
    w: str
    src: object
    dst: object
    c: int
    act: int = L.ACT_NONE
    slope: float = 0.05
    hw: tuple = None
    res: object = None         # a view added before / behind the activation (res_mode), as Conv's
    res_mode: int = L.RES_NONE
    kind, OP = "dw", L.OP_DWCONV

    def blobs(self, plan):
        # a low-resolution map that is a whole dense buffer is stored whole, pad channels (zeros: zero weights, zero bias) included:
        # _stored_width.  The pointwise conv in front of it stored its pad channels the same way
        pad = (self.hw is not None and self.c < 16 and isinstance(self.src, Buffer) and isinstance(self.dst, Buffer)
               and min(self.src.pitch, self.dst.pitch) >= 16)
        return [_blob(self.w, DWPAD if pad else BASE)]

    def encode(self, op, plan, base, weights):
        (w, kind, _), = self.blobs(plan)
        lowres = self.hw is not None                          # a low-resolution map is fp32 in every plan; the DWPAD image has 16 channels
        descs.dwconv3x3(self.desc(op), (plan.n, *self.hw) if lowres else plan.nhw, 0 if lowres else plan.st,
                        x=_view(self.src, base), w=weights[w].data_ptr(), c=16 if kind == DWPAD else self.c, act=self.act, slope=self.slope,
                        y=_view(self.dst, base), res=_view(self.res, base), res_mode=self.res_mode if self.res is not None else L.RES_NONE)

    def cost(self, plan, desc):
        npix, e_act = (plan.npix, plan.esize) if self.hw is None else (plan.n * self.hw[0] * self.hw[1], 4)
        # (a residual that IS the input is served by the caches, as in Conv.cost)
        res_read = self.res is not None and not _same_view(self.res, self.src)
        return _cost(self.w, "dwconv3x3_kernel", self.c, self.c, 3, 2.0 * 9 * self.c * npix, float(npix * e_act * self.c * (2 if res_read else 1)),
                     float(npix * e_act * self.c))

    def dw_counted(self, plan):
        """nn.Conv2d(c, c, 3, groups=c): one input channel per filter (for the networks that count their depthwise layers one by one)"""
        npix = plan.npix if self.hw is None else plan.n * self.hw[0] * self.hw[1]
        return [(1, self.c, 3, npix, self.act)]


@dataclass
class Dw7(_Op):
    """depthwise 7x7 + bias (esr_dwconv7x7) -- see Plan.dwconv7.  The blob `w` is pack_dw7's."""
    w: str
    src: object
    dst: object
    c: int
    kind, OP = "dw7", L.OP_DWCONV7
    reads = (("w", DW7),)

    def encode(self, op, plan, base, weights):
        descs.dwconv7x7(self.desc(op), plan.nhw, plan.st, x=_view(self.src, base), w=weights[self.w].data_ptr(), c=self.c, y=_view(self.dst, base))

    def cost(self, plan, desc):
        npix, es = plan.npix, plan.esize
        return _cost(self.w, f"dwconv7x7_kernel<{L.STORE[plan.store]}>", self.c, self.c, 7, 2.0 * 49 * self.c * npix,
                     float(npix * es * self.c) + 4.0 * 50 * self.c, float(npix * es * self.c),
                     float(npix * es * (_stored_channels(self.src, self.c, 8) + _stored_channels(self.dst, self.c, 8))) + 4.0 * 50 * self.c)

    def counted_convs(self, plan):            # nn.Conv2d(c, c, 7, groups=c): one input channel per filter
        return [(1, self.c, 7, plan.npix, L.ACT_NONE)]


@dataclass
class Bs(_Op):
    """BSConvU in one launch (esr_bsconv_f32): dst = act(dw3x3(pw1x1(src)) [+ res]).  distill: the enclosing block's distillation 1x1
    of the same input."""
    pw: str
    dw: str
    src: object
    dst: object
    cin: int
    cout: int
    act: int = L.ACT_NONE
    slope: float = 0.05
    res: object = None
    res_mode: int = L.RES_NONE
    distill: Post = None
    kind, OP = "bs", L.OP_BSCONV

    def blobs(self, plan):                                    # 16-bit storage: hi + lo 1x1 blobs (esr_pack_conv_s16)
        sfx = S16 if plan.esize == 2 else BASE
        return [_blob(self.pw, sfx), _blob(self.dw)] + ([_blob(self.distill.w, sfx)] if self.distill is not None else [])

    def encode(self, op, plan, base, weights):
        st = L.STORE[plan.store]
        d = self.desc(op)
        d.storage = st
        d.n, d.h, d.w, d.cin, d.c = plan.n, plan.h, plan.w, self.cin, self.cout
        d.act, d.slope, d.res_mode = self.act, self.slope, self.res_mode
        d.inp, d.out = _view(self.src, base), _view(self.dst, base)
        if self.res is not None:
            d.res = _view(self.res, base)
        sfx = S16 if st else ""                               # 16-bit storage: hi + lo 1x1 blobs (esr_pack_conv_s16)
        d.pw_packed = ctypes.c_void_p(weights[self.pw + sfx].data_ptr())
        d.dw_packed = ctypes.c_void_p(weights[self.dw].data_ptr())
        t = self.distill
        if t is not None:
            d.d_packed = ctypes.c_void_p(weights[t.w + sfx].data_ptr())
            d.d_cout, d.d_act = t.cout, t.act
            d.d_out = _view(t.dst, base)

    def cost(self, plan, desc):                               # pointwise (+ distillation) GEMM + depthwise, one launch
        npix, e_act, ci, co = plan.npix, plan.esize, self.cin, self.cout
        dco = self.distill.cout if self.distill is not None else 0
        res_read = self.res is not None and not _same_view(self.res, self.src)
        return _cost(self.dw, f"bsconv_kernel<NTP={(co + 15) // 16},NTD={(dco + 15) // 16}>", ci, co, 3,
                     2.0 * npix * (ci * (co + dco) + 9 * co),
                     npix * e_act * (ci + (co if res_read else 0)) + 4.0 * (ci * (co + dco) + 10 * co), float(npix * e_act * (co + dco)))


@dataclass
class S2(_Op):
    """ESA's 3x3 stride-2 conv2 (esr_conv3x3s2_f32): the full-resolution map `src` -> the low-resolution fp32 `dst`"""
    w: str
    src: Buffer
    dst: Buffer
    f: int
    kind, OP = "s2", L.OP_CONV3X3S2
    reads = (("w", BASE),)

    def encode(self, op, plan, base, weights):
        e = self.desc(op)
        e.n, e.h, e.w, e.h_lo, e.w_lo = plan.n, self.src.h, self.src.w, self.dst.h, self.dst.w
        e.x, e.y = _view(self.src, base), _view(self.dst, base)
        e.storage = L.STORE[plan.store]                       # reads the full-resolution conv1 map
        e.f = self.f
        e.w0 = ctypes.c_void_p(weights[self.w].data_ptr())

    def cost(self, plan, desc):                               # reads the full-resolution conv1 map, writes the half-resolution one
        npix, f = plan.n * self.dst.h * self.dst.w, self.f
        return _cost(self.w, "conv3x3s2_kernel", f, f, 3, 2.0 * 9 * f * f * npix, float(plan.n * self.src.h * self.src.w * f * self.src.esize),
                     float(npix * f * 4))

    def counted_convs(self, plan):
        return [(self.f, self.f, 3, plan.n * self.dst.h * self.dst.w, L.ACT_NONE)]


@dataclass
class Pool(_Op):
    """ESA's 7x7 / stride-3 max pooling (esr_maxpool7s3_f32)"""
    src: Buffer
    dst: Buffer
    kind, OP = "pool", L.OP_MAXPOOL7S3

    def encode(self, op, plan, base, weights):
        e = self.desc(op)
        e.n, e.h, e.w, e.h_lo, e.w_lo = plan.n, self.src.h, self.src.w, self.dst.h, self.dst.w
        e.x, e.y = _view(self.src, base), _view(self.dst, base)

    def cost(self, plan, desc):
        return _cost("pool", "maxpool7s3_kernel", 0, 0, 0, 0.0, float(plan.n * self.src.h * self.src.w * 16 * 4),
                     float(plan.n * self.dst.h * self.dst.w * 16 * 4))


@dataclass
class Pool7(_Op):
    """EFDN's ESA pooling, max_pool2d(7, stride 7, padding 1) of the full-resolution conv1 map (esr_maxpool7s7_f32)"""
    src: Buffer
    dst: Buffer
    kind, OP = "pool7", L.OP_MAXPOOL7S7

    def encode(self, op, plan, base, weights):
        e = self.desc(op)
        e.n, e.h, e.w, e.h_lo, e.w_lo = plan.n, self.src.h, self.src.w, self.dst.h, self.dst.w
        e.x, e.y = _view(self.src, base), _view(self.dst, base)
        e.storage = L.STORE[plan.store]                       # reads the full-resolution conv1 map

    def cost(self, plan, desc):
        return _cost("pool7", f"esa_pool7_kernel<{L.STORE[plan.store]}>", 0, 0, 0, 0.0, float(plan.n * self.src.h * self.src.w * 16 * self.src.esize),
                     float(plan.n * self.dst.h * self.dst.w * 16 * 4))


@dataclass
class _Fused(_Op):
    """ONE op in place of a run of ops, which stay attached as `replaces`: weights, complexity counters and algorithmic costs are theirs.
    Where the kernel takes only some shapes its row of L.LAUNCHERS names the C ABI's predicate (esr_*_supported); the class names the
    kernel in words (`what`) and states the structure it stands for in check(): Plan._fuse asks the predicate about the descriptor
    `encode` fills before it fuses, Plan.finalize once more."""
    replaces: list

    def check(self):
        pass

    def supported(self, op):
        """does the kernel take the descriptor that `encode` filled into `op`?"""
        _, field, predicate = L.LAUNCHERS[self.OP]
        return predicate is None or bool(getattr(L.lib(), predicate)(ctypes.byref(getattr(op, field))))

    def counted_convs(self, plan):
        return [c for o in self.replaces for c in o.counted_convs(plan)]

    def own_blobs(self, plan):                                # what the one-launch form reads beyond the blobs of the ops it replaces ...
        return []

    def blobs(self, plan):                                    # ... and theirs: a plan of another shape may keep the ops, with the same model's blobs
        return self.own_blobs(plan) + [b for o in self.replaces for b in o.blobs(plan)]


class _AnyBlob:
    """the weights of Plan._fuse's probe: every name yields a non-null dummy address (the predicates test blob pointers for null only)"""

    def __getitem__(self, name):
        return self

    def data_ptr(self):
        return 4096


@dataclass
class Lowres(_Fused):
    """ESA's low-resolution branch as ONE op (esr_esa_lowres_f32) -- see Plan.esa_lowres.  w: conv2's weights (None: EFDN's stride-7 branch,
    pooled straight from `src`)."""
    src: Buffer
    pooled: Buffer
    dst: Buffer
    f: int
    w: str
    layers: list
    kind, OP = "lowres", L.OP_ESA_LOWRES

    def own_blobs(self, plan):                                # the layers in the plain dense layout; kind 1: the depthwise half as it is
        out = [_blob(self.w)] if self.w is not None else []
        for ly in self.layers:
            out.append((ly.w + DENSE, DENSE_CAT, (ly.w,)) if ly.kind == 3 else _blob(ly.w, DENSE))
            if ly.kind in (1, 2):
                out.append(_blob(ly.w_dw, DENSE if ly.kind == 2 else BASE))
        return out

    def encode(self, op, plan, base, weights):
        d = self.desc(op)
        d.n, d.h, d.w, d.f, d.storage, d.n_layers = plan.n, plan.h, plan.w, self.f, L.STORE[plan.store], len(self.layers)
        d.x = _view(self.src, base)
        d.w_s2 = ctypes.c_void_p(weights[self.w].data_ptr()) if self.w is not None else None
        d.pooled = ctypes.c_void_p(_addr(self.pooled, base))
        d.y = ctypes.c_void_p(_addr(self.dst, base))
        for l, ly in enumerate(self.layers):
            d.layer[l].kind, d.layer[l].act = ly.kind, ly.act
            d.layer[l].w = ctypes.c_void_p(weights[ly.w + DENSE].data_ptr())
            if ly.kind == 1:
                d.layer[l].w_dw = ctypes.c_void_p(weights[ly.w_dw].data_ptr())
            elif ly.kind == 2:                                # the pair's second 3x3
                d.layer[l].w_dw = ctypes.c_void_p(weights[ly.w_dw + DENSE].data_ptr())

    def cost(self, plan, desc):                               # conv2 (s2) + pooling + the 3x3 layers behind it: two launches, only the pooled map in between
        src, dst, f = self.src, self.dst, self.f
        npl = plan.n * dst.h * dst.w
        if self.w is None:                                    # EFDN: pooling of the full-resolution map, then the pair + conv_23 in one launch
            flops = 2.0 * npl * (2 * 9 * f * f + 9 * 2 * f * f)
            return _cost(self.layers[0].w, f"esa_pool7_kernel<{L.STORE[plan.store]}> + esa_pool7_branch_kernel", f, f, 3, flops,
                         float(plan.n * src.h * src.w * f * src.esize + npl * f * 4), float(2 * npl * f * 4))
        h2, w2 = (src.h - 3) // 2 + 1, (src.w - 3) // 2 + 1
        flops = 2.0 * 9 * f * f * plan.n * h2 * w2
        for ly in self.layers:
            flops += 2.0 * npl * (9 * f * f if ly.kind == 0 else f * f + 9 * f)
        return _cost(self.w, f"esa_s2pool{'16' if plan.esize == 2 else ''}_kernel<{L.STORE[plan.store]}> + esa_chain_kernel", f, f, 3, flops,
                     float(plan.n * src.h * src.w * f * src.esize + npl * f * 4), float(2 * npl * f * 4))


@dataclass
class Chain(_Fused):
    """A block's 3x3 convolutions as ONE esr_conv_chain_s16 op -- see Plan.chain (gate=False: rlfb_chain_kernel) and Plan.hfab
    (gate=True: hfab_kernel)."""
    gate: bool = False
    kind, OP = "chain", L.OP_CONV_CHAIN
    what = property(lambda self: "HFAB" if self.gate else "chain")

    def check(self):
        sub, last = self.replaces, self.replaces[-1]
        assert (len(sub) == 4 if self.gate else len(sub) >= 2) and all(o.kind == "conv" and o.k == 3 for o in sub)
        for a, b in zip(sub[:-1], sub[1:]):
            assert b.src is a.dst and a.res is None and a.post is None
        if self.gate:
            assert all(a.act == sub[0].act for a in sub[:-1])
            assert last.res_mode == L.RES_GATE and last.res is sub[0].src and last.post is None and isinstance(last.dst, Buffer)
        else:
            assert last.dst is None and last.res is sub[0].src and last.post is not None and last.post.post2 is not None

    def encode(self, op, plan, base, weights):
        first, last = self.replaces[0], self.replaces[-1]
        t = last.post
        common = dict(x=_view(first.src, base), w=[weights[so.w + S16].data_ptr() for so in self.replaces], cin=first.cin, cmid=first.cout,
                      cout=last.cout, act=first.act, slope=first.slope)
        if self.gate:
            descs.hfab(self.desc(op), plan.nhw, plan.st, **common, y=_view(last.dst, base), y_width=_stored_width(last.dst, last.cout))
        else:
            descs.chain(self.desc(op), plan.nhw, plan.st, **common, res_mode=last.res_mode, post_w=weights[t.w + POST].data_ptr(), v=_view(t.dst, base),
                        v_width=_stored_width(t.dst, t.cout), post_act=t.act, post2_w=weights[t.post2.w + POST].data_ptr(),
                        c1=_view(t.post2.dst, base), c1_width=t.post2.cout)

    def cost(self, plan, desc):
        sub, npix, es = self.replaces, plan.npix, plan.esize
        flops = sum(2.0 * npix * so.cin_alg * so.cout * 9 for so in sub)
        wb = 4.0 * sum(so.cin_alg * so.cout * 9 for so in sub)
        if self.gate:                   # HFAB in one launch: x read once (also the gate operand), the gated result written once
            kern = f"hfab_kernel<{_tf(plan.store == 'bf16')}, {(sub[0].cin + 15) // 16}>"
            stored = float(npix * es * (_stored_channels(sub[0].src, sub[0].cin, 16) + _stored_channels(sub[-1].dst, sub[-1].cout, 16))) + wb
            return _cost(sub[0].w, kern, sub[0].cin, sub[-1].cout, 3, flops, float(npix * sub[0].cin_alg * es) + wb,
                         float(npix * sub[-1].cout * es), stored)
        # the block's 3x3 chain + its two 1x1s in one launch: the input read once, only the 1x1 results written
        t, t2 = sub[-1].post, sub[-1].post.post2
        flops += 2.0 * npix * (sub[-1].cout * t.cout + t.cout * t2.cout)
        rd = float(npix * sub[0].cin_alg * es) + 4.0 * (sum(so.cin_alg * so.cout * 9 for so in sub) + sub[-1].cout * t.cout + t.cout * t2.cout)
        return _cost(sub[0].w, f"rlfb_chain_kernel<{plan.store}>", sub[0].cin, sub[-1].cout, 3, flops, rd, float(npix * es * (t.cout + t2.cout)))


@dataclass
class Distill(_Fused):
    """A BMDB distillation step as ONE esr_distill_step_s16 op -- see Plan.distill_step (distill_step_kernel).  replaces: [c_d, c_b, c_r]."""
    kind, OP, what = "distill", L.OP_DISTILL_STEP, "distillation step"

    def check(self):
        sub = self.replaces
        assert len(sub) == 3 and all(o.kind == "conv" and o.post is None and o.tail is None and not o.hilo for o in sub)
        cd, cb, cr = sub
        assert cd.k == 1 and cb.k == 3 and cr.k == 3 and cd.act == cr.act == L.ACT_RELU and cb.act == L.ACT_NONE and cd.res is None
        assert _same_view(cb.src, cd.dst) and _same_view(cr.src, cd.src) and _same_view(cr.res, cb.dst) and cr.res_mode == L.RES_PRE_ACT
        assert cb.res is None or (_same_view(cb.res, cd.src) and cb.res_mode == L.RES_PRE_ACT)

    def own_blobs(self, plan):                                # c_r and c_b as one 3x3 over cat[r, d], under c_r's name
        return [_blob(self.replaces[2].w, FOLD, self.replaces[1].w)]

    def encode(self, op, plan, base, weights):
        cd, cb, cr = self.replaces
        descs.distill_step(self.desc(op), plan.nhw, plan.st, x=_view(cd.src, base), w_d=weights[cd.w + S16].data_ptr(),
                           w_fold=weights[cr.w + FOLD].data_ptr(), cin=cd.cin, cmid=cd.cout, cout=cr.cout, res=cb.res is not None,
                           dd=_view(cd.dst, base), d_width=_stored_width(cd.dst, cd.cout), y=_view(cr.dst, base), y_width=_stored_width(cr.dst, cr.cout))

    def cost(self, plan, desc):             # the step's input read once, d and the result written once
        cd, cb, cr = self.replaces
        npix, es = plan.npix, plan.esize
        flops = sum(2.0 * npix * so.cin_alg * so.cout * so.k * so.k for so in self.replaces)
        wb = 4.0 * sum(so.cin_alg * so.cout * so.k * so.k for so in self.replaces)
        kern = f"distill_step_kernel<{_tf(plan.store == 'bf16')}, {(cd.cin + 15) // 16}, {_tf(cb.res is not None)}>"
        stored = float(npix * es * (_stored_channels(cd.src, cd.cin, 16) + _stored_channels(cd.dst, cd.cout, 16) + _stored_channels(cr.dst, cr.cout, 16))) + wb
        return _cost(cd.w, kern, cd.cin, cr.cout, 3, flops, float(npix * cd.cin_alg * es) + wb, float(npix * es * (cd.cout + cr.cout)), stored)


@dataclass
class ResHead(_Fused):
    """The head of ESAN's residual block as ONE esr_resblock_head_s16 op -- see Plan.resblock_head (resblock_head_kernel).  replaces: [add,]
    conv1, conv2, ESA.conv1; the first block of the trunk has no add."""
    kind, OP, what = "reshead", L.OP_RESBLOCK_HEAD, "residual-block head"

    def check(self):
        sub = self.replaces
        assert len(sub) in (3, 4) and all(o.kind == "conv" and o.post is None and o.tail is None and not o.hilo for o in sub)
        c1, c2, ce = sub[-3:]
        assert c1.k == 3 and c2.k == 3 and ce.k == 1 and c1.act == L.ACT_RELU and c2.act == ce.act == L.ACT_NONE
        assert c1.res is None and c2.res is None and ce.res is None and _same_view(c2.src, c1.dst) and _same_view(ce.src, c2.dst)
        if len(sub) == 4:
            add = sub[0]
            assert add.k == 1 and not add.counted and add.act == L.ACT_NONE and add.res_mode == L.RES_PRE_ACT and _same_view(c1.src, add.dst)
            assert not _same_view(add.dst, add.res) and not _same_view(add.dst, add.src)

    def encode(self, op, plan, base, weights):
        add = self.replaces[0] if len(self.replaces) == 4 else None
        c1, c2, ce = self.replaces[-3:]
        # x = xin + g: the add's residual is the block input, its source the ESA result
        xin, g, xs = (add.res, add.src, add.dst) if add is not None else (c1.src, None, None)
        descs.resblock_head(self.desc(op), plan.nhw, plan.st, x=_view(xin, base), g=_view(g, base), xs=_view(xs, base),
                            w1=weights[c1.w + S16].data_ptr(), w2=weights[c2.w + S16].data_ptr(), wc=weights[ce.w + S16].data_ptr(),
                            cin=c1.cin, cout=c2.cout, u=_view(c2.dst, base), c1=_view(ce.dst, base), c1_width=_stored_width(ce.dst, ce.cout))

    def cost(self, plan, desc):             # xin (and g) read once; x, u and c1 written once
        add = len(self.replaces) == 4
        c1, c2, ce = self.replaces[-3:]
        npix, es = plan.npix, plan.esize
        convs = (c1, c2, ce)
        flops = sum(2.0 * npix * so.cin_alg * so.cout * so.k * so.k for so in convs)
        wb = 4.0 * sum(so.cin_alg * so.cout * so.k * so.k for so in convs)
        kern = f"resblock_head_kernel<{_tf(plan.store == 'bf16')}, {_tf(add)}>"
        rd = float(npix * es * c1.cin * (2 if add else 1)) + wb
        wr = float(npix * es * ((c1.cin if add else 0) + c2.cout + ce.cout))
        stored = float(npix * es * (c1.cin * (3 if add else 1) + c2.cout + _stored_channels(ce.dst, ce.cout, 16))) + wb
        return _cost(c1.w, kern, c1.cin, c2.cout, 3, flops, rd, wr, stored)


@dataclass
class Cascade(_Fused):
    """FRFDB's narrowing refinement path as ONE esr_refine_cascade_s16 op -- see Plan.refine_cascade (refine_cascade_kernel).
    replaces: [c2_r, c3_d, c3_r, c4]."""
    kind, OP, what = "cascade", L.OP_REFINE_CASCADE, "refinement cascade"

    def check(self):
        sub = self.replaces
        assert len(sub) == 4 and all(o.kind == "conv" and o.post is None and o.tail is None and not o.hilo and o.hw is None for o in sub)
        c2r, c3d, c3r, c4 = sub
        assert c2r.k == 3 and c3d.k == 1 and c3r.k == 3 and c4.k == 3 and c3d.res is None
        assert all(o.act == L.ACT_LRELU and o.slope == c2r.slope for o in sub)
        assert all(o.res_mode == L.RES_PRE_ACT and _same_view(o.res, o.src) for o in (c2r, c3r, c4))       # every 3x3 adds its own input
        assert _same_view(c3d.src, c2r.dst) and _same_view(c3r.src, c3d.dst) and _same_view(c4.src, c3r.dst)

    def encode(self, op, plan, base, weights):
        c2r, c3d, c3r, c4 = self.replaces
        descs.refine_cascade(self.desc(op), plan.nhw, plan.st, d2=_view(c2r.src, base), w=[weights[so.w + S16].data_ptr() for so in self.replaces],
                             cin=c2r.cin, cmid=c3d.cout, cout=c4.cout, slope=c2r.slope, d3=_view(c3d.dst, base),
                             d3_width=_stored_width(c3d.dst, c3d.cout), r4=_view(c4.dst, base), r4_width=_stored_width(c4.dst, c4.cout))

    def cost(self, plan, desc):             # d2 read once; d3 and r4 written once
        c2r, c3d, c3r, c4 = self.replaces
        npix, es = plan.npix, plan.esize
        flops = sum(2.0 * npix * so.cin_alg * so.cout * so.k * so.k for so in self.replaces)
        wb = 4.0 * sum(so.cin_alg * so.cout * so.k * so.k for so in self.replaces)
        kern = f"refine_cascade_kernel<{_tf(plan.store == 'bf16')}>"
        stored = float(npix * es * (_stored_channels(c2r.src, c2r.cin, 16) + _stored_channels(c3d.dst, c3d.cout, 16) + _stored_channels(c4.dst, c4.cout, 16))) + wb
        return _cost(c2r.w, kern, c2r.cin, c4.cout, 3, flops, float(npix * c2r.cin_alg * es) + wb, float(npix * es * (c3d.cout + c4.cout)), stored)


@dataclass
class CxBlock(_Fused):
    """RFDNeXt's ConvNeXt block as ONE esr_cx_block_s16 op -- see Plan.cx_block (cx_block_kernel).  replaces: [dw7, pw1, pw2]."""
    kind, OP, what = "cx", L.OP_CX_BLOCK, "ConvNeXt block"

    def check(self):
        sub = self.replaces
        assert len(sub) == 3 and sub[0].kind == "dw7" and all(o.kind == "conv" and o.k == 1 and o.post is None and o.tail is None and not o.hilo
                                                              and o.hw is None for o in sub[1:])
        dw, pw1, pw2 = sub
        assert pw1.act == L.ACT_LRELU and pw1.res is None and pw2.act == L.ACT_NONE
        assert pw2.res_mode == L.RES_PRE_ACT and _same_view(pw2.res, dw.src)       # + v (no activation behind it: pre == post)
        assert _same_view(pw1.src, dw.dst) and _same_view(pw2.src, pw1.dst) and pw1.cin == dw.c and pw2.cin == pw1.cout and pw2.cout == dw.c

    def blobs(self, plan):
        """the two 1x1s as pack_cx_pw's pair, and the blobs of dw7 and pw2 -- not pw1's: no kernel takes a 1x1 as wide as the hidden tensor
        in one launch, the per-op form runs it in slices whose images are the network's"""
        dw, pw1, pw2 = self.replaces
        return [_blob(pw1.w, CX1, pw2.w), (pw2.w + CX2, CX2, (pw1.w, pw2.w))] + dw.blobs(plan) + pw2.blobs(plan)

    def encode(self, op, plan, base, weights):
        dw, pw1, pw2 = self.replaces
        descs.cx_block(self.desc(op), plan.nhw, plan.st, v=_view(dw.src, base), w0=weights[dw.w].data_ptr(), w1=weights[pw1.w + CX1].data_ptr(),
                       w2=weights[pw2.w + CX2].data_ptr(), c=dw.c, m=pw1.cout, cout=pw2.cout, slope=pw1.slope, out=_view(pw2.dst, base),
                       out_width=_stored_width(pw2.dst, pw2.cout))

    def cost(self, plan, desc):             # v read once, the result written once
        dw, pw1, pw2 = self.replaces
        npix, es = plan.npix, plan.esize
        flops = 2.0 * npix * (49 * dw.c + pw1.cin * pw1.cout + pw2.cin * pw2.cout)
        wb = 4.0 * (50 * dw.c + pw1.cin * pw1.cout + pw2.cin * pw2.cout)
        kern = f"cx_block_kernel<{_tf(plan.store == 'bf16')}>"
        stored = float(npix * es * (_stored_channels(dw.src, dw.c, 8) + _stored_channels(pw2.dst, pw2.cout, 8))) + wb
        return _cost(dw.w, kern, dw.c, pw2.cout, 7, flops, float(npix * dw.c * es) + wb, float(npix * es * pw2.cout), stored)


@dataclass
class DwPwPair(_Fused):
    """Team 35's refinement path as ONE esr_dwpw_pair_s16 op -- see Plan.dwpw_pair (dwpw_pair_kernel).  replaces: [dw_a, pw_a, dw_b, pw_b]."""
    kind, OP, what = "dwpw", L.OP_DWPW_PAIR, "depthwise-pointwise pair"

    def check(self):
        sub = self.replaces
        assert len(sub) == 4 and [o.kind for o in sub] == ["dw", "conv", "dw", "conv"]
        dwa, pwa, dwb, pwb = sub
        assert all(o.k == 1 and o.post is None and o.tail is None and not o.hilo and o.hw is None and o.cin == dwa.c and o.cout == dwa.c for o in (pwa, pwb))
        assert all(o.hw is None and o.act == L.ACT_NONE and o.c == dwa.c and o.res_mode == L.RES_PRE_ACT and _same_view(o.res, o.src) for o in (dwa, dwb))
        assert pwa.act == L.ACT_RELU and pwa.res is None and pwb.act == L.ACT_LRELU
        assert pwb.res_mode == L.RES_PRE_ACT and _same_view(pwb.res, dwa.src)       # + x in front of the last activation
        assert _same_view(pwa.src, dwa.dst) and _same_view(dwb.src, pwa.dst) and _same_view(pwb.src, dwb.dst)
        assert not _same_view(pwb.dst, dwa.src)

    def own_blobs(self, plan):                                # pw_a and pw_b
        return [_blob(self.replaces[i].w, DWPW) for i in (1, 3)]

    def encode(self, op, plan, base, weights):
        dwa, pwa, dwb, pwb = self.replaces
        w = [weights[name].data_ptr() for name in (dwa.w, pwa.w + DWPW, dwb.w, pwb.w + DWPW)]
        descs.dwpw_pair(self.desc(op), plan.nhw, plan.st, x=_view(dwa.src, base), w=w, c=dwa.c, slope=pwb.slope, out=_view(pwb.dst, base),
                        out_width=_stored_width(pwb.dst, pwb.cout))

    def cost(self, plan, desc):             # x read once, the result written once
        dwa, pwa, dwb, pwb = self.replaces
        npix, es, c = plan.npix, plan.esize, dwa.c
        flops = 2.0 * npix * 2 * (9 * c + c * c)
        wb = 4.0 * 2 * (10 * c + c * c + c)
        kern = f"dwpw_pair_kernel<{_tf(plan.store == 'bf16')}>"
        stored = float(npix * es * (_stored_channels(dwa.src, c, 8) + _stored_channels(pwb.dst, c, 8))) + wb
        return _cost(dwa.w, kern, c, c, 3, flops, float(npix * c * es) + wb, float(npix * es * c), stored)

    def counted_convs(self, plan):
        return [cv for o in self.replaces for cv in (o.dw_counted(plan) if o.kind == "dw" else o.counted_convs(plan))]


@dataclass
class Unshuffle(_Op):
    """The low-resolution branch of team 35's ESA in one launch (esr_esa_unshuffle_f32) -- see Plan.esa_unshuffle"""
    w: str
    src: Buffer
    dst: Buffer
    f: int
    kind, OP = "unshuffle", L.OP_ESA_UNSHUFFLE
    reads = (("w", UNSHUFFLE),)

    def encode(self, op, plan, base, weights):
        descs.esa_unshuffle(self.desc(op), (plan.n, self.src.h, self.src.w), plan.st, c1=_view(self.src, base), w=weights[self.w].data_ptr(), f=self.f,
                            y=_view(self.dst, base), lo=(self.dst.h, self.dst.w))

    def cost(self, plan, desc):             # the conv1 map read (about 49 / 36 times: the windows overlap), the small map written
        f, npl = self.f, plan.n * self.dst.h * self.dst.w
        return _cost(self.w, f"esa_unshuffle_kernel<{L.STORE[plan.store]}>", 4 * f, f, 1, 2.0 * 4 * f * f * npl,
                     float(plan.n * self.src.h * self.src.w * f * self.src.esize) + 4.0 * (4 * f * f + f), float(npl * L.ESA_FP * 4))

    def counted_convs(self, plan):            # con_ = nn.Conv2d(4 f, f, 1, padding 1): the reference's hooks see its padded output
        return [(4 * self.f, self.f, 1, plan.n * self.dst.h * self.dst.w, L.ACT_RELU)]

    def relu_elements(self, plan):
        """elements of the ReLU in front of con_ (an nn.ReLU call on the pooled 4 f-channel map, which no convolution's count carries)"""
        return 4 * self.f * plan.n * (self.dst.h - 2) * (self.dst.w - 2)


@dataclass
class PaGate(_Op):
    """Pixel attention and the skip behind it in one launch (esr_pa_gate) -- see Plan.pa_gate.  The blob `w + PAG` is pack_pa_gate's."""
    w: str
    src: object
    dst: object                # a Plan.pair() where hilo has L.HILO_OUT
    c: int
    s: object = None           # the tensor added behind the gate (a Plan.pair() where hilo has L.HILO_RES), or None
    hilo: int = 0
    kind, OP = "pagate", L.OP_PA_GATE
    reads = (("w", PAG),)

    def encode(self, op, plan, base, weights):
        s, dst, stride = self.s, self.dst, 0
        if self.hilo:
            pairs = [v for bit, v in ((L.HILO_RES, s), (L.HILO_OUT, dst)) if self.hilo & bit]
            assert not self.hilo & L.HILO_IN and all(isinstance(v, Planar) and len(v.segs) == 2 for v in pairs), "hilo: Plan.pair() buffers"
            strides = {v.stride for v in pairs}
            assert len(strides) == 1, "hilo: pairs of one shape"
            stride = strides.pop()
            s, dst = (v.seg(0) if self.hilo & bit else v for bit, v in ((L.HILO_RES, s), (L.HILO_OUT, dst)))
        descs.pa_gate(self.desc(op), plan.nhw, plan.st, t=_view(self.src, base), w=weights[self.w + PAG].data_ptr(), c=self.c, y=_view(dst, base),
                      y_width=_stored_width(dst, self.c) if plan.st else (self.c + 3) // 4 * 4, s=_view(s, base), hilo=self.hilo, hilo_stride=stride)

    def cost(self, plan, desc):             # t (and s) read once, y written once
        npix, es, c = plan.npix, plan.esize, self.c
        ns = 0 if self.s is None else (2 if self.hilo & L.HILO_RES else 1)
        ny = 2 if self.hilo & L.HILO_OUT else 1
        wb = 4.0 * (c * c + c)
        half = lambda v: v.seg(0) if isinstance(v, Planar) else v
        stored = float(npix * es * (_stored_channels(self.src, c, 8) + (ns * _stored_channels(half(self.s), c, 8) if ns else 0)
                                    + ny * _stored_channels(half(self.dst), c, 8))) + wb
        return _cost(self.w, f"pa_gate_kernel<{L.STORE[plan.store]}>", c, c, 1, 2.0 * npix * c * c, float(npix * es * c * (1 + ns)) + wb,
                     float(npix * es * c * ny), stored)

    def counted_convs(self, plan):            # PA.conv = nn.Conv2d(c, c, 1); its sigmoid and the product have no hook in the reference's counters
        return [(self.c, self.c, 1, plan.npix, L.ACT_NONE)]


@dataclass
class Prelu(_Op):
    """A per-channel PReLU over a concat of up to four views as one streaming launch (esr_prelu) -- see Plan.prelu.  The blob `w + PRELU` is
    pack_prelu's."""
    w: str
    srcs: list                 # [(view, channels), ...] in the concat's order
    dst: object
    kind, OP = "prelu", L.OP_PRELU
    reads = (("w", PRELU),)

    @property
    def c(self):
        return sum(c for _, c in self.srcs)

    def encode(self, op, plan, base, weights):
        assert 1 <= len(self.srcs) <= len(descs.PRELU_SRCS)
        d = self.desc(op)
        descs.prelu(d, plan.nhw, plan.st, srcs=[(_view(v, base), c) for v, c in self.srcs], a=weights[self.w + PRELU].data_ptr(), y=_view(self.dst, base))
        if not L.lib().esr_prelu_supported(ctypes.byref(d)):
            raise L.EsrError(f"{self.w}: esr_prelu does not take this descriptor")

    def cost(self, plan, desc):             # every source read once, the dense result written once
        npix, es, c = plan.npix, plan.esize, self.c
        g = 16 // es
        vec = all(n % g == 0 for _, n in self.srcs)
        rd = float(npix * es * c) + 4.0 * c
        return _cost(self.w, f"prelu_kernel<{L.STORE[plan.store]}, {_tf(vec)}>", c, c, 1, float(npix * c), rd, float(npix * es * c),
                     rd + float(npix * es * _stored_channels(self.dst, c, g)))

    def prelu_elements(self, plan):           # the reference's counters add one flop per element of an nn.PReLU's output
        return self.c * plan.npix


@dataclass
class ResdbStep(_Fused):
    """A ResDB step as ONE esr_resdb_step op -- see Plan.resdb_step (resdb_step_kernel).  replaces: [the PReLU over cat(x, earlier distilled
    maps), the expansion 1x1's `res` part, its distilled part, the PReLU of res, the 3x3 with the residual x]; whole: the name under which
    the network packs the expansion 1x1 as ONE image, its `res` rows, then its distilled rows."""
    whole: str = None
    kind, OP, what = "resdb", L.OP_RESDB_STEP, "ResDB step"

    def check(self):
        sub = self.replaces
        assert len(sub) == 5 and [o.kind for o in sub] == ["prelu", "conv", "conv", "prelu", "conv"]
        pe, cr, cd, pc, c3 = sub
        assert all(o.post is None and o.tail is None and not o.hilo and o.act == L.ACT_NONE for o in (cr, cd, c3))
        assert cr.k == 1 and cd.k == 1 and c3.k == 3 and _same_view(cr.src, pe.dst) and _same_view(cd.src, pe.dst) and cr.res is None and cd.res is None
        assert len(pc.srcs) == 1 and _same_view(pc.srcs[0][0], cr.dst) and _same_view(c3.src, pc.dst)
        assert c3.res_mode == L.RES_PRE_ACT and _same_view(c3.res, pe.srcs[0][0]) and cr.cin == cd.cin == pe.c and pc.c == cr.cout == c3.cin

    def own_blobs(self, plan):                                # the slopes of both PReLUs, cat(a_e, a_c), under the first one's name; the whole expansion is the network's image
        return [_blob(self.replaces[0].w, RSTEP, self.replaces[3].w), _blob(self.whole, S16)]

    def encode(self, op, plan, base, weights):
        pe, cr, cd, pc, c3 = self.replaces
        (x, cin), extras = pe.srcs[0], pe.srcs[1:]
        descs.resdb_step(self.desc(op), plan.nhw, plan.st, x=_view(x, base), extras=[_view(v, base) for v, _ in extras],
                         a=weights[pe.w + RSTEP].data_ptr(), w_e=weights[self.whole + S16].data_ptr(), w_c=weights[c3.w + S16].data_ptr(), cin=cin,
                         cout=c3.cout, extra_channels=sum(c for _, c in extras), dists=_view(cd.dst, base), dists_channels=cd.cout, y=_view(c3.dst, base))

    def cost(self, plan, desc):             # x and the earlier distilled maps read once, the step's distilled maps and x' written once
        pe, cr, cd, pc, c3 = self.replaces
        npix, es = plan.npix, plan.esize
        cin, n, nd = pe.c, c3.cout, cd.cout
        macs = cin * (n + nd) + 9 * n * n
        ntiles = plan.n * ((plan.h + 15) // 16) * ((plan.w + 15) // 16)
        nch, nx = cin // 16, (cin - n) // 16
        # executed: v_mfma_f32_16x16x32 steps per tile -- the `res` rows on the 21 pixel groups of the staged 18 x 18, the distilled rows and the
        # 3x3's five tap pairs x three chunks on the tile's 16 rows
        fexec = 2.0 * ntiles * 8192 * (21 * nch * 3 + 16 * nch * (nd // 16) + 16 * 15 * 3)
        kern = f"resdb_step_kernel<{_tf(plan.store == 'bf16')}, {nx}, {nd // 16}>"
        rd = float(npix * es * cin) + 4.0 * macs
        wr = float(npix * es * (n + nd))
        return _cost(pe.w, kern, cin, n, 3, 2.0 * npix * macs + npix * (cin + n), rd, wr, rd + wr, fexec)


@dataclass
class ConvPrelu(_Fused):
    """A dense 64 -> 64 3x3 and the per-channel PReLU behind it as ONE esr_conv_prelu op -- see Plan.conv_prelu (conv_prelu_kernel).
    replaces: [conv, prelu]."""
    kind, OP, what = "convprelu", L.OP_CONV_PRELU, "conv + PReLU"

    def check(self):
        sub = self.replaces
        assert len(sub) == 2 and [o.kind for o in sub] == ["conv", "prelu"]
        cv, pl = sub
        assert cv.k == 3 and cv.act == L.ACT_NONE and cv.res is None and cv.post is None and cv.tail is None and not cv.hilo and cv.hw is None
        assert cv.dst1 is None and cv.border is None and not cv.split and not isinstance(cv.src, (str, Planar)) and cv.cin_alg == cv.cin
        assert len(pl.srcs) == 1 and _same_view(pl.srcs[0][0], cv.dst) and pl.c == cv.cout      # the PReLU reads what the 3x3 stores ...
        assert not _same_view(pl.dst, cv.src)                                                    # ... and the result is another tensor than the input

    def encode(self, op, plan, base, weights):
        cv, pl = self.replaces
        descs.conv_prelu(self.desc(op), plan.nhw, plan.st, x=_view(cv.src, base), w=weights[cv.w + S16].data_ptr(), a=weights[pl.w + PRELU].data_ptr(),
                         cin=cv.cin, cout=cv.cout, y=_view(pl.dst, base))

    def cost(self, plan, desc):             # the input read once, the activated result written once; the raw result never exists
        cv, pl = self.replaces
        npix, es, c = plan.npix, plan.esize, cv.cout
        wb = 4.0 * (9 * cv.cin * c + 2 * c)
        rd, wr = float(npix * es * cv.cin) + wb, float(npix * es * c)
        ntiles = plan.n * ((plan.h + 15) // 16) * ((plan.w + 15) // 16)
        fexec = 2.0 * ntiles * 256 * 10 * cv.cin * c       # five tap pairs (ten tap slots) per chunk on whole 16 x 16 tiles
        return _cost(cv.w, f"conv_prelu_kernel<{_tf(plan.store == 'bf16')}>", cv.cin, c, 3, 2.0 * npix * 9 * cv.cin * c + npix * c, rd, wr, rd + wr, fexec)


@dataclass
class MdsaGate(_Fused):
    """The end of an MDSA block as ONE esr_mdsa_gate op -- see Plan.mdsa_gate (mdsa_gate_kernel).  replaces: [the fuse 1x1 over
    cat(f1, f2, f3), its PReLU, the replicated one-channel gate (a 1x1 of x with res_mode L.RES_GATE on the PReLU's result)]; sa: the
    one-channel gate's own leaf, which the replicated 1x1 is made from."""
    sa: str = None
    kind, OP, what = "mdsagate", L.OP_MDSA_GATE, "MDSA gate"

    def check(self):
        sub = self.replaces
        assert len(sub) == 3 and [o.kind for o in sub] == ["conv", "prelu", "conv"]
        cf, pl, gt = sub
        assert all(o.act == L.ACT_NONE and o.post is None and o.tail is None and not o.hilo and o.hw is None and o.dst1 is None and o.border is None
                   for o in (cf, gt))
        assert cf.k == 1 and gt.k == 1 and cf.res is None and cf.cin_alg == cf.cin and gt.cin == gt.cout == cf.cout == pl.c
        assert len(pl.srcs) == 1 and _same_view(pl.srcs[0][0], cf.dst)                           # the PReLU reads what the 1x1 stores ...
        assert gt.res_mode == L.RES_GATE and _same_view(gt.res, pl.dst)                          # ... and the gate multiplies its result
        assert not isinstance(gt.src, (str, Planar)) and not isinstance(gt.dst, (str, Planar))

    def own_blobs(self, plan):                                # conv_fuse.0, its slopes and sa.0 as one image, under conv_fuse.0's name
        return [_blob(self.replaces[0].w, MGATE, self.replaces[1].w, self.sa)]

    def encode(self, op, plan, base, weights):
        cf, pl, gt = self.replaces
        f, seg = (cf.src.seg(0), (cf.src.stride, (cf.src.pitch + 15) // 16)) if isinstance(cf.src, Planar) else (cf.src, None)
        descs.mdsa_gate(self.desc(op), plan.nhw, plan.st, f=_view(f, base), x=_view(gt.src, base), w=weights[cf.w + MGATE].data_ptr(), cin=cf.cin,
                        cout=cf.cout, y=_view(gt.dst, base), seg=seg)

    def cost(self, plan, desc):             # f1, f2, f3 and x read once, y written once; the raw 1x1 result and f never exist
        cf, pl, gt = self.replaces
        npix, es, c = plan.npix, plan.esize, cf.cout
        wb = 4.0 * (cf.cin * c + 3 * c + 1)
        rd, wr = float(npix * es * (cf.cin + c)) + wb, float(npix * es * c)
        flops = 2.0 * npix * (cf.cin * c + c) + 2.0 * npix * c
        return _cost(cf.w, f"mdsa_gate_kernel<{_tf(plan.store == 'bf16')}>", cf.cin, c, 1, flops, rd, wr, rd + wr, 2.0 * 2.0 * npix * cf.cin * c)


@dataclass
class PaTail(_Fused):
    """A 3x3 and the pixel attention behind it as ONE esr_pa_tail op -- see Plan.pa_tail (pa_tail_kernel).  replaces: [conv, pagate]."""
    kind, OP, what = "patail", L.OP_PA_TAIL, "pixel-attention tail"

    def check(self):
        sub = self.replaces
        assert len(sub) == 2 and [o.kind for o in sub] == ["conv", "pagate"]
        cv, gate = sub
        assert cv.k == 3 and cv.cin == cv.cout == gate.c and cv.act == L.ACT_NONE and cv.res is None and cv.post is None and cv.tail is None
        assert not cv.hilo and cv.hw is None and cv.dst1 is None and cv.border is None and not isinstance(cv.src, (str, Planar))
        assert _same_view(gate.src, cv.dst)                                         # the gate reads what the 3x3 stores, and nothing else does
        assert not any(_same_view(v, cv.src) for v in ((gate.dst.seg(0), gate.dst.seg(1)) if isinstance(gate.dst, Planar) else (gate.dst,)))

    def encode(self, op, plan, base, weights):
        cv, gate = self.replaces
        gate.encode(op, plan, base, weights)                                        # t's view is replaced by the 3x3's input
        descs.pa_tail(self.desc(op), x=_view(cv.src, base), w3=weights[cv.w + S16].data_ptr(), w=weights[gate.w + PAG].data_ptr())

    def cost(self, plan, desc):             # x (and s) read once, y written once; t never exists
        cv, gate = self.replaces
        g = gate.cost(plan, None)
        c = gate.c
        wb = 4.0 * (9 * c * c + c)
        stored = g["stored_bytes"] - plan.npix * plan.esize * _stored_channels(gate.src, c, 8) + plan.npix * plan.esize * _stored_channels(cv.src, c, 16) + wb
        return _cost(cv.w, f"pa_tail_kernel<{_tf(plan.store == 'bf16')}, {(c + 15) // 16}>", c, c, 3, g["flops"] + 2.0 * plan.npix * 9 * c * c,
                     g["read_bytes"] + wb, g["write_bytes"], stored)


@dataclass
class AsymStep(_Fused):
    """An ARFDB step as ONE esr_asym_step op -- see Plan.asym_step (asym_step_kernel).  replaces: [c_d, the folded first convolutions of the
    two pairs (in -> [a_l | a_m]), the folded second ones (+ the residuals)]; p: the earlier steps' distilled maps (views); taps: the
    leaves of the step's four 3-tap convolutions, [c_l1, c_m1, c_l2, c_m2]."""
    p: list = None
    taps: list = None
    kind, OP, what = "asym", L.OP_ASYM_STEP, "asymmetric-convolution step"

    def check(self):
        sub = self.replaces
        assert len(sub) == 3 and all(o.kind == "conv" and o.post is None and o.tail is None and not o.hilo for o in sub) and len(self.p or ()) <= 2
        cd, ca, cb = sub
        assert cd.k == 1 and ca.k == 3 and cb.k == 3 and cd.act == ca.act == cb.act and cd.slope == ca.slope == cb.slope
        assert _same_view(ca.src, cd.src) and cd.res is None and ca.res is None and ca.cout == 2 * cd.cout and cb.cout == cd.cout
        assert cb.res is None or (_same_view(cb.res, cd.src) and cb.res_mode == L.RES_PRE_ACT and cd.cin == cd.cout)

    def own_blobs(self, plan):                                # the four as one image, under c_l1's name
        return [_blob(self.taps[0], ASYM, *self.taps[1:])]

    def encode(self, op, plan, base, weights):
        cd, ca, cb = self.replaces
        descs.asym_step(self.desc(op), plan.nhw, plan.st, x=_view(cd.src, base), w_d=weights[cd.w + S16].data_ptr(),
                        w_taps=weights[self.taps[0] + ASYM].data_ptr(), cin=cd.cin, c=cd.cout, act=cd.act, slope=cd.slope, res=cb.res is not None,
                        dd=_view(cd.dst, base), y=_view(cb.dst, base), y_width=_stored_width(cb.dst, cb.cout), p=[_view(v, base) for v in self.p or ()])

    def cost(self, plan, desc):             # the step's input (and the earlier distilled maps) read once, d and the result written once
        cd, ca, cb = self.replaces
        npix, es, c = plan.npix, plan.esize, cd.cout
        macs = cd.cin_alg * c + 2 * 3 * cd.cin_alg * c + 2 * 3 * c * c         # the reference's five convolutions
        nkp = 2 if cd.cin > 32 else 1
        # executed: v_mfma_f32_16x16x32 steps (16 x 16 x 32 MACs) per 16 x 16 tile -- d's 16 pixel groups x 1x1 chunks, the 36 groups of a_l and
        # a_m x three taps x K pairs, the 16 rows x six taps of the second convolutions -- x two output tiles
        ntiles = plan.n * ((plan.h + 15) // 16) * ((plan.w + 15) // 16)
        fexec = 2.0 * ntiles * 8192 * 2 * (16 * ((cd.cin + 15) // 16) + 36 * 3 * nkp + 16 * 6)
        kern = f"asym_step_kernel<{_tf(plan.store == 'bf16')}, {nkp}, {_tf(cb.res is not None)}>"
        np_ = len(self.p or ())
        rd = float(npix * es * (cd.cin_alg + np_ * c)) + 4.0 * macs
        stored = float(npix * es * (_stored_channels(cd.src, cd.cin, 16) + (2 + np_) * _stored_channels(cd.dst, c, 16))) + 4.0 * macs
        return _cost(self.taps[0], kern, cd.cin, c, 3, 2.0 * npix * macs, rd, float(npix * es * 2 * c), stored, fexec)


@dataclass
class Apply(_Op):
    """ESA's full-resolution tail (esr_esa_apply_f32) -- see Plan.esa_apply"""
    wf: str
    w4: str
    x: object
    c1: Buffer
    c3: Buffer
    dst: object
    c: int
    f: int
    post: list = None
    skip_y: bool = False
    kind, OP = "apply", L.OP_ESA_APPLY

    def blobs(self, plan):                                    # (the 1x1s riding in the launch are ONE blob, under the first one's name)
        return [_blob(self.wf), _blob(self.w4)] + ([_blob(self.post[0].w, APOST, *(t.w for t in self.post[1:]))] if self.post else [])

    def encode(self, op, plan, base, weights):
        e = self.desc(op)
        e.n, e.h, e.w, e.c, e.f, e.storage = plan.n, plan.h, plan.w, self.c, self.f, L.STORE[plan.store]
        e.h_lo, e.w_lo = self.c3.h, self.c3.w
        e.x, e.y = _view(self.x, base), _view(self.dst, base)
        e.c1 = ctypes.c_void_p(_addr(self.c1, base))
        e.c3 = ctypes.c_void_p(_addr(self.c3, base))
        e.w0 = ctypes.c_void_p(weights[self.wf].data_ptr())
        e.w1 = ctypes.c_void_p(weights[self.w4].data_ptr())
        if self.post:
            e.post_w = ctypes.c_void_p(weights[self.post[0].w + APOST].data_ptr())
            e.skip_y = 1 if self.skip_y else 0
            for k, t in enumerate(self.post):
                pp = e.post[k]
                pp.cout, pp.act, pp.slope = t.cout, t.act, t.slope
                pp.out = _view(t.dst, base)
                if t.res is not None:
                    pp.res_mode, pp.res = L.RES_PRE_ACT, _view(t.res, base)

    def cost(self, plan, desc):                               # conv_f (f x f) + conv4 (f x c) per pixel, x read, y written
        npix, es, c, f = plan.npix, plan.esize, self.c, self.f
        flops = 2.0 * npix * (f * f + f * c)
        rd = float(npix * es * (c + f) + plan.n * self.c3.h * self.c3.w * f * 4)
        wr = 0.0 if self.skip_y else float(npix * es * c)
        kin = c
        for t in self.post or ():                             # 1x1 convolutions in the same launch: their flops, residual reads and stores
            flops += 2.0 * npix * kin * t.cout
            rd += float(npix * es * t.cout) if t.res is not None else 0.0
            wr += float(npix * es * t.cout)
            kin = t.cout
        return _cost("apply", "esa_apply_kernel", 0, 0, 0, flops, rd, wr)

    def counted_convs(self, plan):            # conv_f (f->f) and conv4 (f->c), both full resolution (+ the 1x1s riding in the launch)
        r = [(self.f, self.f, 1, plan.npix, L.ACT_NONE), (self.f, self.c, 1, plan.npix, L.ACT_NONE)]
        kin = self.c
        for t in self.post or ():
            r.append((kin, t.cout, 1, plan.npix, t.act))
            kin = t.cout
        return r


class Plan:
    """Builds the op list for one (N, H, W); see HipSRModel._build_plan in each network.

    `store` is the element type of the FULL-RESOLUTION activation buffers ("f32" | "bf16" | "f16"); the ESA
    low-resolution maps (a few hundred KB) are always fp32.  Offsets are bytes into one workspace."""

    def __init__(self, n, h, w, store="f32"):
        self.n, self.h, self.w = n, h, w
        self.npix = n * h * w
        self.store = store
        self.nhw, self.st = (n, h, w), L.STORE[store]          # as the fills of descs.py take them
        self.esize = 4 if store == "f32" else 2
        self.total = 0         # bytes of the full-resolution arena
        self.total_lo = 0      # bytes of the low-resolution (always fp32) arena.  The two never overlap across plans: a 16-bit plan
                               # laid over another shape's fp32 maps would read their bytes as bf16 / fp16 -- Inf / NaN patterns included
        self.buffers = []
        self.ops = []          # op records (Conv, Dw, ...) until finalize()

    def cpad(self, c):
        """channel pitch of a full-resolution buffer holding c channels: whole K chunks of the conv kernels
        (8 fp32 channels, 16 16-bit channels = 32 bytes either way)."""
        m = 8 if self.esize == 4 else 16
        return (c + m - 1) // m * m

    def buffer(self, name, pitch, h=None, w=None, blocked=False):
        """Full-resolution buffer by default; (h, w) gives a low-resolution fp32 one (ESA maps).  blocked: channel-blocked
        [n][pitch / 8][h][w][8] (fp32 plans; only as the dst1 of a split store and the input of the fused IMDB tail)."""
        lowres = h is not None
        assert not blocked or (self.esize == 4 and not lowres and pitch % 8 == 0)
        esize = 4 if lowres else self.esize
        assert (pitch * esize) % 16 == 0
        h = self.h if h is None else h
        w = self.w if w is None else w
        size = (self.n * h * w * pitch * esize + 255) // 256 * 256
        if lowres:
            b = Buffer(name, pitch, self.total_lo, h, w, esize, arena=1)
            self.total_lo += size
        else:
            b = Buffer(name, pitch, self.total, h, w, esize, blocked=blocked)
            self.total += size
        self.buffers.append(b)
        return b

    def release(self, bufs):
        """Gives back full-resolution buffers that no op of the plan addresses (a fused op made the launches between which they lived
        unnecessary).  They must be the plan's LAST allocations, in order: the arena then simply ends in front of them, and no other
        buffer moves or falls outside it -- anything else raises."""
        k = len(bufs)
        if not k or len(self.buffers) < k or any(a is not b or b.arena != 0 for a, b in zip(self.buffers[-k:], bufs)):
            raise L.EsrError("Plan.release: only the plan's last full-resolution allocations can be given back")
        del self.buffers[-k:]
        self.total = bufs[0].offset

    def planar(self, name, nseg, seg_pitch):
        """nseg equal full-resolution buffers back to back (see Planar); 16-bit plans only"""
        assert self.esize == 2 and seg_pitch % 8 == 0            # (whole 16-byte granules; a tight pitch -- 56 -- is not whole K chunks)
        return Planar([self.buffer(f"{name}.{j}", seg_pitch) for j in range(nseg)])

    def pair(self, name, pitch):
        """a hi + lo pair (esr_conv_desc.hilo): value = seg(0) + seg(1), two dense bf16 tensors `stride` bytes apart"""
        return self.planar(name, 2, pitch)

    def conv(self, wname, src, dst, cin, cout, **kw):
        """A convolution; the keywords are Conv's fields.  A 16-bit plan's 3x3 of the network input becomes pack + conv_s16: the NCHW
        fp32 input is first packed to 16-bit hi / lo slots (esr_pack_input_s16), the head convolution then runs on conv_s16_kernel
        with hi / lo weights (`<name>#head#s16`, engine.pack_head_s16)."""
        o = Conv(wname, src, dst, cin, cout, **kw)
        if src is INPUT and self.esize == 2 and o.k == 3 and dst is not OUTPUT:
            x16 = self.buffer('in16', 16)
            self.ops.append(Pack(x16, cin))
            o.src, o.head, o.w = x16, cin, wname + HEAD
        self.ops.append(o)

    def dwconv(self, wname, src, dst, c, **kw):
        self.ops.append(Dw(wname, src, dst, c, **kw))

    def dwconv7(self, wname, src, dst, c):
        """nn.Conv2d(c, c, 7, 1, 3, groups=c) with bias, every storage (esr_dwconv7x7); `wname` names a pack_dw7 blob.  dst is another
        tensor than src."""
        self.ops.append(Dw7(wname, src, dst, c))

    def bsconv(self, pw, dw, src, dst, cin, c, **kw):
        self.ops.append(Bs(pw, dw, src, dst, cin, c, **kw))

    def conv3x3s2(self, wname, src, dst, f):
        self.ops.append(S2(wname, src, dst, f))

    def maxpool7s3(self, src, dst):
        self.ops.append(Pool(src, dst))

    def maxpool7s7(self, src, dst):
        self.ops.append(Pool7(src, dst))

    def esa_lowres(self, mark, c1, pooled, dst, f, s2, layers):
        """ESA's low-resolution branch as ONE op (esr_esa_lowres_f32: two launches with halo recompute) in place of the ops appended
        since `mark = len(plan.ops)` -- conv3x3s2, maxpool7s3 and the 1..3 small 3x3 layers (RFDN / RLFN: dense convs, BSRN: pointwise +
        depthwise pairs); or, with s2 = None, EFDN's maxpool7s7, conv_2, conv_3 and conv_23 (layers: one kind-2 pair and one kind-3 layer);
        those ops stay attached as `replaces`: the complexity counters and the algorithmic costs are theirs.
        layers: [EsaLayer, ...]"""
        self.ops[mark:] = [Lowres(self.ops[mark:], c1, pooled, dst, f, s2, layers)]

    def _fuse(self, mark, fused, **kw):
        """ONE `fused` op (a _Fused class) in place of the ops appended since `mark`, if its kernel takes them; says whether it did -- if
        not, the ops stay as they are.  The kernel's predicate decides, on the descriptor finalize() will launch: `encode` fills it
        against a null workspace and stand-in weights (_AnyBlob; no blob exists yet in HipSRModel._repack's plan), with n = 1: a batch
        and its single images take the same kernels."""
        assert self.esize == 2
        o = fused(self.ops[mark:], **kw)
        o.check()
        probe = L.Op()
        o.encode(probe, self, (0, 0), _AnyBlob())
        getattr(probe, L.LAUNCHERS[o.OP][1]).n = 1
        if not o.supported(probe):
            return False
        self.ops[mark:] = [o]
        return True

    def post_supported(self, o):
        """Does the 16-bit post chain of the Conv `o` (not appended yet) run fused?  esr_conv_post_supported, asked as _fuse asks: about the
        descriptor `o.encode` fills against a null workspace and stand-in weights, with n = 1 -- a batch and its single images take the
        same kernels.  A network appends `o` as it is (plan.ops.append) or its convolutions one by one."""
        assert self.esize == 2 and o.kind == "conv" and o.post is not None
        try:
            o.encode(L.Op(), Plan(1, self.h, self.w, self.store), (0, 0), _AnyBlob())
        except L.EsrError:
            return False
        return True

    def chain(self, mark):
        """The 3x3 convolutions appended since `mark = len(plan.ops)` -- a residual block's chain src -> t1 -> ... -> (+ src) -> post 1x1 ->
        post2 1x1, RLFB's c1_r -> c2_r -> c3_r -> c5 -> esa.conv1 (team04_rlfn.py:109-122) -- as ONE esr_conv_chain_s16 op (16-bit plans):
        the intermediate tensors stay in LDS (rlfb_chain_kernel).  The Conv ops stay attached as `replaces`: weights, complexity
        counters and algorithmic costs are theirs; the result is bit-identical to running them one by one."""
        return self._fuse(mark, Chain)

    def hfab(self, mark):
        """The four 3x3 convolutions appended since `mark = len(plan.ops)` -- FMEN's HFAB with one BasicBlock, x -> squeeze -> conv -> conv ->
        sigmoid(excitate) * x (team03_fmen.py:60-73) -- as ONE esr_conv_chain_s16 op with res_mode L.RES_GATE (hfab_kernel, 16-bit plans): x is
        read once, t1 .. t3 stay in LDS.  The Conv ops stay attached as `replaces` (weights, complexity counters, algorithmic costs); the
        result is bit-identical to running them one by one."""
        return self._fuse(mark, Chain, gate=True)

    def distill_step(self, mark):
        """The three convolutions appended since `mark = len(plan.ops)` -- a BMDB distillation step in its per-op form, d = relu(c_d(r)),
        t = c_b(d) (+ r), r' = relu(c_r(r) + t) (team37_bmdn.py:155-171) -- as ONE esr_distill_step_s16 op (16-bit plans): r is read once, d
        and r' are written once, t never exists (the two 3x3s are one over cat[r, d]: engine.pack_distill_s16, blob `<c_r>#fold`).  The Conv
        ops stay attached as `replaces`: weights, complexity counters and algorithmic costs are theirs.  Not bit-identical to them: the per-op
        form rounds t to the storage type."""
        return self._fuse(mark, Distill)

    def resblock_head(self, mark):
        """The convolutions appended since `mark = len(plan.ops)` -- the head of ESAN's residual block in its per-op form, [x = xin + g as an
        identity 1x1 with the residual xin,] t = relu(conv1(x)), u = conv2(t), c1 = ESA.conv1(u) (team34_esan.py:71-76, :49) -- as ONE
        esr_resblock_head_s16 op (16-bit plans): xin and g are read once, x, u and c1 written once, t never exists.  The Conv ops stay
        attached as `replaces`: weights, complexity counters and algorithmic costs are theirs.  x must not be stored over xin or g: the
        neighbouring tiles read their halo."""
        return self._fuse(mark, ResHead)

    def refine_cascade(self, mark):
        """The four convolutions appended since `mark = len(plan.ops)` -- FRFDB's refinement path behind d2 in its per-op form,
        r2 = lrelu(c2_r(d2) + d2), d3 = lrelu(c3_d(r2)), r3 = lrelu(c3_r(d3) + d3), r4 = lrelu(c4(r3) + r3) (team25_frfdn/block.py:115-122) --
        as ONE esr_refine_cascade_s16 op (16-bit plans): d2 is read once, d3 and r4 are written once, r2 and r3 never exist.  The Conv ops stay
        attached as `replaces`: weights, complexity counters and algorithmic costs are theirs; the result is bit-identical to running them
        one by one.  d3 and r4 must not be stored into d2's tensor: the neighbouring tiles read its halo."""
        return self._fuse(mark, Cascade)

    def cx_block(self, mark):
        """The three ops appended since `mark = len(plan.ops)` -- a ConvNeXt block in its per-layer form, t = dw7(v), h = lrelu(pw1(t)),
        out = pw2(h) + v (team38_rfdnext/rfdn_block.py:132-144) -- as ONE esr_cx_block_s16 op (16-bit plans): v is read once, out is
        written once, t and the 4x-wide h never exist.  The ops stay attached as `replaces`: complexity counters and algorithmic costs are
        theirs; the 1x1 blobs are pack_cx_pw's (`<pw1>#cx1`, `<pw2>#cx2`).  Not bit-identical to the per-layer launches: the 1x1 weights
        are rounded once where conv_s16_kernel multiplies by hi + lo pairs.  out must not be stored into v's tensor."""
        return self._fuse(mark, CxBlock)

    def dwpw_pair(self, mark):
        """The four ops appended since `mark = len(plan.ops)` -- the refinement path of team 35's RFDB in its per-op form, u1 = dw3_a(x) + x,
        h = relu(pw_a(u1)), u2 = dw3_b(h) + h, r = lrelu(pw_b(u2) + x) (team35_rfdn/rmsrb1.py:22-27, :199-210) -- as ONE esr_dwpw_pair_s16 op
        (16-bit plans): x is read once, r is written once, u1, h and u2 never exist.  The ops stay attached as `replaces`: complexity
        counters and algorithmic costs are theirs; the 1x1 blobs are pack_dwpw_pw's (`<pw>#dwpw`).  Not bit-identical to the four launches:
        the 1x1 weights are rounded once where conv_s16_kernel multiplies by hi + lo pairs.  r must not be stored into x's tensor."""
        return self._fuse(mark, DwPwPair)

    def esa_unshuffle(self, wname, c1, dst, f):
        """c3 = relu(con_(relu(max_pool2d(pixel_unshuffle(c1, 2), 7, 3)))) (team35_rfdn/rmsrb1.py:140-144) in one launch, every storage
        (esr_esa_unshuffle_f32); `wname` names a pack_unshuffle blob; dst is the low-resolution fp32 map [n][h3 + 2][w3 + 2][16]."""
        self.ops.append(Unshuffle(wname, c1, dst, f))

    def pa_gate(self, wname, src, dst, c, s=None, hilo=0):
        """dst = src * sigmoid(W . src + b) (+ s): a pixel attention (team10_repafdn/block.py:151-166) and the tensor added behind it in one
        launch, every storage (esr_pa_gate); `wname + PAG` names a pack_pa_gate blob of the plan's storage.  hilo (16-bit plans): L.HILO_RES --
        s is a Plan.pair(), L.HILO_OUT -- dst is one.  dst is another tensor than src and s."""
        self.ops.append(PaGate(wname, src, dst, c, s, hilo))

    def prelu(self, wname, srcs, dst):
        """dst = prelu(cat(srcs), a): an nn.PReLU with one slope per channel in front of a convolution (team43_resdn.py:54-83), every storage
        (esr_prelu), v >= 0 ? v : a v with any fp32 slope.  srcs: [(view, channels), ...], at most four, in the order of the torch.cat that
        never runs; dst: a dense tensor that is none of the sources; `wname + PRELU` names a pack_prelu blob of all the channels' slopes."""
        self.ops.append(Prelu(wname, list(srcs), dst))

    def resdb_step(self, mark, whole):
        """The five ops appended since `mark = len(plan.ops)` -- a ResDB step in its per-layer form, u = prelu(cat(x, ..)), r = W_e[:48] . u,
        dists = W_e[48:] . u, t = prelu(r), x' = x + W_c (*) t (resdn.py; team43_resdn.py:93-106) -- as ONE esr_resdb_step op (16-bit plans): x
        and the earlier distilled maps are read once, dists and x' are written once, u, r and t never exist.  The ops stay attached as
        `replaces`: complexity counters and algorithmic costs are theirs; the blobs are the 3x3's and the WHOLE expansion's esr_pack_conv_s16
        images (`<whole>#s16`: the network's) and pack_prelu(cat(a_e, a_c)) (`<expansion.0>#step`).  It stores what the five launches store, up to
        the summation order of the fp32 sums.  x' must not be stored into x's tensor."""
        return self._fuse(mark, ResdbStep, whole=whole)

    def conv_prelu(self, mark):
        """The two ops appended since `mark = len(plan.ops)` -- a dense 64 -> 64 3x3 and the per-channel PReLU of its result, raw = conv(x),
        f = prelu(raw, a) (mdgn.py; team24_mdgn.py:8-10) -- as ONE esr_conv_prelu op (16-bit plans): x is read once, f is written once, raw stays
        in the accumulators.  The ops stay attached as `replaces`: complexity counters and algorithmic costs are theirs; the blobs are the
        3x3's esr_pack_conv_s16 image and the PReLU's pack_prelu slopes, as the two launches read them.  Not bit-identical to the two launches,
        which round raw once in between: here the activation meets the fp32 sum and the result is rounded once.  f must not be stored into
        x's tensor."""
        return self._fuse(mark, ConvPrelu)

    def mdsa_gate(self, mark, sa):
        """The three ops appended since `mark = len(plan.ops)` -- the end of an MDSA block in its per-layer form, raw = W_f . cat(f1, f2, f3),
        t = prelu(raw, a_f), y = sigmoid(w_s . x) * t (mdgn.py; team24_mdgn.py:26-28) -- as ONE esr_mdsa_gate op (16-bit plans): f1, f2, f3 and x
        are read once, y is written once, raw and t never exist.  The ops stay attached as `replaces`: complexity counters and algorithmic
        costs are theirs; the blob is pack_mdsa_gate's (`<conv_fuse.0>#mgate`), of conv_fuse.0, its PReLU and the gate's leaf `sa`.  Not bit-identical
        to the three launches, which round raw and t: here one rounding, at the store.  y must not be stored into a source's tensor."""
        return self._fuse(mark, MdsaGate, sa=sa)

    def pa_tail(self, mark):
        """The two ops appended since `mark = len(plan.ops)` -- a plain 3x3 and the pixel attention that reads its result, t = conv(x),
        y = t * sigmoid(W . t + b) (+ s) (team10_repafdn/repafdn.py:55-57) -- as ONE esr_pa_tail op (16-bit plans): x (and s) are read once, y
        is written once, t stays in the accumulators.  The ops stay attached as `replaces`: weights, complexity counters and algorithmic
        costs are theirs.  Not bit-identical to the two launches, which round t once in between: the sums differ by at most half a storage
        step of t times the gate before the last rounding -- one step of y without s, more of y's own steps where t g and s cancel
        (include/esr_hip.h: esr_pa_tail).  y must not be stored into x's tensor."""
        return self._fuse(mark, PaTail)

    def asym_step(self, mark, taps, p=None):
        """The three convolutions appended since `mark = len(plan.ops)` -- an ARFDB step in its per-layer form, d = act(c_d(r)), [a_l | a_m] =
        act(P (*) r), r' = act(Q (*) [d .. | a_l | a_m] (+ r)) (arfdn.py; team14_arfdn/block.py:233-254) -- as ONE esr_asym_step op (16-bit
        plans): r is read once, d and r' are written once, a_l and a_m never exist; p: the views of the earlier steps' distilled maps that
        Q adds through identity taps (at most two).  The Conv ops stay attached as `replaces`: complexity counters and algorithmic costs
        are theirs; the 3-tap blob is pack_asym_s16's (`<c_l1>#asym`) of the leaves taps = [c_l1, c_m1, c_l2, c_m2].  Not bit-identical to the three launches: another summation order,
        and the 3-tap weights are rounded once where pack_conv_s16 diffuses the rounding error over a 3x3's taps.  r' must not be stored
        into r's tensor."""
        return self._fuse(mark, AsymStep, p=list(p or ()), taps=list(taps))

    def esa_apply(self, wf, w4, x, c1, c3, dst, c, f, **kw):
        """y = x * sigmoid(conv4(bilinear(c3) + conv_f(c1)));  two nn.Conv2d calls of the reference.
        post (16-bit plans): [Post(w, dst, cout, act, slope, res), ...] -- one or two 1x1 convolutions evaluated in the same launch
        (esr_esa_desc.post[]): the first on y as stored, the second on the first's fp32 result; their weights are ONE blob
        `<post[0].w>#apost` (engine.pack_apply_post; a chain of scaled or folded weights is packed by the network).  skip_y: y itself is not stored (nothing but the chain
        reads it)."""
        self.ops.append(Apply(wf, w4, x, c1, c3, dst, c, f, **kw))

    def finalize(self, workspace, weights):
        """weights: name -> device blob tensor (16-bit-storage plans: `name#s16` for the NHWC convs).  Returns
        (Op array, indices of the ops that read the network input, indices of the ops that write the output)."""
        arr = (L.Op * len(self.ops))()
        base = workspace if isinstance(workspace, tuple) else ((workspace if isinstance(workspace, int) else (workspace.data_ptr() if workspace is not None else 0)), self.total_lo)
        for i, o in enumerate(self.ops):
            o.encode(arr[i], self, base, weights)
            if isinstance(o, _Fused) and not o.supported(arr[i]):
                raise L.EsrError(f"{o.cost(self, None)['name']}: no {o.what} kernel for this shape (the plan should have kept separate ops)")
        in_idx = [i for i, o in enumerate(self.ops) if getattr(o, "src", None) is INPUT]
        out_idx = [i for i, o in enumerate(self.ops) if getattr(o, "dst", None) is OUTPUT]
        return arr, in_idx, out_idx


# ---- torch.library custom op -------------------------------------------------------------------------------------------
# `model(x)` goes through ONE registered operator, esr::sr_forward(x, handle) -> y, so that graph capture / FakeTensor
# tracing / torch.compile see an opaque op with a shape function instead of ctypes calls: the "thin PyTorch-ROCm custom-op
# layer" the drop-in modules sit on.  The real implementation replays the fused op list through the C ABI; the fake (meta)
# implementation only computes the output shape.  `handle` identifies the live module: a key from a process-wide counter handed out
# at construction and never reused (an `id()` can be recycled by another object once its owner is collected); the registry holds
# weak references, so an entry disappears with its module.
_LIVE = weakref.WeakValueDictionary()
_HANDLES = itertools.count(1)


@torch.library.custom_op("esr::sr_forward", mutates_args=())
def sr_forward(x: torch.Tensor, handle: int) -> torch.Tensor:
    m = _LIVE.get(handle)
    if m is None:
        raise L.EsrError(f"esr::sr_forward: no live model with handle {handle}")
    return m._forward_impl(x)


@sr_forward.register_fake
def _sr_forward_fake(x, handle):
    m = _LIVE.get(handle)
    if m is None:
        raise L.EsrError(f"esr::sr_forward: no live model with handle {handle}")
    if x.dim() != 4:
        raise L.EsrError("expected a 4-D float32 NCHW tensor (uint2tensor4 output)")
    return x.new_empty((x.shape[0], m.out_nc, x.shape[2] * m.upscale, x.shape[3] * m.upscale), dtype=torch.float32)


class _ModelLock:
    """threading.RLock that survives copy.deepcopy / pickling of the module that owns it (a copy gets a lock of its own)."""

    def __init__(self):
        self._l = threading.RLock()

    def __enter__(self):
        return self._l.__enter__()

    def __exit__(self, *a):
        return self._l.__exit__(*a)

    def __deepcopy__(self, memo):
        return _ModelLock()

    def __reduce__(self):
        return (_ModelLock, ())


class _Entry:
    """One cached shape: the Plan, its esr_op array finalized against workspace base `base`, and (after the second forward of the
    shape on this stream) the HIP graph of its launches (esr_graph_create)."""
    __slots__ = ("plan", "arr", "in_idx", "out_idx", "base", "graph", "uses")

    def __init__(self, plan):
        self.plan, self.arr, self.in_idx, self.out_idx, self.base = plan, None, (), (), None
        self.graph, self.uses = None, 0

    def drop_graph(self):
        if self.graph is not None:
            L.lib().esr_graph_destroy(self.graph)
            self.graph = None
        self.uses = 0

    def __del__(self):
        try:
            self.drop_graph()
        except Exception:          # interpreter shutdown: the library may be gone
            pass


class _StreamCtx:
    """What a forward needs that is private to ONE HIP stream: the workspace, the plans finalized against it and the
    per-kernel event sets.  Two forwards of the same model enqueued on two streams run concurrently on the GPU, so they must
    not share activation buffers; the packed weights (read-only) are shared."""
    __slots__ = ("plans", "ws", "ws_owner", "lo_cap", "profs")

    def __init__(self):
        self.plans = collections.OrderedDict()   # (n, c, h, w, device) -> _Entry, LRU
        self.ws = None             # ONE grow-only workspace (all cached plans lay their buffers out in it)
        self.ws_owner = None       # key of the plan that ran last in the workspace (None: content unknown -> zero before use)
        self.lo_cap = 0            # bytes reserved in front of the workspace for the plans' low-resolution fp32 maps (grow-only)
        self.profs = {}

    def drop_profs(self):
        """destroys the per-kernel event sets"""
        for prof in self.profs.values():
            L.lib().esr_prof_destroy(prof)
        self.profs = {}


def _mark_dirty_hook(module, incompatible):
    """HipSRModel's load_state_dict post hook.  A module-level function: the hook table is part of what copy.deepcopy / pickle carry, and
    the hook marks the module it is called on -- a copy's load re-packs the copy, not its source."""
    module._mark_dirty()


def _wb(m, path):
    leaf = m._leaf(path)
    return leaf.weight, leaf.bias


def _pack_dense_cat(m, store, path):
    """a 3x3 over the pair's concat: the two halves' inputs at rows 0 and 16 (esr_esa_layer kind 3)"""
    w, bias = _wb(m, path)
    w, f = _host(w), w.shape[1] // 2
    w32 = torch.zeros(w.shape[0], 2 * L.ESA_FP, 3, 3)
    w32[:, :f], w32[:, L.ESA_FP:L.ESA_FP + f] = w[:, :f], w[:, f:]
    return pack_dense(w32, bias, 2 * L.ESA_FP, L.ESA_FP)


def _pack_dw_pad16(m, store, path):
    w, bias = _wb(m, path)
    w16, b16 = torch.zeros(16, 1, 3, 3), torch.zeros(16)
    w16[:len(w)] = _host(w)
    if bias is not None:
        b16[:len(w)] = _host(bias)
    return pack_dw(w16, b16)


# kind -> packer(model, storage, *source leaf paths): how HipSRModel._repack builds a blob that an op of its plan names (_Op.blobs)
_PACKERS = {
    S16: lambda m, st, p: pack_conv_s16(*_wb(m, p), st, cin_map=m._cin_map(p, m._conv_specs[p][3], st)),
    POST: lambda m, st, p: pack_post_s16(*_wb(m, p), st),
    HEAD: lambda m, st, p: pack_head_s16(*_wb(m, p), st),
    APOST: lambda m, st, p, p2=None: pack_apply_post(*_wb(m, p), *(_wb(m, p2) if p2 else (None, None)), st),
    DENSE: lambda m, st, p: pack_dense(*_wb(m, p), L.ESA_FP, L.ESA_FP),
    DENSE_CAT: _pack_dense_cat,
    DWPAD: _pack_dw_pad16,
    DW7: lambda m, st, p: pack_dw7(*_wb(m, p)),
    UNSHUFFLE: lambda m, st, p: pack_unshuffle(*_wb(m, p)),
    FOLD: lambda m, st, r, b: pack_distill_s16(*_wb(m, r), *_wb(m, b), st),
    CX1: lambda m, st, p1, p2: pack_cx_pw(*_wb(m, p1), *_wb(m, p2), st)[0],
    CX2: lambda m, st, p1, p2: pack_cx_pw(*_wb(m, p1), *_wb(m, p2), st)[1],
    DWPW: lambda m, st, p: pack_dwpw_pw(*_wb(m, p), st),
    PAG: lambda m, st, p: pack_pa_gate(*_wb(m, p), st),
    ASYM: lambda m, st, *taps: pack_asym_s16(*(t for p in taps for t in _wb(m, p)), st),
    PRELU: lambda m, st, p: pack_prelu(m._leaf(p).weight),
    RSTEP: lambda m, st, e, c: pack_prelu(torch.cat([_host(m._leaf(e).weight), _host(m._leaf(c).weight)])),
    MGATE: lambda m, st, cf, a, sa: pack_mdsa_gate(*_wb(m, cf), m._leaf(a).weight, *_wb(m, sa), st),
}
# the generic images: derived only from a leaf registered in _conv_specs (_add_conv without custom=True) -- a leaf outside it, or a name that
# is no leaf at all, is the network's to pack in _extra_pack.  The dedicated packers above take any registered leaf.
_GENERIC = (S16, POST, HEAD, APOST)


class HipSRModel(nn.Module):
    """Base of the drop-in nn.Modules.  Subclasses register reference-compatible parameters
    with `_add_conv` and describe their forward with `_build_plan`."""

    def __init__(self):
        super().__init__()
        self._conv_specs = {}      # path -> (cin, cout, k, cin_map)
        self._dense_specs = {}     # path -> (cin_p, cout_p): small ESA weights in the plain dense layout
        self._dw_specs = []        # depthwise 3x3 parameter paths
        self._packed = None        # path -> device blob
        self._packed_sig = None
        self._dirty = True         # parameters may have changed since the last repack (load_state_dict / .to() / repack())
        self._ctxs = {}            # (device, HIP stream handle) -> _StreamCtx: workspace + plans of the forwards enqueued on that stream
        self.compute = "f32"       # "f32" | "bf16" | "f16": MFMA operand format of the full-resolution 3x3 convs
        self._fuse_esa_lowres = True  # ESA's low-resolution branch as one esr_esa_lowres_f32 op (two launches) instead of 3 .. 8 launches
        self._winograd = True      # fp32 plans: 3x3 convs whose shape qualifies run as Winograd F(2x2, 3x3) (esr_conv_desc.wino_wpacked)
        self._hilo_skip = True     # bf16 plans: the long skip's tensors (`fea`, `out_lr`) as hi + lo pairs (esr_conv_desc.hilo; Plan.hilo_skip)
        self._fuse_tail = True     # 16-bit RFDN plans: RFDB's c4 -> cat -> c5 -> esa.conv1 as one launch (rfdb_tail_kernel, ABI v12)
        self._tight_pitch = True   # 16-bit RFDN plans: nf-wide tensors at pitch round_up(nf, 8) instead of whole K chunks (56 for nf = 50; esr_conv2d_s16: tight pitch)
        self._fuse_chain = True    # 16-bit plans: a block's 3x3 chain as one esr_conv_chain_s16 launch where a kernel exists (Plan.chain)
        self._fuse_step = True     # 16-bit BMDN plans: a distillation step as one esr_distill_step_s16 launch (Plan.distill_step); measured: DESIGN.md 7d
        self._fuse_head = True     # 16-bit ESAN plans: a residual block's head as one esr_resblock_head_s16 launch (Plan.resblock_head); measured: DESIGN.md 7e
        self._fuse_cascade = False # 16-bit FasterRFDN plans: FRFDB's refinement path as one esr_refine_cascade_s16 launch (Plan.refine_cascade); OFF: faster on one image, not at 32 x 256 x 256
        self._fuse_pair = True     # 16-bit DWRFDN plans: the depthwise-pointwise refinement path as one esr_dwpw_pair_s16 launch (Plan.dwpw_pair); measured: DESIGN.md 7h
        self._fuse_pa_tail = False # 16-bit RePAFDN plans: LR_conv and the pixel attention behind it as one esr_pa_tail launch (Plan.pa_tail); OFF: 2 % slower than the two launches at 32 x 256 x 256 and on one image
        self._fuse_asym = True     # 16-bit ARFDN plans: an ARFDB step as one esr_asym_step launch (Plan.asym_step); measured: DESIGN.md 7k
        self._fuse_resdb = False   # 16-bit ResDN plans: a ResDB step as one esr_resdb_step launch (Plan.resdb_step); OFF: 1.8x slower than the five launches at 32 x 256 x 256, 1.5x on one image
        self._fuse_conv_prelu = True   # 16-bit MDGN plans: a 3x3 and the PReLU behind it as one esr_conv_prelu launch (Plan.conv_prelu); ON: 1.3 .. 1.5 % faster than the two launches at 32 x 256 x 256 (repeat spread 0.6 %), 5 .. 6 % on one image; next to fuse_mdsa_gate 1.4 % / 0.1 % (f16: inside the spread) and 9 %
        self._fuse_mdsa_gate = True    # 16-bit MDGN plans: the fuse 1x1, its PReLU and the sigmoid gate as one esr_mdsa_gate launch (Plan.mdsa_gate); ON: 21 % faster than the three launches at 32 x 256 x 256, 29 % on one image
        self._fuse_cx = True       # 16-bit RFDNeXt plans: the ConvNeXt block as one esr_cx_block_s16 launch (Plan.cx_block); measured: DESIGN.md 7g
        self.use_graphs = True     # forwards of at most GRAPH_MAX_PIXELS input pixels replay a captured HIP graph (esr_graph_launch)
        self._lock = _ModelLock()       # plan / workspace bookkeeping and the pointer patch + enqueue of one forward (see _forward_impl)
        self._prof_passes = 0      # >0: record HIP events around every op (bench roofline leg)
        self.handle = next(_HANDLES)       # the `handle` argument of esr::sr_forward
        _LIVE[self.handle] = self
        self.register_load_state_dict_post_hook(_mark_dirty_hook)

    # -- copies: copy.copy / copy.deepcopy / pickle (torch.save(model)) all go through these two -----------------
    def __getstate__(self):
        """What a copy carries: parameters, specs, compute mode and flags.  Not the runtime state derived from them -- the packed blobs,
        the per-stream workspaces, plans, esr_op arrays (raw device pointers), HIP graphs and event sets stay with the source, and the
        `handle` names the source alone."""
        state = self.__dict__.copy()
        state.update(_packed=None, _packed_sig=None, _dirty=True, _ctxs={})
        del state["handle"]
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        self.handle = next(_HANDLES)
        _LIVE[self.handle] = self

    # -- parameter registration: same key names as the reference state_dict -------------------
    def _add_leaf(self, path, leaf):
        """registers `leaf` under the dotted `path`, creating the nested containers on the way"""
        parts = path.split(".")
        mod = self
        for p in parts[:-1]:
            if p not in mod._modules:
                mod.add_module(p, nn.Module())
            mod = mod._modules[p]
        mod.add_module(parts[-1], leaf)

    def _add_conv(self, path, cin, cout, k, cin_map=None, linear=False, dense=None, stride=1, padding=None, custom=False):
        """Create nested containers so that `path + '.weight'` / `path + '.bias'` are the
        state_dict keys (e.g. 'model.1.sub.0.conv1.0').  The leaf is an nn.Conv2d / nn.Linear
        used purely as a parameter holder with the reference's shapes and default init."""
        self._add_leaf(path, nn.Linear(cin, cout) if linear else nn.Conv2d(cin, cout, k, stride, (k - 1) // 2 if padding is None else padding))
        if dense is not None:
            self._dense_specs[path] = dense
        elif not custom:
            self._conv_specs[path] = (cin, cout, k, cin_map)

    def _add_dw(self, path, c):
        """depthwise nn.Conv2d(c, c, 3, 1, 1, groups=c) parameter holder (`path.weight` is [c,1,3,3])."""
        self._add_leaf(path, nn.Conv2d(c, c, 3, 1, 1, groups=c))
        self._dw_specs.append(path)

    def _leaf(self, path):
        mod = self
        for p in path.split("."):
            mod = mod._modules[p]
        return mod

    # Plan-shaping switches: which blobs repack() builds and which ops _build_plan emits depend on them, so a change re-packs and drops
    # the cached plans exactly like set_compute() (as plain attributes a late change was ignored or raised KeyError).
    def _set_flag(self, name, value):
        value = bool(value)
        with self._lock:               # (another thread may be inside forward(): plans / profiler handles must not vanish under it)
            if getattr(self, name) != value:
                setattr(self, name, value)
                self._dirty = True
                self._drop_plans()

    fuse_esa_lowres = property(lambda self: self._fuse_esa_lowres, lambda self, v: self._set_flag("_fuse_esa_lowres", v))
    winograd = property(lambda self: self._winograd, lambda self, v: self._set_flag("_winograd", v))
    hilo_skip = property(lambda self: self._hilo_skip, lambda self, v: self._set_flag("_hilo_skip", v))
    fuse_chain = property(lambda self: self._fuse_chain, lambda self, v: self._set_flag("_fuse_chain", v))
    fuse_tail = property(lambda self: self._fuse_tail, lambda self, v: self._set_flag("_fuse_tail", v))
    tight_pitch = property(lambda self: self._tight_pitch, lambda self, v: self._set_flag("_tight_pitch", v))
    fuse_step = property(lambda self: self._fuse_step, lambda self, v: self._set_flag("_fuse_step", v))
    fuse_head = property(lambda self: self._fuse_head, lambda self, v: self._set_flag("_fuse_head", v))
    fuse_cascade = property(lambda self: self._fuse_cascade, lambda self, v: self._set_flag("_fuse_cascade", v))
    fuse_cx = property(lambda self: self._fuse_cx, lambda self, v: self._set_flag("_fuse_cx", v))
    fuse_pa_tail = property(lambda self: self._fuse_pa_tail, lambda self, v: self._set_flag("_fuse_pa_tail", v))
    fuse_pair = property(lambda self: self._fuse_pair, lambda self, v: self._set_flag("_fuse_pair", v))
    fuse_resdb = property(lambda self: self._fuse_resdb, lambda self, v: self._set_flag("_fuse_resdb", v))
    fuse_asym = property(lambda self: self._fuse_asym, lambda self, v: self._set_flag("_fuse_asym", v))
    fuse_conv_prelu = property(lambda self: self._fuse_conv_prelu, lambda self, v: self._set_flag("_fuse_conv_prelu", v))
    fuse_mdsa_gate = property(lambda self: self._fuse_mdsa_gate, lambda self, v: self._set_flag("_fuse_mdsa_gate", v))

    def _skip_hilo(self, plan, c):
        """bf16 plans: keep the long skip `upsampler(LR_conv(body) + fea)` in hi + lo pairs?  (c = its channel count; the hi + lo kernels
        exist for 3 and 4 output tiles.)  Two bf16 roundings of the image itself cost 0.03-0.09 dB on near-detail-free content, the pairs
        bring that to <= 0.003 dB (LAB_NOTES 9.4; tools/emulate_skip.py)."""
        return bool(self._hilo_skip) and plan.store == "bf16" and (c + 15) // 16 in (3, 4)

    def set_compute(self, mode):
        """'f32': exact fp32 MFMA, fp32 activations.  'bf16' / 'f16' (BASELINE.json configs [2]-[4]): the full-resolution
        activations are STORED in that type and are the MFMA operands as they are (v_mfma_f32_16x16x32), accumulation,
        bias, residual and activation stay fp32, one rounding per stored value; the NCHW input / output and the ESA
        low-resolution branch stay fp32."""
        if mode not in L.COMPUTE:
            raise ValueError(f"compute must be one of {sorted(L.COMPUTE)}")
        with self._lock:
            if mode != self.compute:
                self.compute = mode
                self._dirty = True
        return self

    def _store(self):
        """storage type of the full-resolution activations for the current compute mode"""
        return self.compute

    # -- packing ------------------------------------------------------------------------------
    GRAPH_MAX_PIXELS = 4 * 512 * 512   # larger forwards are GPU-bound by a wide margin: esr_run_ops
    MAX_PLANS = 128                # DIV2K has ~100 distinct LR shapes; a plan is a few tens of KB of host memory
    # Plans of different shapes lay their buffers out in ONE workspace, so after a shape switch another shape's activations lie where
    # this plan keeps its pad channels.  That is harmless: every pad slot is only ever multiplied by a zero weight (packers), added
    # to an accumulator nobody stores, or copied into another pad slot -- stale FINITE values of the SAME element type cannot reach a
    # result (bit-identical outputs in every mode: tools/dbg/rezero_probe.py, test_hundred_shapes_one_workspace, and for every form the
    # engine plans under hostile finite patterns tests/test_gpu_stale_workspace.py).  Same type is what
    # the two arenas of a Plan are for: the low-resolution fp32 maps of all plans live in front of the workspace (`_lo_cap` bytes),
    # the full-resolution buffers behind them, so a 16-bit plan never reads another shape's fp32 bytes (Inf / NaN patterns).
    # Re-zeroing 130 MB per forward was 26 us of a 0.7 ms image (every DIV2K image has its own shape): +3 % in DIV2K mode (A/B).
    # Set True to isolate forwards from a previous one whose activations overflowed to Inf / NaN.
    rezero_on_switch = False

    def _mark_dirty(self):
        self._dirty = True

    def invalidate_workspaces(self):
        """Forget what the per-stream workspaces hold: the next forward on each stream zero-fills before it runs.  For callers that
        saw a non-finite output (overflowing activations in a 16-bit mode): with rezero_on_switch = False another shape's pad
        channels may lie where Inf / NaN were stored, and 0 * Inf = NaN would reach its results."""
        with self._lock:
            for ctx in self._ctxs.values():
                ctx.ws_owner = None

    def _apply(self, fn, *args, **kwargs):          # .to() / .cuda() / .float(): parameters move or change
        self._dirty = True
        return super()._apply(fn, *args, **kwargs)

    def _signature(self):
        return tuple((p.data_ptr(), p._version, p.device) for p in self.parameters())

    def _drop_plans(self):
        with self._lock:
            for ctx in self._ctxs.values():
                ctx.drop_profs()
                for ent in ctx.plans.values():
                    ent.drop_graph()
                ctx.plans.clear()
                ctx.ws_owner = None

    MAX_STREAMS = 16               # contexts kept (LRU): bench.py's DIV2K mode uses 8 streams + the default stream of the replay leg; the
                                   # least recently USED context beyond that is dropped (its workspace is freed, its plans are rebuilt on return)

    def _ctx(self, device):
        """The context of the CURRENT HIP stream of `device` (torch.cuda.stream(...) selects it, like every torch op)."""
        key = (device, torch.cuda.current_stream(device).cuda_stream)
        ctx = self._ctxs.pop(key, None)
        if ctx is None:
            ctx = _StreamCtx()
        self._ctxs[key] = ctx          # (re)inserted at the end: dict order = least recently used first
        while len(self._ctxs) > self.MAX_STREAMS:
            self._ctxs.pop(next(iter(self._ctxs))).drop_profs()
        return ctx

    # the default-stream context under its historical names (tests, tools)
    def _ctx0(self):
        dev = next(self.parameters()).device
        return self._ctxs.get((dev, torch.cuda.default_stream(dev).cuda_stream)) or _StreamCtx()

    _plans = property(lambda self: self._ctx0().plans)
    _ws = property(lambda self: self._ctx0().ws)

    def _cin_map(self, path, cin_map, store):
        """physical-slot -> logical-channel map of a conv reading a padded concat buffer; networks whose slice padding
        depends on the storage type override this"""
        return cin_map

    def repack(self, device):
        with self._lock:
            self._repack(device)

    def _repack(self, device):
        store = self._store()
        # the blobs the ops of the current mode read (_Op.blobs): one plan of a small shape has every op the network emits
        plan = Plan(1, 32, 32, store)
        self._build_plan(plan, self.in_nc)
        want = {name: (o, kind, srcs) for o in plan.ops[::-1] for name, kind, srcs in o.blobs(plan)}      # (of a blob's readers, the first op)
        packed = {}
        # every registered leaf's own image, read or not
        for path, (cin, cout, k, cin_map) in self._conv_specs.items():
            leaf = self._leaf(path)
            packed[path] = pack_conv(leaf.weight, leaf.bias, cin_map=self._cin_map(path, cin_map, "f32")).to(device)
            if k == 3 and self.winograd and store == "f32" and cin >= 32 and cout <= 64:
                packed[path + WINO] = pack_wino(leaf.weight, leaf.bias, cin_map=self._cin_map(path, cin_map, "f32")).to(device)
        for path, (cin_p, cout_p) in self._dense_specs.items():
            packed[path] = pack_dense(*_wb(self, path), cin_p, cout_p).to(device)
        for path in self._dw_specs:
            packed[path] = pack_dw(*_wb(self, path)).to(device)
        # what the ops name beyond that
        for name, (o, kind, srcs) in want.items():
            spec = self._conv_specs.get(srcs[0])
            own = kind not in _GENERIC or (spec is not None and not (kind == HEAD and spec[3]))      # (a head over a cin_map: custom-packed)
            if kind in _PACKERS and own:
                packed[name] = _PACKERS[kind](self, store, *srcs).to(device)
        self._extra_pack(packed, device)
        for name, (o, kind, srcs) in reversed(want.items()):      # (in the plan's order)
            if name not in packed:
                raise L.EsrError(f"{type(self).__name__}: op {o.cost(plan, None)['name']!r} ({o.kind}) reads the blob {name!r}, which neither the engine nor _extra_pack built")
        if torch.device(device).type == "cuda":
            torch.cuda.synchronize(device)           # the blobs are read by forwards on ANY stream from here on
        self._packed = packed
        self._packed_sig = self._signature()
        self._dirty = False
        self._drop_plans()

    def _extra_pack(self, packed, device):
        pass

    def _pack_own(self, packed, device, name, w, bias, wino=False):
        """A network's own weights (folded, scaled, sliced ...) under `name`, as a Conv reads a leaf's: the fp32 image, and `#s16` in a 16-bit
        mode; wino: `#wino` where the engine would build a leaf's"""
        store = self._store()
        packed[name] = pack_conv(w, bias).to(device)
        if store != "f32":
            packed[name + S16] = pack_conv_s16(w, bias, store).to(device)
        elif wino and self.winograd:
            packed[name + WINO] = pack_wino(w, bias).to(device)

    # -- forward ------------------------------------------------------------------------------
    def _build_plan(self, plan):
        raise NotImplementedError

    def _ensure_packed(self, device):
        """Weights are re-packed after load_state_dict ON THE MODEL / .to() / set_compute / a plan-shaping flag (dirty flag) or when
        the blobs live on another device.  Not tracked: a load_state_dict on a sub-module (`model.B1.load_state_dict(...)`: the post
        hook is the model's own, a container's load never reaches it) and in-place edits of a parameter's storage (`p.copy_()` under
        no_grad, an optimizer step) -- the next forward still runs the old blobs.  Call repack(device) after them."""
        if self._packed is None or self._dirty or next(iter(self._packed.values())).device != device:
            self.repack(device)

    def _entry(self, key, ctx=None):
        """Cached plan for (n, c, h, w, device) in the current stream's context: built on first use, finalized against that
        context's workspace."""
        n, c, h, w, device = key
        if ctx is None:
            ctx = self._ctx(device)
        ent = ctx.plans.get(key)
        if ent is None:
            plan = Plan(n, h, w, self._store())
            self._build_plan(plan, c)
            ent = _Entry(plan)
            ctx.plans[key] = ent
            while len(ctx.plans) > self.MAX_PLANS:
                old, _ = ctx.plans.popitem(last=False)
                prof = ctx.profs.pop(old, None)
                if prof is not None:
                    L.lib().esr_prof_destroy(prof)
        else:
            ctx.plans.move_to_end(key)
        if ent.plan.total_lo > ctx.lo_cap:
            ctx.lo_cap = ent.plan.total_lo             # the low-resolution arena grows: every plan's full-resolution buffers move
            ctx.ws_owner = None
        need = max(ctx.lo_cap + ent.plan.total, 256)
        if ctx.ws is None or ctx.ws.device != device or ctx.ws.numel() < need:
            ctx.ws = None                                               # release before the larger allocation
            ctx.ws = torch.zeros(need, dtype=torch.uint8, device=device)
            ctx.ws_owner = key                                          # fresh zeros: this plan's pad channels are 0
        base = (ctx.ws.data_ptr(), ctx.lo_cap)
        if ent.base != base:
            ent.drop_graph()                        # (the captured launches hold the old workspace addresses)
            ent.arr, ent.in_idx, ent.out_idx = ent.plan.finalize(base, self._packed)
            ent.base = base
        if ctx.ws_owner is None:
            ctx.ws.zero_()              # unknown content (plans dropped: another storage type's bytes; the arenas moved)
        elif ctx.ws_owner != key and self.rezero_on_switch:
            ctx.ws.zero_()              # isolation requested
        ctx.ws_owner = key
        return ent

    def prepare(self, shape, device=None):
        """Everything a forward of an [N, C, H, W] input needs besides the kernels themselves: weight packing (first
        call, or after load_state_dict / .to()), plan construction, workspace growth and zero fill.  Callers that time
        `model(x)` with an event pair (test_demo.py:429-432) call this first so that the bracket holds only the
        esr_run_ops launches; forward() does the same work itself when it was not called."""
        device = torch.device(device) if device is not None else next(self.parameters()).device
        if device.type != "cuda":
            raise L.EsrError(f"{type(self).__name__}.prepare: device {device} -- this engine only runs on an MI355X")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        n, c, h, w = (int(v) for v in shape)
        with self._lock:
            self._ensure_packed(device)
            return self._entry((n, c, h, w, device))

    def forward(self, x):
        """NCHW fp32 [N, in_nc, H, W] on the GPU -> NCHW fp32 [N, out_nc, 4H, 4W]: one esr::sr_forward call."""
        if (type(x) is torch.Tensor and x.is_cuda and not torch.compiler.is_compiling()
                and torch._C._get_tracing_state() is None and torch._C._len_torch_dispatch_stack() == 0):
            # plain eager call on a real tensor: straight to the C ABI (the registered operator costs ~8 us of dispatch per call -- a
            # fifth of a graph-launched forward's host time).  torch.jit.trace, make_fx, any active TorchDispatchMode (FlopCounterMode,
            # profiler modes), FakeTensor and torch.compile go through esr::sr_forward below: they must SEE the operator
            return self._forward_impl(x)
        return torch.ops.esr.sr_forward(x, self.handle)         # (a copy has a handle of its own: __setstate__)

    def _forward_impl(self, x):
        if not x.is_cuda:
            raise L.EsrError(f"{type(self).__name__}: input is on {x.device}; this engine only runs on an "
                             "MI355X through libesr_hip.so and has no CPU fallback (use oracle/ for CPU checks)")
        if x.dtype != torch.float32 or x.dim() != 4:
            raise L.EsrError("expected a 4-D float32 NCHW tensor (uint2tensor4 output)")
        lib = L.lib()
        x = x.contiguous()
        n, c, h, w = x.shape
        key = (n, c, h, w, x.device)
        y = torch.empty((n, self.out_nc, h * self.upscale, w * self.upscale), dtype=torch.float32, device=x.device)
        if n == 0:
            return y                        # an empty batch: nn.Conv2d returns an empty tensor too (nothing to launch: a grid of 0 blocks is an error)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        # One lock per model around the host-side bookkeeping AND the enqueue: the cached esr_op array of a (stream, shape) carries
        # this call's x / y pointers from the patch below until esr_run_ops has read it (it only enqueues: ~0.1-0.25 ms of host
        # time, no device wait), and plan / workspace creation mutates dicts.  Two Python threads calling one model therefore
        # enqueue their forwards one after the other -- on their own streams the forwards still overlap on the GPU.
        with self._lock:
            self._ensure_packed(x.device)
            ctx = self._ctx(x.device)
            ent = self._entry(key, ctx)
            arr = ent.arr
            for i in ent.in_idx:
                arr[i].conv.inp.ptr = x.data_ptr()
            for i in ent.out_idx:
                arr[i].conv.out0.ptr = y.data_ptr()
            if self._prof_passes > 0:
                prof = ctx.profs.get(key)
                if prof is None:
                    prof = ctypes.c_void_p()
                    L.check(lib.esr_prof_create(len(arr), self._prof_passes, ctypes.byref(prof)), "esr_prof_create")
                    ctx.profs[key] = prof
                rc = lib.esr_run_ops_profiled(arr, len(arr), ctypes.c_void_p(stream), prof)
            elif self.use_graphs and n * h * w <= self.GRAPH_MAX_PIXELS:
                # small forwards (one image: test_demo.py:416-433) are host-bound -- 20-35 launches at 5-8 us each: from the second
                # forward of a (stream, shape) on, the launches are replayed as ONE hipGraphLaunch with x / y patched (esr_graph_launch)
                ent.uses += 1
                if ent.graph is None and ent.uses >= 2:
                    gh = ctypes.c_void_p()
                    rc = lib.esr_graph_create(arr, len(arr), ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.byref(gh))
                    if rc == L.ESR_OK:
                        ent.graph = gh
                    else:
                        ent.uses = -(1 << 30)      # this plan's launches cannot be captured: stay on esr_run_ops
                if ent.graph is not None:
                    rc = lib.esr_graph_launch(ent.graph, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), ctypes.c_void_p(stream))
                else:
                    rc = lib.esr_run_ops(arr, len(arr), ctypes.c_void_p(stream))
            else:
                rc = lib.esr_run_ops(arr, len(arr), ctypes.c_void_p(stream))
        L.check(rc, f"{type(self).__name__}.forward")
        return y

    # -- per-kernel timing (HIP events on the launch stream; see esr_run_ops_profiled) ---------
    def enable_profiling(self, max_passes):
        self.disable_profiling()
        self._prof_passes = int(max_passes)

    def disable_profiling(self):
        with self._lock:
            for ctx in self._ctxs.values():
                ctx.drop_profs()
            self._prof_passes = 0

    def op_costs(self, plan, arr=None):
        """Per op of `plan`: device kernel symbol, ALGORITHMIC flops (2 x MACs of the matrix products the op stands
        for) and ALGORITHMIC HBM bytes (every input slice / residual / weight read once, every output written once,
        at the storage type of the buffer) -- the numerators of bench.py's roofline leg.  arr: the finalized
        esr_op array (kernel variants that depend on the descriptor)."""
        return [o.cost(plan, None if arr is None else arr[i]) for i, o in enumerate(plan.ops)]

    def collect_profile(self):
        """After a device synchronise: list of dicts {name, kernel, flops, read_bytes, write_bytes, ms_sum, passes} per
        op, summed over the recorded passes of every cached shape."""
        out = []
        for ctx in self._ctxs.values():
            for key, prof in ctx.profs.items():
                ent = ctx.plans.get(key)
                if ent is None or ent.arr is None:
                    continue
                n = len(ent.arr)
                ms = (ctypes.c_double * n)()
                passes = ctypes.c_int(0)
                L.check(L.lib().esr_prof_collect(prof, ms, n, ctypes.byref(passes)), "esr_prof_collect")
                buf = ctypes.create_string_buffer(256)
                for i, c in enumerate(self.op_costs(ent.plan, ent.arr)):
                    c.update(ms_sum=ms[i], passes=passes.value, shape=key[:4], label=c["kernel"])
                    # the device symbol the library launched for this op (rocprofv3's spelling); `label` keeps the descriptive name
                    if L.lib().esr_prof_kernel_symbol(prof, i, buf, 256) == 0 and buf.value:
                        c["kernel"] = buf.value.decode()
                    out.append(c)
        return out

    def _complexity_terms(self, plan, o):
        """(flops, activations, n_conv) that the reference's model_summary hooks would count for op `o`."""
        flops = acts = nconv = 0
        for (cin, cout, k, npix, act) in self._counted_convs(plan, o):
            flops += k * k * cin * cout * npix
            acts += cout * npix
            nconv += 1
            if act in (L.ACT_LRELU, L.ACT_RELU):
                flops += cout * npix
        return flops, acts, nconv

    def _counted_convs(self, plan, o):
        """nn.Conv2d calls of the REFERENCE graph that op `o` stands for: (cin, cout, k, pixels, act) tuples
        (logical channel counts as the reference's hooks see them)."""
        return o.counted_convs(plan)

    def workspace_bytes(self, n, h, w, c=3):
        plan = Plan(n, h, w, self._store())
        self._build_plan(plan, c)
        return plan.total + plan.total_lo
