"""The frame the networks share: the sizes and maps of their layouts, the input check, and three small builders that a
`_build_plan` calls where the reference has its ESA low-resolution branch (EsaBranch), its long skip (LongSkip) and a torch.cat (Concat).
The builders allocate and append exactly what the networks used to spell out, in that order; what is specific to a network stays in its file.
"""
import torch

from . import _lib as L
from .engine import INPUT, OUTPUT, EsaLayer, Planar, pack_dense

FP = L.ESA_FP


def _pad8(c):
    return (c + 7) // 8 * 8


def _lowres(h, w):
    """sizes of ESA's maps: the 3x3 / stride 2 convolution without padding, then max_pool2d(7, stride 3)"""
    h2, w2 = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return h2, w2, (h2 - 7) // 3 + 1, (w2 - 7) // 3 + 1


def _pool7(h, w):
    """size of max_pool2d(7, stride 7, padding 1) (team05_efdn/plainblock.py:143)"""
    return (h - 5) // 7 + 1, (w - 5) // 7 + 1


def _slice_map(n_slices, logical, padded):
    """physical slot -> logical channel for `n_slices` slices of `logical` channels padded to `padded`."""
    return [(s // padded) * logical + s % padded if s % padded < logical else -1 for s in range(n_slices * padded)]


def block_cin_map(model, path, cin_map, store):
    """HipSRModel._cin_map of the RFDN family: c.0 reads block-output slices as wide as the storage type's K chunks"""
    if path == 'c.0':
        return _slice_map(model.num_modules, model.nf, _pad8(model.nf) if store == "f32" else (model.nf + 15) // 16 * 16)
    return cin_map


def check_input(name, plan, c, in_nc, esa=True):
    if c != in_nc:
        raise L.EsrError(f'{name} expects {in_nc} input channels, got {c}')
    if esa and (plan.h < 15 or plan.w < 15):
        raise L.EsrError('ESA needs H, W >= 15 (3x3/s2 then 7x7/s3 pooling)')


def set_scale(self, scale_idx):
    """the reference models' no-op setter, for the classes whose reference has one"""
    self.scale_idx = scale_idx


def identity_conv_f(f, device):
    """ESA without conv_f: c3 + c1_ == c3 + conv_f(c1_) with conv_f = identity (esr_esa_apply_f32 always applies one)"""
    return pack_dense(torch.eye(f)[:, :, None, None], torch.zeros(f), FP, FP).to(device)


class EsaBranch:
    """ESA's maps -- conv1's (`c1`, full resolution), the stride-2 map and the two pooled-size maps `a`, `b` -- and its low-resolution branch."""

    def __init__(self, plan, f):
        self.plan, self.f = plan, f
        h2, w2, h3, w3 = _lowres(plan.h, plan.w)
        self.hw = (h3, w3)
        self.c1 = plan.buffer('esa_c1', FP)
        self.s2 = plan.buffer('esa_s2', FP, h2, w2)
        self.a, self.b = plan.buffer('esa_a', FP, h3, w3), plan.buffer('esa_b', FP, h3, w3)

    def lowres(self, conv2, layers, fuse):
        """conv2 (3x3 / stride 2) of c1, the pooling into `a`, then the dense 3x3 `layers` [(weight name, act), ...] ping-ponging between
        `a` and `b`; fuse: all of it as one op of two launches (Plan.esa_lowres: halo recompute; only the pooled map reaches memory).
        Returns the map that holds c3."""
        plan, f = self.plan, self.f
        mark = len(plan.ops)
        plan.conv3x3s2(conv2, self.c1, self.s2, f)
        plan.maxpool7s3(self.s2, self.a)
        src, dst = self.a, self.b
        for w, act in layers:
            plan.conv(w, src, dst, f, f, act=act, hw=self.hw)
            src, dst = dst, src
        if fuse:
            plan.esa_lowres(mark, self.c1, self.a, src, f, conv2, [EsaLayer(0, act, w) for w, act in layers])
        return src


class LongSkip:
    """upsampler(LR_conv(body) + fea): `fea` and `out_lr` as hi + lo pairs where the model keeps the skip that way in a bf16 plan
    (HipSRModel._skip_hilo; Plan.pair: two dense tensors), else `fea` as one buffer and the LR conv's output in a buffer of the network's."""

    def __init__(self, plan, model, c, pitch, name='fea', pair_pitch=None):
        self.plan, self.c = plan, c
        self.hl = model._skip_hilo(plan, c)
        if self.hl:
            self.dst = plan.pair(name, pair_pitch or pitch)
            self.fea, self.out = self.dst.seg(0), plan.pair('out_lr', pair_pitch or pitch)
        else:
            self.dst = self.fea = plan.buffer(name, pitch)

    def head(self, wname, cin, **kw):
        """the convolution of the network input that produces `fea`"""
        self.plan.conv(wname, INPUT, self.dst, cin, self.c, hilo=L.HILO_OUT if self.hl else 0, **kw)

    def close(self, lr_conv, up, src, scratch, cout, conv=None):
        """LR_conv(src) + fea, then the upsampler convolution with the pixel shuffle in its store.  scratch: where the sum goes when it is not
        a pair; conv: what appends the LR conv in place of plan.conv (BSRN's is a BSConvU)"""
        plan, c = self.plan, self.c
        conv = conv or plan.conv
        if self.hl:
            conv(lr_conv, src, self.out, c, c, res=self.dst, res_mode=L.RES_PRE_ACT, hilo=L.HILO_RES | L.HILO_OUT)
            plan.conv(up, self.out, OUTPUT, c, cout, hilo=L.HILO_IN)
        else:
            conv(lr_conv, src, scratch, c, c, res=self.fea, res_mode=L.RES_PRE_ACT)
            plan.conv(up, scratch, OUTPUT, c, cout)


class Concat:
    """A torch.cat of `nseg` maps that never runs: `planar` (16-bit plans) -- nseg dense tensors (engine.Planar); else channel slices,
    `seg_pitch` apart, of one buffer of `pitch` (default nseg * seg_pitch) channels.  seg(j) is what a producer writes, `whole` what the 1x1
    behind the concat reads."""

    def __init__(self, plan, name, nseg, seg_pitch, planar, pitch=None):
        self.seg_pitch = seg_pitch
        self.whole = plan.planar(name, nseg, seg_pitch) if planar else plan.buffer(name, pitch or nseg * seg_pitch)

    def seg(self, j):
        if isinstance(self.whole, Planar):
            return self.whole.seg(j)
        return self.whole[j * self.seg_pitch:(j + 1) * self.seg_pitch]
