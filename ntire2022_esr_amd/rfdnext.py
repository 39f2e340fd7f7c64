"""RFDNeXt (x4) on the HIP engine -- drop-in for `models.team38_rfdnext.RFDN.RFDN` (RFDN.py:38-68; NTIRE 2022 ESR team 38, test_demo.py
data_range 1.0) with block_type "RFDB" and act_type "lrelu".

Same constructor keywords and the same 96 state_dict keys (`fea_conv`, `B{k}.c{1,2,3}_d`, `B{k}.c{1,2,3}_r`, `B{k}.c4`, `B{k}.c5`,
`B{k}.esa.conv.{0,1,3}`, `c.0`, `LR_conv`, `upsampler.0`).  An RFDN at nf = 50 / dc = 25 whose refinement path is dc wide and whose block
ends in a ConvNeXt block instead of ESA (rfdn_block.py:146-185), every activation LeakyReLU(0.05):

    dc_1 = c1_d . x                 rc_1 = c1_r (*) x + dc_1              (no activation)
    dc_2 = c2_d . rc_1              rc_2 = c2_r (*) rc_1 + rc_1           (no activation)
    dc_3 = c3_d . rc_2              rc_3 = lrelu(c3_r (*) rc_2 + rc_2)
    rc_4 = c4 (*) rc_3
    v    = c5 . lrelu(cat[dc_1, dc_2, dc_3, rc_4])                        100 -> 50
    out  = CX(v) = pw2 . lrelu(pw1 . dw7(v) + b1) + b2 + v                esa.conv.{0, 1, 3}: depthwise 7x7, 50 -> 200, 200 -> 50

then c.0 (1x1 200 -> 50, lrelu) over the four block outputs, LR_conv + fea, upsampler.0 and the pixel shuffle stored directly.  No ESA: no
H, W >= 15 limit.  The layouts are rfdn.py's at nf = 50: nf-wide tensors at pitch 56 (16-bit plans, tight pitch) or whole K chunks, the
25-channel maps in 32-wide tensors, the concat as four dense 32-wide segments (engine.Planar; one 128-wide buffer in fp32) read by c5 through
`_slice_map`, the block outputs as four 56-wide tensors read by c.0, the long skip as a hi + lo pair in bf16 -- torch.cat never runs.

The activation sits on the concat, so dc_1, dc_2, dc_3 and rc_4 are STORED ACTIVATED.  dc_1 is also needed raw inside rc_1: c1_d is folded
into the centre tap of c1_r when packing (engine.fold_center: W_r + centre(W_d), b_r + b_d, summed in fp32; blob `B{k}.c1_r#fold`), so rc_1
is one existing 3x3 without a residual and c1_d is launched only in its activated form.  The complexity counters still see c1_d and c1_r.

The ConvNeXt block has two forms (model.fuse_cx):
  per-op   dwconv7 (esr_dwconv7x7) -> 1x1 + lrelu -> 1x1 with v as the residual.  The first 1x1 has 200 outputs; conv_f32_kernel stops at
           64 and conv_s16_kernel at four output tiles, so the plan splits it into output-channel slices that write channel slices of one
           hidden buffer (fp32: 56 + 56 + 56 + 32 of pitch 200; 16-bit: 64 + 64 + 64 + 8 of pitch 208), weights sliced in _extra_pack
           (`B{k}.esa.conv.1#o{j}`).  The only form of an fp32 plan.
  fused    ONE esr_cx_block_s16 launch (cx_block_kernel; Plan.cx_block): v is read once, out written once: 224 bytes per pixel where the
           per-op form moves 1728 as stored (about 1360 algorithmically: the four slices each re-read t).  Within one rounding per stage of the per-op form, not bit-identical to it (its 1x1 weights are rounded once).
           ON by default: in bf16 a forward takes 5.91 against 12.85 ms at 32 x 256 x 256 and 0.876 against 1.468 ms on one 339 x 510
           image, the repeats at most 0.6 % apart.
Which form a plan takes depends on the per-image shape and esr_cx_block_supported only, never on the batch size.

The long skip (RFDN.py:64) and the two concats are the shared frame's (frame.py).
"""
import torch

from . import _lib as L
from .engine import HipSRModel, fold_center
from .frame import Concat, LongSkip, _pad8, _slice_map, block_cin_map, check_input, set_scale


def _hidden_slices(cmid, store):
    """(first channel, width) of the output-channel slices of the per-op first 1x1: fp32 -- conv_f32_kernel takes up to 64 outputs, slices of
    56 keep the offsets on whole 8-channel chunks; 16-bit -- conv_s16_kernel takes up to four 16-channel output tiles"""
    step = 56 if store == "f32" else 64
    return [(a, min(step, cmid - a)) for a in range(0, cmid, step)]


class RFDNeXt(HipSRModel):
    def __init__(self, in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4, block_type="RFDB", act_type="lrelu", **kwargs):
        super().__init__()
        if block_type != "RFDB" or act_type != "lrelu":
            raise NotImplementedError('HIP RFDNeXt supports block_type="RFDB" and act_type="lrelu"')
        if upscale != 4 or nf != 50 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP RFDNeXt supports upscale=4, nf=50, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = nf // 2                        # rfdn_block.py:150
        self.cm = 4 * nf                         # rfdn_block.py:138: the ConvNeXt block's hidden width
        self.DP = (self.dc + 31) // 32 * 32
        self.scale_idx = 0
        nf, dc = self.nf, self.dc
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            self._add_conv(b + 'c1_d', nf, dc, 1)
            self._add_conv(b + 'c1_r', nf, dc, 3, custom=True)            # launched as `c1_r#fold` (with c1_d on its centre tap)
            self._add_conv(b + 'c2_d', dc, dc, 1)
            self._add_conv(b + 'c2_r', dc, dc, 3)
            self._add_conv(b + 'c3_d', dc, dc, 1)
            self._add_conv(b + 'c3_r', dc, dc, 3)
            self._add_conv(b + 'c4', dc, dc, 3)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=_slice_map(4, dc, self.DP))
            self._add_leaf(b + 'esa.conv.0', torch.nn.Conv2d(nf, nf, 7, 1, 3, groups=nf))
            self._add_conv(b + 'esa.conv.1', nf, self.cm, 1, custom=True)
            self._add_conv(b + 'esa.conv.3', self.cm, nf, 1)
        self._add_conv('c.0', nf * num_modules, nf, 1, cin_map=_slice_map(num_modules, nf, _pad8(nf)))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('RFDNeXt', plan, c, self.in_nc, esa=False)
        nf, dc, cm, DP = self.nf, self.dc, self.cm, self.DP
        s16 = plan.esize == 2
        KP = plan.cpad(nf)                                # 56 fp32 channels / 64 16-bit channels: whole K chunks
        P = _pad8(nf) if (s16 and self.tight_pitch) else KP  # 16-bit storage: the nf-wide tensors at the tight pitch 56 (rfdn.py)
        HP = plan.cpad(cm)                                # the hidden tensor of the per-op ConvNeXt block: 200 fp32 / 208 16-bit channels
        skip = LongSkip(plan, self, nf, P)
        bcat = Concat(plan, 'bcat', 4, P, s16)
        cat = Concat(plan, 'cat', 4, DP, s16, _pad8(4 * DP))
        cs = cat.seg
        r1, r2, r3 = plan.buffer('r1', DP), plan.buffer('r2', DP), plan.buffer('r3', DP)
        v = plan.buffer('v', P)
        lr = None if skip.hl else plan.buffer('lr', P)
        act = dict(act=L.ACT_LRELU, slope=0.05)
        res = lambda x: dict(res=x, res_mode=L.RES_PRE_ACT)
        skip.head('fea_conv', self.in_nc)                 # (16-bit plans: allocates the packed input)
        # the per-op ConvNeXt block's t and hidden tensor: the plan's LAST allocations, so that a plan whose blocks all fused can give
        # their bytes back (Plan.release below; nothing behind this line allocates)
        t, hid = plan.buffer('t', P), plan.buffer('hid', HP)
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            plan.conv(b + 'c1_d', cur, cs(0), nf, dc, k=1, **act)         # lrelu(dc_1): what the concat holds
            plan.conv(b + 'c1_r#fold', cur, r1, nf, dc)                   # rc_1 = c1_r(x) + c1_d(x): c1_d on the centre tap
            plan.conv(b + 'c2_d', r1, cs(1), dc, dc, k=1, **act)
            plan.conv(b + 'c2_r', r1, r2, dc, dc, **res(r1))              # rc_2 = c2_r(rc_1) + rc_1, no activation
            plan.conv(b + 'c3_d', r2, cs(2), dc, dc, k=1, **act)
            plan.conv(b + 'c3_r', r2, r3, dc, dc, **res(r2), **act)
            plan.conv(b + 'c4', r3, cs(3), dc, dc, **act)                 # lrelu(rc_4)
            plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc)
            out = bcat.seg(k - 1)
            # the ConvNeXt block in its per-layer form ...
            mark = len(plan.ops)
            plan.dwconv7(b + 'esa.conv.0', v, t, nf)
            plan.conv(b + 'esa.conv.1', t, hid, nf, cm, k=1, **act)
            plan.conv(b + 'esa.conv.3', hid, out, cm, nf, k=1, **res(v))
            if not (self.fuse_cx and s16 and plan.cx_block(mark)):
                # ... launched per op: the first 1x1 as output-channel slices the existing kernels take
                pw2 = plan.ops.pop()
                del plan.ops[mark + 1:]
                for j, (a, wd) in enumerate(_hidden_slices(cm, plan.store)):
                    plan.conv(b + f'esa.conv.1#o{j}', t, hid[a:a + wd], nf, wd, k=1, **act, counted=(j == 0))
                plan.ops.append(pw2)
            cur = out
        if not any(o.kind == "dw7" for o in plan.ops):    # every block fused: nothing reads or writes t and the hidden tensor
            plan.release([t, hid])
        plan.conv('c.0', bcat.whole, v, 4 * KP, nf, k=1, cin_alg=4 * nf, **act)
        skip.close('LR_conv', 'upsampler.0', v, lr, self.out_nc * 16)

    _cin_map = block_cin_map

    def _extra_pack(self, packed, device):
        for k in range(1, 5):
            b = f'B{k}.'
            # rc_1 = c1_r(x) + c1_d(x) as one 3x3
            w, bias = fold_center(self._leaf(b + 'c1_r').weight, self._leaf(b + 'c1_r').bias, self._leaf(b + 'c1_d').weight, self._leaf(b + 'c1_d').bias)
            self._pack_own(packed, device, b + 'c1_r#fold', w, bias, wino=True)
            pw1 = self._leaf(b + 'esa.conv.1')
            for j, (a, wd) in enumerate(_hidden_slices(self.cm, self._store())):      # the per-op first 1x1: output-channel slices
                self._pack_own(packed, device, b + f'esa.conv.1#o{j}', pw1.weight[a:a + wd], pw1.bias[a:a + wd])

    def _counted_convs(self, plan, o):
        """the ConvNeXt block's first 1x1 is one nn.Conv2d of 200 outputs however many slices launch it (c5 and c.0 carry their logical
        input channels themselves: Conv.cin_alg)"""
        if o.kind == "conv" and o.w.endswith('esa.conv.1#o0'):
            return [(o.cin, self.cm, 1, plan.npix, o.act)]
        return super()._counted_convs(plan, o)
