"""FasterRFDN (x4) on the HIP engine -- drop-in for `models.team25_frfdn.FRFDN.FasterRFDN` (FRFDN.py:17-50; NTIRE 2022 ESR team 25,
test_demo.py data_range 1.0).

Same constructor keywords and the same 128 state_dict keys (`fea_conv`, `B{k}.c1_d`, `B{k}.c{1,2,3}_r`, `B{k}.c{2,3}_d`, `B{k}.c4`, `B{k}.c5`,
`B{k}.esa.{conv1,conv_f,conv_max,conv2,conv3,conv3_,conv4}`, `c.0`, `LR_conv`, `upsampler.0`).  An RFDN at nf = 64 whose refinement path
narrows (FRFDB, team25_frfdn/block.py:92-127), every activation LeakyReLU(0.05):

    d1 = lrelu(c1_d . x)             1x1 64 -> 32          r1 = lrelu(c1_r (*) x + x)       3x3 64 -> 64
    d2 = lrelu(c2_d . r1)            1x1 64 -> 32          r2 = lrelu(c2_r (*) d2 + d2)     3x3 32 -> 32
    d3 = lrelu(c3_d . r2)            1x1 32 -> 16          r3 = lrelu(c3_r (*) d3 + d3)     3x3 16 -> 16
                                                           r4 = lrelu(c4   (*) r3 + r3)     3x3 16 -> 16

then c5 over cat(d1, d2, d3, r4) (32 + 32 + 16 + 16 = 96 -> 64) and the baseline ESA with f = 16; c.0 over the four block outputs with
LeakyReLU, LR_conv + fea, upsampler.0 and the pixel shuffle stored directly.  The layouts are RFDN's at nf = 64, where nothing is padded:
the concat is three dense 32-channel segments d1 | d2 | [d3, r4] (engine.Planar in 16-bit plans, a 96-wide buffer in fp32) that c5 reads
through an identity map, the block outputs are four dense 64-channel tensors read by c.0, the long skip is a hi + lo pair in bf16 --
torch.cat never runs.  In 16-bit plans c1_d rides in the launch that produces the block's input (the head, the previous block's ESA
apply), c2_d in c1_r's epilogue and esa.conv1 in c5's; an fp32 plan launches each of them on its own.

The refinement path behind d2 has two forms (model.fuse_cascade):
  per-op   four launches on the existing kernels: c2_r, c3_d, c3_r, c4; d3 and r4 are written as 16-channel slices of the third concat segment.
           The only form of an fp32 plan.
  fused    ONE esr_refine_cascade_s16 launch (refine_cascade_kernel; Plan.refine_cascade): d2 is read once, d3 and r4 are written once, r2 and
           r3 stay in LDS.  Bit-identical to the per-op form.  OFF by default: in bf16 it is 14 % faster on one 339 x 510 image (0.659 against
           0.764 ms per forward) but not at 32 x 256 x 256 (4.486 against 4.476 ms, inside the spread between repeats); DESIGN.md 7f.
Which form a plan takes depends on the per-image shape and esr_refine_cascade_supported only, never on the batch size.

The long skip (FRFDN.py:46), the concats and ESA's low-resolution branch are the shared frame's (frame.py); d3 and r4, two halves of one concat
segment, are this file's.
"""
from . import _lib as L
from .engine import HipSRModel, Post
from .frame import FP, Concat, EsaBranch, LongSkip, check_input, set_scale


class FasterRFDN(HipSRModel):
    def __init__(self, in_nc=3, nf=64, num_modules=4, out_nc=3, upscale=4):
        super().__init__()
        if upscale != 4 or nf != 64 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP FasterRFDN supports upscale=4, nf=64, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = nf // 2                        # block.py:95: distilled channels
        self.qc = nf // 4                        # block.py:101-103: the width of d3, r3, r4
        self.f = nf // 4                         # block.py:66
        self.scale_idx = 0
        nf, dc, qc, f = self.nf, self.dc, self.qc, self.f
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            self._add_conv(b + 'c1_d', nf, dc, 1)
            self._add_conv(b + 'c1_r', nf, nf, 3)
            self._add_conv(b + 'c2_d', nf, dc, 1)
            self._add_conv(b + 'c2_r', dc, dc, 3)
            self._add_conv(b + 'c3_d', dc, qc, 1)
            self._add_conv(b + 'c3_r', qc, qc, 3)
            self._add_conv(b + 'c4', qc, qc, 3)
            self._add_conv(b + 'c5', 2 * dc + 2 * qc, nf, 1)
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_max', f, f, 3)
            self._add_conv(b + 'esa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'esa.conv3', f, f, 3)
            self._add_conv(b + 'esa.conv3_', f, f, 3)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, nf))
        self._add_conv('c.0', nf * num_modules, nf, 1)
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('FasterRFDN', plan, c, self.in_nc)
        nf, dc, qc, f = self.nf, self.dc, self.qc, self.f
        s16 = plan.esize == 2
        CW = 2 * dc + 2 * qc                              # the concat: 96 channels, no pad slot in any storage
        skip = LongSkip(plan, self, nf, nf)
        # the four block outputs (FRFDN.py:45) and d1 | d2 | [d3, r4] (block.py:124): dense tensors in the 16-bit modes (engine.Planar), slices in fp32
        bcat = Concat(plan, 'bcat', 4, nf, s16)
        cat = Concat(plan, 'cat', 3, dc, s16, CW)
        d1, d2 = cat.seg(0), cat.seg(1)
        d3 = (cat.seg(2), 0, qc) if s16 else cat.whole[2 * dc:2 * dc + qc]
        r4 = (cat.seg(2), qc, qc) if s16 else cat.whole[2 * dc + qc:CW]
        r1, r2, r3 = plan.buffer('r1', nf), plan.buffer('r2', dc), plan.buffer('r3', qc)
        v = plan.buffer('v', nf)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        act = dict(act=L.ACT_LRELU, slope=0.05)
        res = lambda t: dict(res=t, res_mode=L.RES_PRE_ACT)
        # 16-bit modes: block 1's c1_d (of fea) rides in the head convolution's epilogue, the other blocks' in the ESA apply launch that
        # produces their input (esr_esa_desc.post[])
        apply_d = s16 and bool(L.lib().esr_esa_apply_post_supported(nf, dc, 0))
        skip.head('fea_conv', self.in_nc, post=Post('B1.c1_d', d1, dc, L.ACT_LRELU) if s16 else None)
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            if not (s16 and (k == 1 or apply_d)):
                plan.conv(b + 'c1_d', cur, d1, nf, dc, k=1, **act)
            if s16:
                # c2_d, the distillation conv of r1, rides in the epilogue of the conv that produces r1 (block.py:111-114)
                plan.conv(b + 'c1_r', cur, r1, nf, nf, **res(cur), **act, post=Post(b + 'c2_d', d2, dc, L.ACT_LRELU))
            else:
                # fp32: a launch of its own.  conv_f32_kernel evaluates a post 1x1 in its epilogue only from 256 tiles of 16 x 32 and as a
                # second launch below that, in another summation order: one 256 x 256 image and the same image in a batch of two would differ
                plan.conv(b + 'c1_r', cur, r1, nf, nf, **res(cur), **act)
                plan.conv(b + 'c2_d', r1, d2, nf, dc, k=1, **act)
            mark = len(plan.ops)
            plan.conv(b + 'c2_r', d2, r2, dc, dc, **res(d2), **act)
            plan.conv(b + 'c3_d', r2, d3, dc, qc, k=1, **act)
            plan.conv(b + 'c3_r', d3, r3, qc, qc, **res(d3), **act)
            plan.conv(b + 'c4', r3, r4, qc, qc, **res(r3), **act)
            if self.fuse_cascade and s16:
                plan.refine_cascade(mark)                 # (where the kernel takes the path; else the four launches stay)
            if s16:
                # 16-bit storage: esa.conv1 rides in c5's epilogue on the fp32 tile (one launch less per block)
                plan.conv(b + 'c5', cat.whole, v, CW, nf, k=1, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c5', cat.whole, v, CW, nf, k=1)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'esa.conv2', [(b + 'esa.conv_max', L.ACT_RELU), (b + 'esa.conv3', L.ACT_RELU), (b + 'esa.conv3_', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            out = bcat.seg(k - 1)
            nxt_d = [Post(f'B{k + 1}.c1_d', d1, dc, L.ACT_LRELU, slope=0.05)] if (apply_d and k < 4) else None
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f, post=nxt_d)
            cur = out
        plan.conv('c.0', bcat.whole, v, 4 * nf, nf, k=1, **act)
        skip.close('LR_conv', 'upsampler.0', v, r1, self.out_nc * 16)
