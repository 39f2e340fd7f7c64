"""BMDN (x4) on the HIP engine -- drop-in for `models.team37_bmdn.BMDN` (team37_bmdn.py:187-221; NTIRE 2022 ESR team 37, test_demo.py
data_range 1.0).

Same constructor keywords and the same 152 state_dict keys (`fea_conv`, `B{k}.c{j}_d`, `B{k}.c{j}_r`, `B{k}.c{j}_b`, `B{k}.c4`, `B{k}.c5`,
`B{k}.esa.{conv1,conv_f,conv_max,conv2,conv3,conv3_,conv4}`, `c.0`, `LR_conv`, `upsampler.0`).  An RFDN whose refinement path is half as
wide as its trunk (BMDB, team37_bmdn.py:135-178): nf = 40, and per block three distillation steps

    d_j = relu(c_d(r_{j-1}));   r_j = relu(c_r(r_{j-1}) + c_b(d_j) [+ r_{j-1}, j >= 2])          (r_0 = the block input, 40 channels; r_j: 20)

then c4 (3x3 20 -> 20, ReLU), c5 over cat(d1, d2, d3, r4) (80 -> 40) and the baseline ESA with f = 10; c.0 over the four block outputs with
ReLU, LR_conv + fea, upsampler.0 and the pixel shuffle stored directly.  The layouts are RFDN's at nf = 40: 16-bit plans keep the nf-wide
tensors at the tight pitch 40, d1, d2, d3, r4 and the block outputs as dense tensors (engine.Planar) that c5 / c.0 read through a cin_map,
the long skip as hi + lo pairs in bf16 -- torch.cat never runs.

A distillation step has two forms (model.fuse_step):
  per-op   three launches on the existing kernels: d_j = relu(c_d(r)); t = c_b(d_j) (+ r before no activation, j >= 2); r_j = relu(c_r(r) + t).
           The only form of an fp32 plan.  16-bit plans round t to the storage type.
  fused    ONE esr_distill_step_s16 launch (distill_step_kernel; Plan.distill_step): r is read once, d_j and r_j are written once, the two
           3x3s run as one over cat[r, d_j] (engine.pack_distill_s16), t never exists.  On by default in 16-bit plans: 17 % / 34 % faster
           forwards at 32 x 256 x 256 / one 339 x 510 image in bf16.
Which form a plan takes depends on the per-image shape and esr_distill_step_supported only, never on the batch size.

The long skip (team37_bmdn.py:214), the concats and ESA's low-resolution branch are the shared frame's (frame.py).
"""
from . import _lib as L
from .engine import HipSRModel, Post
from .frame import FP, Concat, EsaBranch, LongSkip, _pad8, _slice_map, block_cin_map, check_input, set_scale


class BMDN(HipSRModel):
    def __init__(self, in_nc=3, nf=40, num_modules=4, out_nc=3, upscale=4):
        super().__init__()
        if upscale != 4 or nf > 64 or nf < 34 or nf % 2 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP BMDN supports upscale=4, even 34 <= nf <= 64, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = nf // 2                        # team37_bmdn.py:138-139: distilled = remaining = in_channels // 2
        self.f = nf // 4                         # team37_bmdn.py:109
        self.DP = (self.dc + 31) // 32 * 32      # distilled slices are whole 128-byte lines in fp32 / 64-byte lines in 16-bit storage (rfdn.py)
        self.scale_idx = 2
        nf, dc, f = self.nf, self.dc, self.f
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            for j in (1, 2, 3):
                cin = nf if j == 1 else dc
                self._add_conv(b + f'c{j}_d', cin, dc, 1)
                self._add_conv(b + f'c{j}_r', cin, dc, 3)
                self._add_conv(b + f'c{j}_b', dc, dc, 3)
            self._add_conv(b + 'c4', dc, dc, 3)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=_slice_map(4, dc, self.DP))
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_max', f, f, 3)
            self._add_conv(b + 'esa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'esa.conv3', f, f, 3)
            self._add_conv(b + 'esa.conv3_', f, f, 3)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, (nf + 3) // 4 * 4))
        self._add_conv('c.0', nf * num_modules, nf, 1, cin_map=_slice_map(num_modules, nf, _pad8(nf)))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('BMDN', plan, c, self.in_nc)
        nf, dc, f, DP = self.nf, self.dc, self.f, self.DP
        s16 = plan.esize == 2
        KP = plan.cpad(nf)                                # 40 fp32 channels / 48 16-bit channels: whole K chunks
        P = _pad8(nf) if (s16 and self.tight_pitch) else KP          # 16-bit storage: the nf-wide tensors at the tight pitch (rfdn.py)
        RP = plan.cpad(dc)                                # the 20-channel refinement tensors: 24 fp32 / 32 16-bit channels
        skip = LongSkip(plan, self, nf, P)
        # the four block outputs (team37_bmdn.py:213) and d1 d2 d3 r4 (:175): dense tensors in the 16-bit modes (engine.Planar), slices in fp32
        bcat = Concat(plan, 'bcat', 4, P, s16)
        cat = Concat(plan, 'cat', 4, DP, s16, _pad8(4 * DP))
        cs = cat.seg
        ra, rb, t = plan.buffer('ra', RP), plan.buffer('rb', RP), plan.buffer('t', RP)
        v = plan.buffer('v', P)
        lr = None if skip.hl else plan.buffer('lr', P)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        relu = dict(act=L.ACT_RELU)
        skip.head('fea_conv', self.in_nc)
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            r = cur
            for j, dst in ((1, ra), (2, rb), (3, ra)):
                cin = nf if j == 1 else dc
                mark = len(plan.ops)
                plan.conv(b + f'c{j}_d', r, cs(j - 1), cin, dc, k=1, **relu)
                if j == 1:                                # team37_bmdn.py:157-159: no `+ input` in the first step (40 -> 20 channels)
                    plan.conv(b + f'c{j}_b', cs(j - 1), t, dc, dc)
                else:                                     # :163-165 / :169-171: r_j = act(c_r(r) + r + c_b(d))
                    plan.conv(b + f'c{j}_b', cs(j - 1), t, dc, dc, res=r, res_mode=L.RES_PRE_ACT)
                plan.conv(b + f'c{j}_r', r, dst, cin, dc, res=t, res_mode=L.RES_PRE_ACT, **relu)
                if self.fuse_step and s16:
                    plan.distill_step(mark)               # (where the kernel takes the step; else the three launches stay)
                r = dst
            plan.conv(b + 'c4', r, cs(3), dc, dc, **relu)
            if s16 and (nf + 15) // 16 in (3, 4) and f <= 16:
                # 16-bit storage: esa.conv1 rides in c5's epilogue on the fp32 tile (one launch less per block)
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'esa.conv2', [(b + 'esa.conv_max', L.ACT_RELU), (b + 'esa.conv3', L.ACT_RELU), (b + 'esa.conv3_', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            out = bcat.seg(k - 1)
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f)
            cur = out
        plan.conv('c.0', bcat.whole, v, 4 * KP, nf, k=1, cin_alg=4 * nf, **relu)
        skip.close('LR_conv', 'upsampler.0', v, lr, self.out_nc * 16)

    _cin_map = block_cin_map
