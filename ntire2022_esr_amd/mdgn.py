"""MDGN (x4) on the HIP engine -- drop-in for `models.team24_mdgn.MDGN` (team24_mdgn.py:31-51; NTIRE 2022 ESR team 24, test_demo.py id 24,
data_range 255.0).

Same constructor keywords and the same 62 state_dict keys (`fea_conv`, `B.{k}.{f1,f2,f3,conv_fuse}.{0, 1 (nn.PReLU)}`, `B.{k}.sa.0`, `LR_conv`,
`upsampler.0`), 560 244 parameters.  nf = 64: whole K chunks in every storage, no pitch is padded.  No ESA and no low-resolution branch --
everything runs at full resolution on 64 channels, so there is no minimum input size: a 1 x 1 image is a valid forward.

    fea = fea_conv(x)                                            3 -> 64, 3x3
    MDSA x num_modules (team24_mdgn.py:5-28) on the running x:
        f1 = prelu(f1.0 (*) x, a1);  f2 = prelu(f2.0 (*) f1, a2);  f3 = prelu(f3.0 (*) f2, a3)        3x3, 64 -> 64, the PReLU BEHIND it
        f  = prelu(conv_fuse.0 . cat(f1, f2, f3), a_f)           1x1, 192 -> 64
        s  = sigmoid(sa.0 . x)                                   1x1, 64 -> 1
        x' = f * s                                               s broadcast over the channels
    out_lr = LR_conv(x) + fea;  PixelShuffle(4)(upsampler.0(out_lr))                               the shared frame's long skip (frame.py)

Every nn.PReLU has one slope per channel (the checkpoint's 1 024 span -0.88 .. +0.98; esr_prelu implements v >= 0 ? v : a v for any slope).
A block is nine launches on the existing kernels, in every storage:
    raw = f{j}.0 (*) src;  f{j} = prelu(raw)       the convolution (Winograd in fp32 plans where esr_wino_supported), then esr_prelu into the
                                                   concat's segment -- cat(f1, f2, f3) never runs (frame.Concat: three dense tensors in a
                                                   16-bit plan, slices of one 192-wide buffer in fp32)                              (x 3)
    raw = conv_fuse.0 . cat;  t = prelu(raw)
    x'  = sigmoid(W_s . x) * t                     FMEN's gate epilogue (L.RES_GATE) on a 64 x 64 1x1 whose rows are ALL w_s (`sa.0#rep`): every
                                                   output channel computes the same dot product in the same order, so every channel sees the
                                                   same s.  The counters report it as the reference's 64 -> 1 convolution.
x' goes to the other tensor of a ping-pong pair: an output never lands in the tensor a 3x3 reads as halo.
  fused (16-bit plans; two independent flags, csrc/esr_mdsa.hip)
    model.fuse_conv_prelu   each conv + prelu pair as ONE esr_conv_prelu launch (Plan.conv_prelu, conv_prelu_kernel): the activation on the
                            fp32 accumulators, raw never stored: 256 instead of 512 bytes per pixel and pair
    model.fuse_mdsa_gate    the last three ops as ONE esr_mdsa_gate launch (Plan.mdsa_gate, mdsa_gate_kernel): f1, f2, f3 and x read once, x'
                            written once: 640 instead of 1 152 bytes per pixel
  Both on: four ops per block.  Which form a plan takes depends on the flag and the esr_*_supported predicate only, never on the batch
  size.  Measurements and which flag ships on: DESIGN.md 7m.
A 16-bit plan rounds each tensor it stores once (per layer: raw, f{j}, t and x'; fused: f{j} and x') where the reference's graph keeps fp32;
tools/gen_golden_mdgn.py emulates exactly those roundings on the reference (tests/golden/emul_team24_mdgn.json), which is where the 16-bit
tests take their bound from.

fp16 storage: the reference's largest activation is 4 239 on tests/golden/test.bmp (B.0.f2.0) and 3.2e4 on uniform noise, both below 65 504.
"""
import torch
import torch.nn as nn

from . import _lib as L
from .engine import HipSRModel
from .frame import Concat, LongSkip, check_input

REP = "#rep"               # sa.0 as a 64 x 64 1x1 whose rows are all w_s, biases all b_s (the gate of L.RES_GATE)


class MDGN(HipSRModel):
    def __init__(self, in_nc=3, nf=64, num_modules=4, out_nc=3, upscale=4):
        super().__init__()
        if in_nc != 3 or nf != 64 or out_nc != 3 or upscale != 4 or num_modules < 1:
            raise NotImplementedError('HIP MDGN supports in_nc=3, nf=64, out_nc=3, upscale=4, num_modules >= 1: the kernels behind an MDSA '
                                      'block take 64 channels, the head and the pixel-shuffle store 3 colours at x4')
        self.in_nc, self.out_nc, self.nf, self.upscale, self.num_modules = in_nc, out_nc, nf, upscale, num_modules
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(num_modules):
            b = f'B.{k}.'
            for j in (1, 2, 3):
                self._add_conv(b + f'f{j}.0', nf, nf, 3)
                self._add_leaf(b + f'f{j}.1', nn.PReLU(nf))
            self._add_conv(b + 'conv_fuse.0', 3 * nf, nf, 1)
            self._add_leaf(b + 'conv_fuse.1', nn.PReLU(nf))
            self._add_conv(b + 'sa.0', nf, 1, 1, custom=True)      # packed by _extra_pack, replicated
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    def _build_plan(self, plan, c):
        check_input('MDGN', plan, c, self.in_nc, esa=False)
        nf = self.nf
        s16 = plan.esize == 2
        skip = LongSkip(plan, self, nf, nf)
        cat = Concat(plan, 'cat', 3, nf, planar=s16)             # cat(f1, f2, f3), team24_mdgn.py:26
        raw, t = plan.buffer('raw', nf), plan.buffer('t', nf)
        xa, xb = plan.buffer('xa', nf), plan.buffer('xb', nf)    # the blocks' outputs: x' is never stored over the x its block reads
        skip.head('fea_conv', self.in_nc)
        x = skip.fea
        for k in range(self.num_modules):
            b = f'B.{k}.'
            src = x
            for j in (1, 2, 3):
                mark = len(plan.ops)
                plan.conv(b + f'f{j}.0', src, raw, nf, nf)
                plan.prelu(b + f'f{j}.1', [(raw, nf)], cat.seg(j - 1))
                if s16 and self.fuse_conv_prelu:
                    plan.conv_prelu(mark)                  # (where the kernel takes the pair; else the two launches stay)
                src = cat.seg(j - 1)
            mark = len(plan.ops)
            plan.conv(b + 'conv_fuse.0', cat.whole, raw, 3 * nf, nf, k=1)
            plan.prelu(b + 'conv_fuse.1', [(raw, nf)], t)
            out = xb if x is xa else xa
            plan.conv(b + 'sa.0' + REP, x, out, nf, nf, k=1, res=t, res_mode=L.RES_GATE)      # f * sigmoid(sa.0 . x)
            if s16 and self.fuse_mdsa_gate:
                plan.mdsa_gate(mark, sa=b + 'sa.0')
            x = out
        skip.close('LR_conv', 'upsampler.0', x, raw, self.out_nc * 16)

    def _extra_pack(self, packed, device):
        cpu = lambda p: p.detach().to("cpu", torch.float32)
        nf = self.nf
        for k in range(self.num_modules):
            leaf = self._leaf(f'B.{k}.sa.0')
            w, bias = cpu(leaf.weight).expand(nf, nf, 1, 1).contiguous(), cpu(leaf.bias).expand(nf).contiguous()
            self._pack_own(packed, device, f'B.{k}.sa.0' + REP, w, bias)

    def _counted_convs(self, plan, o):
        """the replicated gate is the reference's sa.0: nn.Conv2d(64, 1, 1); its nn.Sigmoid and the product have no hook in the counters"""
        if o.kind == "conv" and o.w.endswith(REP):
            return [(self.nf, 1, 1, plan.npix, L.ACT_NONE)]
        return super()._counted_convs(plan, o)

    def _complexity_terms(self, plan, o):
        if o.kind in ("convprelu", "mdsagate"):
            terms = [self._complexity_terms(plan, q) for q in o.replaces]
            return tuple(sum(t[i] for t in terms) for i in range(3))
        if o.kind == "prelu":                            # one flop per element of an nn.PReLU's output, like the ReLU family
            return o.prelu_elements(plan), 0, 0
        return super()._complexity_terms(plan, o)
