"""Team 35's RFDN (x4) on the HIP engine -- drop-in for `models.team35_rfdn.rfdn.RFDN` (rfdn.py:11-42 + rmsrb1.py; NTIRE 2022 ESR team 35,
test_demo.py id 35, data_range 255.0).

Same constructor keywords and the same 184 state_dict keys (`fea_conv`, `B{k}.c{1,2,3}_d`, `B{k}.c{1,2,3}_r.{0,2}.{0.fn,1}`, `B{k}.c4`,
`B{k}.c5`, `B{k}.esa.{conv1,conv_f,conv_max,con_,conv4}`, `c.0`, `LR_conv`, `upsampler.0`).  RFDN's frame at nf = 50 / dc = 25 with
LeakyReLU(0.05), ReLU and sigmoid only (rmsrb1.py:199-217); two things differ from the baseline.

The refinement path: each c{j}_r is `conv_four_layer(50)` (rmsrb1.py:22-27) instead of a dense 3x3, followed by the block's act(. + x):

    u1 = dw3_a(x) + x              Residual(depthwise 3x3, zero padding, bias)        c{j}_r.0.0.fn
    h  = relu(Wa . u1 + ba)        1x1, 50 -> 50                                      c{j}_r.0.1
    u2 = dw3_b(h) + h                                                                 c{j}_r.2.0.fn
    r  = lrelu(Wb . u2 + bb + x)   1x1, 50 -> 50, the block input added               c{j}_r.2.1

It has two forms (model.fuse_pair):
  per-op   esr_dwconv3x3_f32 with its input as the pre-activation residual -> 1x1 + relu -> the same again -> 1x1 with x as the residual
           + lrelu: four launches, nine tensor passes, 1008 bytes per pixel in bf16 at pitch 56.  The only form of an fp32 plan.
  fused    ONE esr_dwpw_pair_s16 launch (dwpw_pair_kernel; Plan.dwpw_pair): x is read once, r written once: 224 bytes per pixel.  Within one
           rounding per stage of the per-op form, not bit-identical to it (its 1x1 weights are rounded once).  Measured: DESIGN.md 7h.
Which form a plan takes depends on the per-image shape and esr_dwpw_pair_supported only, never on the batch size.

ESA's low-resolution branch (rmsrb1.py:137-150): c3 = relu(con_(relu(max_pool2d(pixel_unshuffle(conv1(x), 2), 7, 3)))) with con_ a 1x1
48 -> 12 built with padding=1 -- its output is two pixels larger each way than the pooled map, the ring equals relu(bias) -- as ONE launch
(esr_esa_unshuffle_f32; Plan.esa_unshuffle), then the usual tail x * sigmoid(conv4(bilinear(c3) + conv_f(conv1(x)))) (Plan.esa_apply).
`esa.conv_max` is in the checkpoint and is loaded and counted as parameters, but the forward never calls it: it is never launched.
pixel_unshuffle is a strided convolution there, so an odd H or W is floored; H, W >= 14 (one pooling window), the reference fails below.

The layouts are rfdn.py's at nf = 50: nf-wide tensors at pitch 56 (16-bit plans, tight pitch) or whole K chunks, the 25-channel maps in
32-wide tensors, the concat as four dense 32-wide segments (engine.Planar; one 128-wide buffer in fp32) read by c5 through `_slice_map`,
the block outputs as four 56-wide tensors read by c.0, the long skip as a hi + lo pair in bf16 -- torch.cat never runs.  The long skip
(rfdn.py:38) and the two concats are the shared frame's (frame.py).
"""
from . import _lib as L
from .engine import HipSRModel, Post
from .frame import FP, Concat, LongSkip, _pad8, _slice_map, block_cin_map, check_input, set_scale


def _unshuffle_hw(h, w):
    """size of con_'s output: pixel_unshuffle(2) floors, max_pool2d(7, stride 3), then the 1x1 with padding 1"""
    return (h // 2 - 7) // 3 + 3, (w // 2 - 7) // 3 + 3


class DWRFDN(HipSRModel):
    def __init__(self, in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4):
        super().__init__()
        if upscale != 4 or nf != 50 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP DWRFDN supports upscale=4, nf=50, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = nf // 2                        # rmsrb1.py:184
        self.f = nf // 4                         # rmsrb1.py:126
        self.DP = (self.dc + 31) // 32 * 32
        self.scale_idx = 0
        nf, dc, f = self.nf, self.dc, self.f
        cp4 = (nf + 3) // 4 * 4
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            for j in (1, 2, 3):
                self._add_conv(b + f'c{j}_d', nf, dc, 1)
                for half in (0, 2):              # conv_four_layer: Sequential(conv_two_layer, ReLU, conv_two_layer)
                    self._add_dw(b + f'c{j}_r.{half}.0.fn', nf)
                    self._add_conv(b + f'c{j}_r.{half}.1', nf, nf, 1)
            self._add_conv(b + 'c4', nf, dc, 3)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=_slice_map(4, dc, self.DP))
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_max', f, f, 3)                               # never launched (rmsrb1.py:137-150 does not call it)
            self._add_conv(b + 'esa.con_', 4 * f, f, 1, padding=1, custom=True)       # packed for Plan.esa_unshuffle (pack_unshuffle)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, cp4))
        self._add_conv('c.0', nf * num_modules, nf, 1, cin_map=_slice_map(num_modules, nf, _pad8(nf)))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('DWRFDN', plan, c, self.in_nc, esa=False)
        if plan.h < 14 or plan.w < 14:
            raise L.EsrError('ESA needs H, W >= 14 (pixel_unshuffle(2), then 7x7/s3 pooling of the half-resolution map)')
        nf, dc, f, DP = self.nf, self.dc, self.f, self.DP
        s16 = plan.esize == 2
        KP = plan.cpad(nf)                                # 56 fp32 channels / 64 16-bit channels: whole K chunks
        P = _pad8(nf) if (s16 and self.tight_pitch) else KP  # 16-bit storage: the nf-wide tensors at the tight pitch 56 (rfdn.py)
        skip = LongSkip(plan, self, nf, P)
        bcat = Concat(plan, 'bcat', 4, P, s16)
        cat = Concat(plan, 'cat', 4, DP, s16, _pad8(4 * DP))
        cs = cat.seg
        r1, r2 = plan.buffer('r1', P), plan.buffer('r2', P)
        v = plan.buffer('v', P)
        c1 = plan.buffer('esa_c1', FP)
        c3 = plan.buffer('esa_c3', FP, *_unshuffle_hw(plan.h, plan.w))
        act = dict(act=L.ACT_LRELU, slope=0.05)
        res = lambda x: dict(res=x, res_mode=L.RES_PRE_ACT)
        skip.head('fea_conv', self.in_nc)                 # (16-bit plans: allocates the packed input)
        # u1 / u2 and h of the per-op refinement path: the plan's LAST allocations, so that a plan whose paths all fused can give their
        # bytes back (Plan.release below; nothing behind this line allocates)
        t1, t2 = plan.buffer('t1', P), plan.buffer('t2', P)

        def refine(path, x, dst):
            """dst = lrelu(conv_four_layer(x) + x): rmsrb1.py:201-202"""
            mark = len(plan.ops)
            plan.dwconv(path + '.0.0.fn', x, t1, nf, **res(x))
            plan.conv(path + '.0.1', t1, t2, nf, nf, k=1, act=L.ACT_RELU)
            plan.dwconv(path + '.2.0.fn', t2, t1, nf, **res(t2))
            plan.conv(path + '.2.1', t1, dst, nf, nf, k=1, **res(x), **act)
            if self.fuse_pair and s16:
                plan.dwpw_pair(mark)

        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            plan.conv(b + 'c1_d', cur, cs(0), nf, dc, k=1, **act)
            refine(b + 'c1_r', cur, r1)
            plan.conv(b + 'c2_d', r1, cs(1), nf, dc, k=1, **act)
            refine(b + 'c2_r', r1, r2)
            plan.conv(b + 'c3_d', r2, cs(2), nf, dc, k=1, **act)
            refine(b + 'c3_r', r2, r1)
            plan.conv(b + 'c4', r1, cs(3), nf, dc, **act)
            if s16 and (nf + 15) // 16 in (3, 4) and f <= 16:
                # 16-bit storage: esa.conv1 rides in c5's epilogue on the fp32 tile (one launch less per block; rfdn.py)
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            plan.esa_unshuffle(b + 'esa.con_', c1, c3, f)
            out = bcat.seg(k - 1)
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f)
            cur = out
        if not any(o.kind == "dw" for o in plan.ops):     # every path fused: nothing reads or writes t1 and t2
            plan.release([t1, t2])
        plan.conv('c.0', bcat.whole, v, 4 * KP, nf, k=1, cin_alg=4 * nf, **act)
        skip.close('LR_conv', 'upsampler.0', v, r1, self.out_nc * 16)

    _cin_map = block_cin_map

    def _counted_convs(self, plan, o):
        """the depthwise layers are nn.Conv2d calls of their own here (Dw counts nothing by itself: BSRN's ride in its BSConvU counts); an
        esa.conv1 riding in c5's epilogue is counted with it (Conv.counted_convs: the post 1x1)"""
        if o.kind == "dw":
            return o.dw_counted(plan)
        return super()._counted_convs(plan, o)

    def _complexity_terms(self, plan, o):
        """+ the nn.ReLU call on the pooled map in front of con_ (rmsrb1.py:142), which no convolution's count carries"""
        flops, acts, nconv = super()._complexity_terms(plan, o)
        if o.kind == "unshuffle":
            flops += o.relu_elements(plan)
        return flops, acts, nconv
