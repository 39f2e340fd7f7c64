"""EFDN (x4) on the HIP engine -- drop-in for `models.team05_efdn.plainsr.PLAINRFDN` (plainsr.py:5-38; NTIRE 2022 ESR team 05, third in the
runtime track; test_demo.py:59-65, data_range 255).

Same constructor keywords and the same 118 state_dict keys (`fea_conv`, `B{k}.c{j}_d`, `B{k}.c{j}_r.conv3x3`, `B{k}.c4.conv3x3`, `B{k}.c5`,
`B{k}.esa.{conv1,conv_f,conv_2,conv_3,conv_23,conv4}`, `LR_conv`, `upsampler.0`).  An RFDN without its residuals (plainblock.py:152-194):
dc = 10 in every block, no `+ input` in the RFDB, no 1x1 over the four block outputs -- out_lr = LR_conv(B4) + fea (plainsr.py:23-34) -- and
an ESA whose low-resolution branch pools the conv1 map directly, max_pool2d(7, stride 7, padding 1), then runs two parallel 3x3s and a 3x3
over their concat (plainblock.py:124-150; Plan.maxpool7s7, or one esr_esa_lowres_f32 op with w_s2 = NULL).  nf = 42 lives in NHWC buffers
of pitch 48 (whole K chunks in every storage type, so the tight pitch is the same); d1, d2, d3 and r4 are 16-wide slices (16-bit: four dense
tensors, engine.Planar) that c5 reads through a cin_map -- torch.cat never runs.  The long skip (plainsr.py:30) and the concat are the shared
frame's (frame.py); the stride-7 ESA branch and its maps are this file's.
"""
from . import _lib as L
from .engine import EsaLayer, HipSRModel, Post
from .frame import FP, Concat, LongSkip, _pool7, _slice_map, check_input, set_scale


class PLAINRFDN(HipSRModel):
    def __init__(self, in_nc=3, nf=42, num_modules=4, out_nc=3, upscale=4):
        super().__init__()
        if upscale != 4 or nf > 64 or nf < 33 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP PLAINRFDN supports upscale=4, 33 <= nf <= 64, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = 10                             # plainblock.py:155: fixed, not a rate of nf
        self.f = nf // 4                         # plainblock.py:127
        self.DP = 16                             # one 16-wide slice per distilled map (d1, d2, d3, r4)
        self.scale_idx = 0
        nf, dc, f = self.nf, self.dc, self.f
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            for j in (1, 2, 3):
                self._add_conv(b + f'c{j}_d', nf, dc, 1)
                self._add_conv(b + f'c{j}_r.conv3x3', nf, nf, 3)
            self._add_conv(b + 'c4.conv3x3', nf, dc, 3)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=_slice_map(4, dc, self.DP))
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_2', f, f, 3)
            self._add_conv(b + 'esa.conv_3', f, f, 3)
            # conv_23 reads the pair's [.., 32] map: conv_2's f channels from slot 0, conv_3's from slot 16
            self._add_conv(b + 'esa.conv_23', 2 * f, f, 3, cin_map=_slice_map(2, f, FP))
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, (nf + 3) // 4 * 4))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('PLAINRFDN', plan, c, self.in_nc, esa=False)
        if plan.h < 5 or plan.w < 8:
            # the pooling needs H, W >= 5; esr_esa_apply_f32's kernels carry a 16-pixel group's column over at most two image rows, which
            # holds for W >= 8 (RFDN, RLFN and BSRN never go below W = 15)
            raise L.EsrError('PLAINRFDN needs H >= 5 and W >= 8 (max_pool2d(7, stride 7, padding 1); the ESA apply kernels)')
        nf, dc, f, DP = self.nf, self.dc, self.f, self.DP
        P = plan.cpad(nf)                                 # 48 in every storage type
        h7, w7 = _pool7(plan.h, plan.w)
        # 16-bit plans: 1x1s in another launch's epilogue where a kernel takes dc = f = 10 -- esa.conv1 behind c5 (esr_conv_post_supported) and the
        # next block's c1_d in the ESA apply (esr_esa_apply_post_supported).  c2_d / c3_d behind c1_r / c2_r and block 1's c1_d behind the head are
        # refused by esr_conv_post_supported for a 42-channel 3x3 with a 10-channel post (the fp32 post kernels need 48 < cout): separate 1x1s
        s16 = plan.esize == 2
        apply_d = s16 and bool(L.lib().esr_esa_apply_post_supported(nf, dc, 0))
        skip = LongSkip(plan, self, nf, P)
        cat = Concat(plan, 'cat', 4, DP, s16)
        cs = cat.seg
        r1, r2, v = plan.buffer('r1', P), plan.buffer('r2', P), plan.buffer('v', P)
        bo = [plan.buffer('bo0', P), plan.buffer('bo1', P)]
        c1 = plan.buffer('esa_c1', FP)
        pooled = plan.buffer('esa_p', FP, h7, w7)
        pair = plan.buffer('esa_pair', 2 * FP, h7, w7)
        c3 = plan.buffer('esa_c3', FP, h7, w7)
        act = dict(act=L.ACT_LRELU, slope=0.05)
        lo = dict(hw=(h7, w7))
        skip.head('fea_conv', self.in_nc)
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            if not (apply_d and k > 1):
                plan.conv(b + 'c1_d', cur, cs(0), nf, dc, k=1, **act)
            plan.conv(b + 'c1_r.conv3x3', cur, r1, nf, nf, **act)
            plan.conv(b + 'c2_d', r1, cs(1), nf, dc, k=1, **act)
            plan.conv(b + 'c2_r.conv3x3', r1, r2, nf, nf, **act)
            plan.conv(b + 'c3_d', r2, cs(2), nf, dc, k=1, **act)
            plan.conv(b + 'c3_r.conv3x3', r2, r1, nf, nf, **act)
            plan.conv(b + 'c4.conv3x3', r1, cs(3), nf, dc, **act)
            if s16:
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            # ESA's low-resolution branch (plainblock.py:143-147): pooling, the pair into the two 16-wide slices of one map, conv_23 over it
            mark = len(plan.ops)
            plan.maxpool7s7(c1, pooled)
            plan.conv(b + 'esa.conv_2', pooled, pair[0:f], f, f, act=L.ACT_RELU, **lo)
            plan.conv(b + 'esa.conv_3', pooled, pair[FP:FP + f], f, f, act=L.ACT_RELU, **lo)
            plan.conv(b + 'esa.conv_23', pair, c3, 2 * FP, f, cin_alg=2 * f, **lo)
            if self.fuse_esa_lowres:
                # the four launches above as one op of two (halo recompute; only the pooled map reaches memory)
                plan.esa_lowres(mark, c1, pooled, c3, f, None, [EsaLayer(2, L.ACT_RELU, b + 'esa.conv_2', b + 'esa.conv_3'),
                                                                 EsaLayer(3, L.ACT_NONE, b + 'esa.conv_23')])
            out = bo[(k - 1) % 2]
            nxt_d = [Post(f'B{k + 1}.c1_d', cs(0), dc, L.ACT_LRELU, slope=0.05)] if (apply_d and k < 4) else None
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f, post=nxt_d)
            cur = out
        skip.close('LR_conv', 'upsampler.0', cur, r1, self.out_nc * 16)
