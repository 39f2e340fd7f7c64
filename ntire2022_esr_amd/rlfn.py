"""RLFN_cut (x4) on the HIP engine -- drop-in for `models.team04_rlfn.RLFN_cut` (team04_rlfn.py:124-155).

Same constructor keywords and the same 78 state_dict keys (`fea_conv`, `B{k}.{c1_r,c2_r,c3_r,c5}`,
`B{k}.esa.{conv1,conv_f,conv2,conv3,conv4}`, `LR_conv`, `upsampler.0`).  nf=46 lives in NHWC buffers of
pitch 48 with two zero pad channels.  Per RLFB (team04_rlfn.py:109-122): three fused 3x3+LeakyReLU (the third
adds the block input AFTER the activation), the 1x1 c5, then ESA as 1x1 conv1 -> 3x3/s2 -> maxpool 7/3 ->
3x3 at ~H/6 -> one fused full-resolution tail (bilinear + conv_f + conv4 + sigmoid * x).  The long skip (team04_rlfn.py:149-150) and ESA's
low-resolution branch with its one 3x3 are the shared frame's (frame.py); specific to RLFN are the epilogue 1x1s and the 3x3 chain below.
"""
from . import _lib as L
from .engine import HipSRModel, Post
from .frame import FP, EsaBranch, LongSkip, check_input, set_scale


class RLFN_cut(HipSRModel):
    def __init__(self, in_nc=3, out_nc=3, nf=46, mf=48, upscale=4):
        super().__init__()
        if upscale != 4 or nf > 64 or mf > 64 or in_nc > 4 or out_nc * 16 > 64:
            raise NotImplementedError('HIP RLFN_cut supports upscale=4, nf/mf <= 64, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.mf, self.upscale = in_nc, out_nc, nf, mf, upscale
        self.esa_channels = 16
        self.scale_idx = 0
        f = self.esa_channels
        cp4 = (nf + 3) // 4 * 4
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            self._add_conv(b + 'c1_r', nf, mf, 3)
            self._add_conv(b + 'c2_r', mf, mf, 3)
            self._add_conv(b + 'c3_r', mf, nf, 3)
            self._add_conv(b + 'c5', nf, nf, 1)
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'esa.conv3', f, f, 3)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, cp4))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('RLFN_cut', plan, c, self.in_nc)
        nf, mf, f = self.nf, self.mf, self.esa_channels
        P, M = plan.cpad(nf), plan.cpad(mf)
        skip = LongSkip(plan, self, nf, P)
        xa, xb = plan.buffer('xa', P), plan.buffer('xb', P)
        t1, t2 = plan.buffer('t1', M), plan.buffer('t2', M)
        u, v = plan.buffer('u', P), plan.buffer('v', P)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        act = dict(act=L.ACT_LRELU, slope=0.05)
        skip.head('fea_conv', self.in_nc)
        cur, nxt = skip.fea, xa
        for k in range(1, 5):
            b = f'B{k}.'
            mark_c = len(plan.ops)
            plan.conv(b + 'c1_r', cur, t1, nf, mf, **act)
            plan.conv(b + 'c2_r', t1, t2, mf, mf, **act)
            if plan.esize == 2 and (nf + 15) // 16 == 3 and f <= 16:
                # 16-bit storage: c5 and esa.conv1 are evaluated in c3_r's epilogue on the fp32 tile (esr_conv_desc.post_* /
                # post2_*): u = lrelu(c3_r(..)) + x (team04_rlfn.py:117-119) is never stored, never rounded -- two launches
                # and three tensor passes less per block, and the rounding that cost RLFN bf16 most of its PSNR budget is gone
                plan.conv(b + 'c3_r', t2, None, mf, nf, res=cur, res_mode=L.RES_POST_ACT, **act,
                          post=Post(b + 'c5', v, nf, post2=Post(b + 'esa.conv1', c1, f)))
                if self.fuse_chain:
                    # ... and the three 3x3s as ONE launch where the kernel takes the shape: a layer-per-SIMD pipeline with t1 / t2 / u in LDS
                    # (esr_conv_chain_s16, round 5)
                    plan.chain(mark_c)
            else:
                plan.conv(b + 'c3_r', t2, u, mf, nf, res=cur, res_mode=L.RES_POST_ACT, **act)
                plan.conv(b + 'c5', u, v, nf, nf, k=1)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'esa.conv2', [(b + 'esa.conv3', L.ACT_NONE)], self.fuse_esa_lowres)
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, nxt, nf, f)
            cur = nxt
            nxt = xb if cur is xa else xa
        skip.close('LR_conv', 'upsampler.0', cur, u, self.out_nc * 16)
