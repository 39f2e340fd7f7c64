"""RFDN (x4) on the HIP engine -- drop-in for `models.rfdn_baseline.RFDN.RFDN` (RFDN.py:11-41; ids 0, 6, 22).

Same constructor keywords and the same 128 state_dict keys.  nf=50 lives in NHWC buffers of pitch 56 (six
zero pad channels); the 25-channel distilled maps are stored as 32-wide (one 128-byte line) slices of one 128-wide concat buffer
and the four block outputs as 56-wide slices of one 224-wide buffer, so neither torch.cat
(rfdn_baseline/block.py:163, RFDN.py:36) exists as a kernel: the following 1x1 convs are packed with a
`cin_map` that skips the pad slots.  Per RFDB (block.py:148-166): {1x1 distil + LeakyReLU, 3x3 + input
residual + LeakyReLU} x3, 3x3 50->25 + LeakyReLU, 1x1 c5 over the concat, ESA.  The long skip (RFDN.py:44-47), the two concats and ESA's
low-resolution branch are the shared frame's (frame.py); specific to RFDN is which 1x1 rides in which launch, and the fused block tail.
"""
from . import _lib as L
from .engine import HipSRModel, Planar, Post, Tail
from .frame import FP, Concat, EsaBranch, LongSkip, _pad8, _slice_map, block_cin_map, check_input, identity_conv_f, set_scale


class RFDN(HipSRModel):
    def __init__(self, in_nc=3, nf=50, num_modules=4, out_nc=3, upscale=4, block_residual=True, esa_f=None,
                 esa_conv_f=True):
        """The last three keywords are not in the reference's constructor; they select its two RFDN derivatives
        (SURVEY 8f N2): `models.team40_rfdn_pruned.RFDN` = RFDN(nf=40, block_residual=False, esa_f=12)
        (team40_rfdn_pruned.py:148-166 has no `+ input` in the refinement convs, :106 fixes the ESA width at 50 // 4) and
        `models.team08_sfdn.RFDN` = RFDN(block_residual=False, esa_conv_f=False) (team08_sfdn.py:137-147; its ESA adds
        conv1's output itself where the baseline adds conv_f of it, :118-129; the checkpoint is re-parameterised)."""
        super().__init__()
        if upscale != 4 or nf > 64 or in_nc > 4 or out_nc * 16 > 64 or num_modules != 4:
            raise NotImplementedError('HIP RFDN supports upscale=4, nf <= 64, 4 modules, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.num_modules, self.upscale = in_nc, out_nc, nf, num_modules, upscale
        self.dc = nf // 2
        self.f = nf // 4 if esa_f is None else esa_f
        self.block_residual, self.esa_conv_f = block_residual, esa_conv_f
        self.scale_idx = 0
        nf, dc, f = self.nf, self.dc, self.f
        # distilled slices are padded to whole 128-byte lines: a 1x1 writing a 112-byte slice of every 448 bytes costs
        # 17 % more time than one writing 128 of every 512 (partial-line writes), the wider c5 read costs 5 %
        self.DP = (dc + 31) // 32 * 32
        cp4 = (nf + 3) // 4 * 4
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            for j in (1, 2, 3):
                self._add_conv(b + f'c{j}_d', nf, dc, 1)
                self._add_conv(b + f'c{j}_r', nf, nf, 3)
            self._add_conv(b + 'c4', nf, dc, 3)
            self._add_conv(b + 'c5', dc * 4, nf, 1, cin_map=_slice_map(4, dc, self.DP))
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            if esa_conv_f:
                self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_max', f, f, 3)
            self._add_conv(b + 'esa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'esa.conv3', f, f, 3)
            self._add_conv(b + 'esa.conv3_', f, f, 3)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, cp4))
        self._add_conv('c.0', nf * num_modules, nf, 1, cin_map=_slice_map(num_modules, nf, _pad8(nf)))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('RFDN', plan, c, self.in_nc)
        nf, dc, f, DP = self.nf, self.dc, self.f, self.DP
        KP = plan.cpad(nf)                                # 56 fp32 channels / 64 16-bit channels: whole K chunks
        # 16-bit storage, round 6: the nf-wide tensors at a TIGHT pitch -- round_up(nf, 8) = 56 channels (112-byte pixels) instead of 64; a consumer's
        # last K chunk runs 8 channels into the next pixel against zero weight rows (esr_conv2d_s16).  12.5 % fewer bytes per launch of an
        # HBM-bound model
        P = _pad8(nf) if (plan.esize == 2 and self.tight_pitch) else KP
        skip = LongSkip(plan, self, nf, P)
        # the four block outputs, RFDN.py:36: four dense tensors in the 16-bit modes (engine.Planar; same slot order as the padded
        # [.., 4 P] buffer, so c.0's weight blob does not change)
        planar = plan.esize == 2
        bcat = Concat(plan, 'bcat', 4, P, planar)
        # d1 d2 d3 r4, block.py:163.  16-bit storage: four dense tensors (engine.Planar) -- a 32-channel slice of a 128-wide
        # buffer is a partial-line store there (64 of 256 bytes per pixel), 2.3x the cost of a dense one
        cat = Concat(plan, 'cat', 4, DP, planar, _pad8(4 * DP))
        cs = cat.seg
        r1, r2 = plan.buffer('r1', P), plan.buffer('r2', P)
        v = plan.buffer('v', P)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        act = dict(act=L.ACT_LRELU, slope=0.05)
        res = (lambda v: dict(res=v, res_mode=L.RES_PRE_ACT)) if self.block_residual else (lambda v: {})
        fused_post = (48 < nf <= 64 and 16 < dc <= 32) if plan.esize == 4 else ((nf + 15) // 16 in (3, 4) and 16 < dc <= 32)
        # 16-bit modes: block 1's first distillation conv (c1_d of fea) rides in the head convolution's epilogue
        # the fused block tail needs rfdb_tail_kernel's shapes (esr_conv_tail_supported has the last word in Plan.finalize)
        fused_tail = (self.fuse_tail and plan.esize == 2 and fused_post and planar and 48 < nf <= 64 and DP == 32 and f <= 16 and FP == 16
                      and plan.n * ((plan.w + 15) // 16) * ((plan.h + 15) // 16) >= 256)
        head_d = plan.esize == 2 and fused_post
        skip.head('fea_conv', self.in_nc, post=Post('B1.c1_d', cs(0), dc, L.ACT_LRELU) if head_d else None)
        # ... and the other blocks' in the ESA apply launch that produces their input (esr_esa_desc.post[])
        apply_d = plan.esize == 2 and fused_post and bool(L.lib().esr_esa_apply_post_supported(nf, dc, 0))
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            if not ((head_d and k == 1) or (apply_d and k > 1)):
                plan.conv(b + 'c1_d', cur, cs(0), nf, dc, k=1, **act)
            if fused_post:
                # the distillation conv of r_j rides in the epilogue of the conv that produces r_j (block.py:150-160)
                plan.conv(b + 'c1_r', cur, r1, nf, nf, **res(cur), **act,
                          post=Post(b + 'c2_d', cs(1), dc, L.ACT_LRELU))
                plan.conv(b + 'c2_r', r1, r2, nf, nf, **res(r1), **act,
                          post=Post(b + 'c3_d', cs(2), dc, L.ACT_LRELU))
            else:
                plan.conv(b + 'c1_r', cur, r1, nf, nf, **res(cur), **act)
                plan.conv(b + 'c2_d', r1, cs(1), nf, dc, k=1, **act)
                plan.conv(b + 'c2_r', r1, r2, nf, nf, **res(r1), **act)
                plan.conv(b + 'c3_d', r2, cs(2), nf, dc, k=1, **act)
            plan.conv(b + 'c3_r', r2, r1, nf, nf, **res(r2), **act)
            if fused_tail:
                # round 6 (ABI v12): c4 -> cat(d1, d2, d3, r4) -> c5 -> esa.conv1 in ONE launch (rfdb_tail_kernel; block.py:161-164, :117):
                # r4 stays in registers, d1 .. d3 are read once, v and esa.conv1's map are the only stores
                plan.conv(b + 'c4', r1, v, nf, dc, tail=Tail(b + 'c5#tail', Planar(cat.whole.segs[:3]), 3 * DP, 3 * dc, nf, L.ACT_LRELU),
                          post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c4', r1, cs(3), nf, dc, **act)
            if fused_tail:
                pass
            elif plan.esize == 2 and (nf + 15) // 16 in (3, 4) and f <= 16:
                # 16-bit storage: esa.conv1 rides in c5's epilogue on the fp32 tile (one launch less per block)
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE))
            else:
                plan.conv(b + 'c5', cat.whole, v, 4 * DP, nf, k=1, cin_alg=4 * dc)
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'esa.conv2', [(b + 'esa.conv_max', L.ACT_RELU), (b + 'esa.conv3', L.ACT_RELU), (b + 'esa.conv3_', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            out = bcat.seg(k - 1)
            nxt_d = [Post(f'B{k + 1}.c1_d', cs(0), dc, L.ACT_LRELU, slope=0.05)] if (apply_d and k < 4) else None
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f, post=nxt_d)
            cur = out
        plan.conv('c.0', bcat.whole, v, 4 * KP, nf, k=1, cin_alg=4 * nf, **act)
        skip.close('LR_conv', 'upsampler.0', v, r1, self.out_nc * 16)

    _cin_map = block_cin_map

    def _extra_pack(self, packed, device):
        if self._store() != "f32" and 48 < self.nf <= 64 and self.dc <= 32:
            from .engine import pack_tail_s16    # c5 over cat(d1, d2, d3, r4) for rfdb_tail_kernel
            for k in range(1, 5):
                leaf = self._leaf(f'B{k}.c5')
                packed[f'B{k}.c5#tail'] = pack_tail_s16(leaf.weight, leaf.bias, 3, self.dc, self.dc, self._store()).to(device)
        if not self.esa_conv_f:                  # SFDN: c3 + c1_  ==  c3 + conv_f(c1_) with conv_f = identity
            for k in range(1, 5):
                packed[f'B{k}.esa.conv_f'] = identity_conv_f(self.f, device)

    def _counted_convs(self, plan, o):
        """what the launches' own counts (Conv.cin_alg: c5 and c.0 carry their logical input channels) leave to say"""
        r = super()._counted_convs(plan, o)
        if o.kind == "apply" and not self.esa_conv_f:
            return r[1:]                         # no conv_f call in the reference graph
        if o.kind == "conv" and o.tail is not None and o.w.endswith('.c4'):      # the fused block tail: c4, c5, esa.conv1
            return [(o.cin, o.cout, 3, plan.npix, L.ACT_LRELU), (self.dc * 4, o.tail.cout, 1, plan.npix, L.ACT_NONE),
                    (o.tail.cout, o.post.cout, 1, plan.npix, L.ACT_NONE)]
        if o.kind == "conv" and o.w.endswith('.c5'):
            return r[:1]                         # (an esa.conv1 riding in c5's epilogue is not counted)
        return r
