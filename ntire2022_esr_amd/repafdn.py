"""RePAFDN (x4) on the HIP engine -- drop-in for `models.team10_repafdn.repafdn.RePAFDN` (repafdn.py:14-59 + block.py; NTIRE 2022 ESR team 10,
test_demo.py id 10, data_range 1.0).

Same constructor keywords and the same 118 state_dict keys (`fea_conv`, `B{1,2,3}.{c1_d,c1_r,c2_d,c2_r,c4,c5}`, `B4.{c1_d .. c3_r,c4,c5}`,
`B{k}.esa.{conv1,conv_f,conv_max,conv2,conv3,conv3_,conv4}`, `c.0`, `LR_conv`, `pa.conv`, `upsampler.0`).  It is RFDN's frame (frame.py) at
nf = 48 without a block residual, with LeakyReLU(0.05), ReLU and sigmoid only (act_type "lrelu"):

  B1 .. B3   FDB_S (block.py:216-254): two distillation steps, dc = 24, c5 over cat(d1, d2, r4) = 72 -> 48
  B4         FDB   (block.py:169-213): three steps, dc = int(48 * ds_rate) = 12, c5 over cat(d1, d2, d3, r4) = 48 -> 48
  every block ends in the baseline ESA with f = 12 and all seven of its convolutions (block.py:113-142)

and the end of the forward (repafdn.py:55-58), the one piece no other network has:

    t      = LR_conv(out_B)                 3x3, 48 -> 48
    out_lr = t * sigmoid(pa.conv(t)) + fea  PA (block.py:151-166): a 1x1 48 -> 48 that gates its own input, then the long skip
    y      = upsampler(out_lr)

It has two forms (model.fuse_pa_tail):
  per-op   the LR convolution, then the gate and the skip as ONE esr_pa_gate launch (Plan.pa_gate, pa_gate_kernel; every storage): t is
           stored once in the plan's storage type in between; t and `fea` are read once, out_lr is written once.  The only form of an
           fp32 plan.
  fused    ONE esr_pa_tail launch for all three (Plan.pa_tail, pa_tail_kernel; 16-bit plans): t stays in the fp32 accumulators, only its
           copy rounded to the storage type feeds the gate's 1x1.  Differs from the per-op form by the rounding of t.  OFF by default: measured
           2 % slower than the two launches at 32 x 256 x 256 and on one 339 x 510 image.
In a bf16 plan `fea` and `out_lr` are hi + lo pairs (LongSkip; LAB_NOTES 9.4) and both kernels add and split them in fp32.  Which form a
plan takes depends on the flag, the per-image shape and esr_pa_tail_supported only, never on the batch size.

The layouts: nf = 48 is whole K chunks in every storage (pitch 48); the 24-channel maps of B1 .. B3 live in 32-wide tensors, the 12-channel
maps of B4 in 16-wide ones -- the concats as dense tensors in 16-bit plans (engine.Planar), as slices of one buffer in fp32 -- read by c5
through `_slice_map`; the block outputs as four 48-wide tensors read by c.0.  torch.cat never runs.

The rides are rfdn.py's, each taken where RFDN's own condition holds AND the kernel's predicate accepts the descriptor (Plan.post_supported), and launched as an
op of its own otherwise (16-bit plans only; an fp32 plan at nf = 48 has none): c{j+1}_d in the epilogue of c{j}_r (dc = 24: B1 .. B3),
B1.c1_d in the head convolution, the next block's c1_d in the ESA apply launch, esa.conv1 in c5's epilogue.
"""
from . import _lib as L
from .engine import HEAD, OUTPUT, Buffer, Conv, HipSRModel, Post
from .frame import FP, Concat, EsaBranch, LongSkip, _slice_map, block_cin_map, check_input, set_scale


class RePAFDN(HipSRModel):
    def __init__(self, in_nc=3, nf=48, out_nc=3, upscale=4, act_type="lrelu", ds_rate=0.25, rgb_range=255.0, dc=24):
        super().__init__()
        if upscale != 4 or nf != 48 or act_type != "lrelu" or ds_rate != 0.25 or dc != 24 or in_nc > 4 or out_nc > 4:
            raise NotImplementedError('HIP RePAFDN supports upscale=4, nf=48, act_type="lrelu", ds_rate=0.25, dc=24, in_nc <= 4, out_nc <= 4')
        self.in_nc, self.out_nc, self.nf, self.upscale, self.rgb_range = in_nc, out_nc, nf, upscale, rgb_range
        self.num_modules = 4
        self.dc, self.dc4 = dc, int(nf * ds_rate)            # FDB_S (B1 .. B3) / FDB (B4: block.py:181)
        self.f = nf // 4                                     # block.py:117
        self.DP, self.DP4 = (self.dc + 31) // 32 * 32, (self.dc4 + 15) // 16 * 16
        self.scale_idx = 0
        f = self.f
        self._add_conv('fea_conv', in_nc, nf, 3)
        for k in range(1, 5):
            b = f'B{k}.'
            steps, bdc, pitch = self._block(k)
            for j in range(1, steps + 1):
                self._add_conv(b + f'c{j}_d', nf, bdc, 1)
                self._add_conv(b + f'c{j}_r', nf, nf, 3)
            self._add_conv(b + 'c4', nf, bdc, 3)
            self._add_conv(b + 'c5', bdc * (steps + 1), nf, 1, cin_map=_slice_map(steps + 1, bdc, pitch))
            self._add_conv(b + 'esa.conv1', nf, f, 1)
            self._add_conv(b + 'esa.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'esa.conv_max', f, f, 3)
            self._add_conv(b + 'esa.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'esa.conv3', f, f, 3)
            self._add_conv(b + 'esa.conv3_', f, f, 3)
            self._add_conv(b + 'esa.conv4', f, nf, 1, dense=(FP, nf))
        self._add_conv('c.0', nf * 4, nf, 1, cin_map=_slice_map(4, nf, nf))
        self._add_conv('LR_conv', nf, nf, 3)
        self._add_conv('pa.conv', nf, nf, 1, custom=True)    # packed for Plan.pa_gate (pack_pa_gate)
        self._add_conv('upsampler.0', nf, out_nc * upscale * upscale, 3)

    def _block(self, k):
        """(distillation steps, distilled channels, their pitch in the concat) of block k"""
        return (2, self.dc, self.DP) if k < 4 else (3, self.dc4, self.DP4)

    set_scale = set_scale

    def _build_plan(self, plan, c):
        check_input('RePAFDN', plan, c, self.in_nc)
        nf, f = self.nf, self.f
        s16 = plan.esize == 2
        P = plan.cpad(nf)                                 # 48 in every storage: whole K chunks
        skip = LongSkip(plan, self, nf, P)
        bcat = Concat(plan, 'bcat', 4, P, s16)
        cat3 = Concat(plan, 'cat', 3, self.DP, s16)       # d1 d2 r4 of FDB_S, block.py:251
        cat4 = Concat(plan, 'cat4', 4, self.DP4, s16)     # d1 d2 d3 r4 of FDB, block.py:210
        r1, r2 = plan.buffer('r1', P), plan.buffer('r2', P)
        v = plan.buffer('v', P)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        act = dict(act=L.ACT_LRELU, slope=0.05)
        d_post = lambda k, j, dst: Post(f'B{k}.c{j}_d', dst, self._block(k)[1], L.ACT_LRELU, slope=0.05)
        # rfdn.py's rides: its own condition on the shape and the kernel's predicate, both
        rides = lambda k: s16 and 16 < self._block(k)[1] <= 32
        head_d = rides(1) and plan.post_supported(Conv('fea_conv' + HEAD, Buffer('in16', 16, 0, esize=2), skip.dst, self.in_nc, nf, head=self.in_nc,
                                                     hilo=L.HILO_OUT if skip.hl else 0, post=d_post(1, 1, cat3.seg(0))))
        skip.head('fea_conv', self.in_nc, post=d_post(1, 1, cat3.seg(0)) if head_d else None)
        apply_d = lambda k: k <= 4 and rides(k) and bool(L.lib().esr_esa_apply_post_supported(nf, self._block(k)[1], 0))
        cur = skip.fea
        for k in range(1, 5):
            b = f'B{k}.'
            steps, dc, pitch = self._block(k)
            cat = cat3 if k < 4 else cat4
            cs = cat.seg
            if not ((head_d and k == 1) or (k > 1 and apply_d(k))):
                plan.conv(b + 'c1_d', cur, cs(0), nf, dc, k=1, **act)
            src, dst = cur, r1
            for j in range(1, steps + 1):
                # r_j = act(c{j}_r(r_{j-1})) (no block residual); d_{j+1} = act(c{j+1}_d(r_j)) rides in its epilogue where a kernel takes it
                ride = Conv(b + f'c{j}_r', src, dst, nf, nf, **act, post=d_post(k, j + 1, cs(j))) if (j < steps and rides(k)) else None
                if ride is not None and plan.post_supported(ride):
                    plan.ops.append(ride)
                else:
                    plan.conv(b + f'c{j}_r', src, dst, nf, nf, **act)
                    if j < steps:
                        plan.conv(b + f'c{j + 1}_d', dst, cs(j), nf, dc, k=1, **act)
                src, dst = dst, (r2 if dst is r1 else r1)
            plan.conv(b + 'c4', src, cs(steps), nf, dc, **act)
            c5 = dict(w=b + 'c5', src=cat.whole, dst=v, cin=(steps + 1) * pitch, cout=nf, k=1, cin_alg=(steps + 1) * dc)
            ride = Conv(**c5, post=Post(b + 'esa.conv1', c1, f, L.ACT_NONE)) if s16 else None
            if ride is not None and plan.post_supported(ride):
                plan.ops.append(ride)                     # esa.conv1 on the fp32 tile in c5's epilogue
            else:
                plan.ops.append(Conv(**c5))
                plan.conv(b + 'esa.conv1', v, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'esa.conv2', [(b + 'esa.conv_max', L.ACT_RELU), (b + 'esa.conv3', L.ACT_RELU), (b + 'esa.conv3_', L.ACT_NONE)],
                            self.fuse_esa_lowres)
            out = bcat.seg(k - 1)
            nxt = [d_post(k + 1, 1, (cat3 if k + 1 < 4 else cat4).seg(0))] if (k < 4 and apply_d(k + 1)) else None
            plan.esa_apply(b + 'esa.conv_f', b + 'esa.conv4', v, c1, c3, out, nf, f, post=nxt)
            cur = out
        plan.conv('c.0', bcat.whole, v, 4 * P, nf, k=1, cin_alg=4 * nf, **act)
        # the end of the long skip, repafdn.py:55-58: t = LR_conv(out_B); out_lr = t * sigmoid(pa.conv(t)) + fea; upsampler(out_lr)
        mark = len(plan.ops)
        plan.conv('LR_conv', v, r1, nf, nf)
        if skip.hl:
            plan.pa_gate('pa.conv', r1, skip.out, nf, s=skip.dst, hilo=L.HILO_RES | L.HILO_OUT)
        else:
            plan.pa_gate('pa.conv', r1, r2, nf, s=skip.fea)
        if self.fuse_pa_tail and s16:
            plan.pa_tail(mark)                            # ONE launch for the two (esr_pa_tail_supported has the last word)
        if skip.hl:
            plan.conv('upsampler.0', skip.out, OUTPUT, nf, self.out_nc * 16, hilo=L.HILO_IN)
        else:
            plan.conv('upsampler.0', r2, OUTPUT, nf, self.out_nc * 16)

    _cin_map = block_cin_map
