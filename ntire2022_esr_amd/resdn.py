"""ResDN (x4) on the HIP engine -- drop-in for `models.team43_resdn.ResDN` (team43_resdn.py:115-182; NTIRE 2022 ESR team 43, test_demo.py id 43,
data_range 1.0).

Same constructor keywords and the same 162 state_dict keys (`sub_mean`, `add_mean`, `fea_conv`, `body_unit{k}.{expansion{j}, compression{j},
conv_tail}.{0 (nn.PReLU), 1}`, `body_unit{k}.attention.{conv1,conv_f,conv_max,conv2,conv3,conv3_,conv4}`, `{T,L}_tdm{j}.0`, `tail.{0,1}`), 406 504
parameters.  n_feats = 48, d = 16: every width of the network -- 48, 64, 80, 96 -- is whole K chunks in every storage, no pitch is padded.

    x0 = fea_conv(sub_mean(x))                                   3 -> 48, 3x3; the mean shift comes BEFORE the zero padding
    ResDB x 4 (team43_resdn.py:48-111); step j = 1, 2, 3 on the block's running x:
        e = expansion{j}.1 . prelu(cat(x, earlier distilled maps)) 1x1, 48 / 64 / 80 -> 96 / 80 / 64;  res, dists = e[:48], e[48:]
        x = x + compression{j}.1 (*) prelu(res)                   3x3, zero padding of prelu(res)
      t = conv_tail.1 . prelu(cat(x, d13, d22, d31)); out = ESA(48, f = 12)(t) + block input
    TDM: three pairs of 1x1 48 -> 24 + ReLU (T over the running concat, L over res3, res2, res1), concatenated; + x0
    tail.0, tail.1 (3x3 48 -> 48), PixelShuffle(4), add_mean

Every nn.PReLU has one slope per channel and PRE-activates a convolution; the raw tensor is read again (the residual, later layers with slopes
of their own), so the activation is the consumer's: ONE esr_prelu launch per convolution (Plan.prelu; v >= 0 ? v : a v -- the checkpoint's
slopes span -1.82 .. +3.62, max(v, a v) is another function) that also gathers the concat, which never runs: the block tail's four sources
go in one launch.  A step is five launches on the existing kernels plus esr_prelu, in every storage:
    u = prelu(cat(..))        esr_prelu -> a dense 48 / 64 / 80-channel tensor
    r = W_e[:48] . u          the expansion 1x1, split into its `res` part (esr_conv2d_f32 stores at most 64 channels) ...
    dists = W_e[48:] . u      ... and its distilled part, stored RAW into the block's 96-channel buffer [d11 d12 d13 | d21 d22 | d31]
    t = prelu(r)              esr_prelu
    x' = x + W_c (*) t        the 3x3 with the pre-activation residual x; x' goes to the other buffer of a ping-pong pair
The block's `+ input` is ESAN's identity 1x1 with the residual (esan.py): a 16-bit plan rounds t * sigmoid(..) once more than the reference's
graph.
  fused (model.fuse_resdb; 16-bit plans) ONE esr_resdb_step launch per step (Plan.resdb_step, resdb_step_kernel): x and the earlier distilled
    maps are read once, the step's distilled maps and x' written once; u, r and t stay in LDS, rounded where the five launches round them.
    Which form a plan takes depends on the flag and esr_resdb_step_supported only, never on the batch size.  Measurements: DESIGN.md 7l.

The mean shifts (MeanShift: 1x1 convolutions with the identity as weight; a checkpoint with another weight is refused, the biases are free):
  add_mean   folds into tail.1's bias (colour c of the shuffled output is channels 16 c .. 16 c + 15).
  sub_mean   must stay exact on the outermost pixels: fea_conv's taps outside the image meet 0, not -mean, so a plain bias fold is wrong there.
             fp32 plans run it as the convolution it is -- an identity centre tap over the NCHW input, bias -mean, into a 3-channel NHWC
             tensor that fea_conv then zero-pads; 16-bit plans keep the input's hi + lo packing (engine.Plan.conv) and fold
             sum_taps W . b_sub into fea_conv's bias, with esr_conv_desc.border_bias taking back the taps that fall outside.
  Either way it is part of the plan: a forward stays one graph launch.
"""
import torch
import torch.nn as nn

from . import _lib as L
from .engine import HEAD, INPUT, OUTPUT, S16, Conv, HipSRModel, Post, pack_conv, pack_conv_s16, pack_head_s16
from .frame import FP, EsaBranch, check_input

IDENT = "ident"            # the blob of the 48 -> 48 identity 1x1 behind every block's `+ input`
RES, DIST = "#res", "#dist"  # the two parts of an expansion 1x1, under its name
MS = "#ms"                 # fea_conv with sub_mean folded in (16-bit plans), and its border table
SUB = "sub_mean#c3"        # sub_mean as a centre-tap 3x3 over the NCHW input (fp32 plans)


class ResDN(HipSRModel):
    def __init__(self, upscale_factor=4, in_channels=3, n_feats=48, out_channels=3):
        super().__init__()
        if upscale_factor != 4 or in_channels != 3 or n_feats != 48 or out_channels != 3:
            raise NotImplementedError('HIP ResDN supports upscale_factor=4, in_channels=3, n_feats=48, out_channels=3')
        self.in_nc, self.out_nc, self.nf, self.upscale = in_channels, out_channels, n_feats, upscale_factor
        self.nd = 16                                       # team43_resdn.py:49
        self.f = n_feats // 4                              # team43_resdn.py:23
        nf, nd, f = self.nf, self.nd, self.f
        self._add_conv('sub_mean', 3, 3, 1, custom=True)
        self._add_conv('add_mean', 3, 3, 1, custom=True)
        self._add_conv('fea_conv', in_channels, nf, 3)
        for k in range(1, 5):
            b = f'body_unit{k}.'
            for j in (1, 2, 3):
                cin = nf + (j - 1) * nd
                self._add_leaf(b + f'expansion{j}.0', nn.PReLU(cin))
                self._add_conv(b + f'expansion{j}.1', cin, nf + (4 - j) * nd, 1, custom=True)
            for j in (1, 2, 3):
                self._add_leaf(b + f'compression{j}.0', nn.PReLU(nf))
                self._add_conv(b + f'compression{j}.1', nf, nf, 3)
            self._add_leaf(b + 'conv_tail.0', nn.PReLU(nf + 3 * nd))
            self._add_conv(b + 'conv_tail.1', nf + 3 * nd, nf, 1)
            self._add_conv(b + 'attention.conv1', nf, f, 1)
            self._add_conv(b + 'attention.conv_f', f, f, 1, dense=(FP, FP))
            self._add_conv(b + 'attention.conv_max', f, f, 3)
            self._add_conv(b + 'attention.conv2', f, f, 3, dense=(FP, FP), stride=2, padding=0)
            self._add_conv(b + 'attention.conv3', f, f, 3)
            self._add_conv(b + 'attention.conv3_', f, f, 3)
            self._add_conv(b + 'attention.conv4', f, nf, 1, dense=(FP, nf))
        for j in (1, 2, 3):
            self._add_conv(f'T_tdm{j}.0', nf, nf // 2, 1)
            self._add_conv(f'L_tdm{j}.0', nf, nf // 2, 1)
        self._add_conv('tail.0', nf, nf, 3)
        self._add_conv('tail.1', nf, out_channels * 16, 3, custom=True)

    def _build_plan(self, plan, c):
        check_input('ResDN', plan, c, self.in_nc)
        nf, nd, f, h = self.nf, self.nd, self.f, self.nf // 2
        s16 = plan.esize == 2
        x0 = plan.buffer('x0', nf)
        outs = [plan.buffer(f'res{k}', nf) for k in range(1, 5)]          # the blocks' outputs: the TDM reads all four
        xa, xb = plan.buffer('xa', nf), plan.buffer('xb', nf)             # a block's running x: x' is never stored over the x it is made from
        us = {cin: plan.buffer(f'u{cin}', cin) for cin in (nf, nf + nd, nf + 2 * nd, nf + 3 * nd)}      # prelu(cat(..)), dense
        r, D = plan.buffer('r', nf), plan.buffer('dists', 6 * nd)        # [d11 d12 d13 | d21 d22 | d31]
        t, g = plan.buffer('t', nf), plan.buffer('g', nf)
        ta, tb = plan.buffer('tdm_a', nf), plan.buffer('tdm_b', nf)
        esa = EsaBranch(plan, f)
        c1 = esa.c1
        d = lambda i: (D[i * nd:(i + 1) * nd], nd)
        if s16:
            plan.conv('fea_conv' + MS, INPUT, x0, self.in_nc, nf, border='fea_conv' + MS + '#border')
        else:
            sm = plan.buffer('sub', plan.cpad(self.in_nc))
            plan.conv(SUB, INPUT, sm, self.in_nc, 4)           # (a fourth output of zeros: whole 16-byte granules)
            plan.conv('fea_conv', sm, x0, self.in_nc, nf)
        cur = x0
        for k in range(1, 5):
            b = f'body_unit{k}.'
            x = cur
            # the distilled maps each step reads next to x, and where its own go (team43_resdn.py:93-108)
            for j, (extra, (lo, hi)) in enumerate((((), (0, 3)), ((d(0),), (3, 5)), ((d(1), d(3)), (5, 6))), start=1):
                cin = nf + (j - 1) * nd
                e = b + f'expansion{j}.'
                nxt = xb if x is xa else xa
                plan.prelu(e + '0', [(x, nf), *extra], us[cin])
                plan.conv(e + '1' + RES, us[cin], r, cin, nf, k=1)
                plan.conv(e + '1' + DIST, us[cin], D[lo * nd:hi * nd], cin, (hi - lo) * nd, k=1, counted=False)
                plan.prelu(b + f'compression{j}.0', [(r, nf)], us[nf])
                mark = len(plan.ops) - 4
                plan.conv(b + f'compression{j}.1', us[nf], nxt, nf, nf, res=x, res_mode=L.RES_PRE_ACT)
                if self.fuse_resdb and s16:
                    plan.resdb_step(mark, whole=e + '1')   # (where the kernel takes the step; else the five launches stay)
                x = nxt
            plan.prelu(b + 'conv_tail.0', [(x, nf), d(2), d(4), d(5)], us[nf + 3 * nd])
            tail = dict(w=b + 'conv_tail.1', src=us[nf + 3 * nd], dst=t, cin=nf + 3 * nd, cout=nf, k=1)
            ride = Conv(**tail, post=Post(b + 'attention.conv1', c1, f, L.ACT_NONE)) if s16 else None
            if ride is not None and plan.post_supported(ride):
                plan.ops.append(ride)                     # attention.conv1 on the fp32 tile in conv_tail's epilogue (rfdn.py)
            else:
                plan.ops.append(Conv(**tail))
                plan.conv(b + 'attention.conv1', t, c1, nf, f, k=1)
            c3 = esa.lowres(b + 'attention.conv2', [(b + 'attention.conv_max', L.ACT_RELU), (b + 'attention.conv3', L.ACT_RELU),
                                                    (b + 'attention.conv3_', L.ACT_NONE)], self.fuse_esa_lowres)
            plan.esa_apply(b + 'attention.conv_f', b + 'attention.conv4', t, c1, c3, g, nf, f)
            plan.conv(IDENT, g, outs[k - 1], nf, nf, k=1, res=cur, res_mode=L.RES_PRE_ACT, counted=False)      # res + input
            cur = outs[k - 1]
        relu = dict(k=1, act=L.ACT_RELU)
        plan.conv('T_tdm1.0', outs[3], ta[0:h], nf, h, **relu)
        plan.conv('L_tdm1.0', outs[2], ta[h:nf], nf, h, **relu)
        plan.conv('T_tdm2.0', ta, tb[0:h], nf, h, **relu)
        plan.conv('L_tdm2.0', outs[1], tb[h:nf], nf, h, **relu)
        plan.conv('T_tdm3.0', tb, ta[0:h], nf, h, res=x0[0:h], res_mode=L.RES_POST_ACT, **relu)              # out_TDM3 + x0
        plan.conv('L_tdm3.0', outs[0], ta[h:nf], nf, h, res=x0[h:nf], res_mode=L.RES_POST_ACT, **relu)
        plan.conv('tail.0', ta, t, nf, nf)
        plan.conv('tail.1', t, OUTPUT, nf, self.out_nc * 16)

    def _mean_shifts(self):
        """(sub_mean.bias, add_mean.bias) as fp32 CPU tensors; refuses a checkpoint whose mean-shift weights are not the identity"""
        eye = torch.eye(3)[:, :, None, None]
        out = []
        for name in ('sub_mean', 'add_mean'):
            leaf = self._leaf(name)
            w = leaf.weight.detach().to("cpu", torch.float32)
            if not torch.equal(w, eye):
                raise L.EsrError(f'HIP ResDN: {name}.weight is not the 3x3 identity -- the plan folds the mean shifts into the biases of fea_conv '
                                 'and tail.1, which only a pure shift allows (MeanShift with rgb_std = 1, team43_resdn.py:7-17)')
            out.append(leaf.bias.detach().to("cpu", torch.float32))
        return out

    def _extra_pack(self, packed, device):
        store = self._store()
        s16 = store != "f32"
        cpu = lambda p: p.detach().to("cpu", torch.float32)
        nf = self.nf
        b_sub, b_add = self._mean_shifts()
        eye, zero = torch.eye(nf)[:, :, None, None], torch.zeros(nf)
        self._pack_own(packed, device, IDENT, eye, zero)
        for k in range(1, 5):
            b = f'body_unit{k}.'
            for j in (1, 2, 3):
                leaf = self._leaf(b + f'expansion{j}.1')
                w, bias = cpu(leaf.weight), cpu(leaf.bias)
                for sfx, sl in ((RES, slice(0, nf)), (DIST, slice(nf, None))):
                    self._pack_own(packed, device, b + f'expansion{j}.1' + sfx, w[sl].contiguous(), bias[sl].contiguous())
                if s16 and self.fuse_resdb:               # the one-launch step: the whole expansion as one image
                    packed[b + f'expansion{j}.1' + S16] = pack_conv_s16(w, bias, store).to(device)
        # add_mean into tail.1's bias: colour c of the shuffled output is channels 16 c .. 16 c + 15
        leaf = self._leaf('tail.1')
        w, bias = cpu(leaf.weight), cpu(leaf.bias) + b_add.repeat_interleave(16)
        self._pack_own(packed, device, 'tail.1', w, bias, wino=True)
        # sub_mean
        wf, bf = cpu(self._leaf('fea_conv').weight), cpu(self._leaf('fea_conv').bias)
        if s16:
            # fea_conv(x + b_sub) with zero padding: inside, every tap meets b_sub; row m of the table takes back the taps outside for mask m
            # (bit 0: x == 0, bit 1: x == w - 1, bit 2: y == 0, bit 3: y == h - 1)
            tap = torch.einsum('ocij,c->oij', wf.double(), b_sub.double())          # [48, 3, 3]: what one tap adds
            table = torch.zeros(16, nf, dtype=torch.float64)
            for m in range(1, 16):
                out = torch.zeros(3, 3, dtype=torch.bool)
                if m & 1: out[:, 0] = True
                if m & 2: out[:, 2] = True
                if m & 4: out[0, :] = True
                if m & 8: out[2, :] = True
                table[m] = -(tap * out.double()).sum(dim=(1, 2))
            packed['fea_conv' + MS + HEAD + S16] = pack_head_s16(wf, (bf.double() + tap.sum(dim=(1, 2))).float(), store).to(device)
            packed['fea_conv' + MS + '#border'] = table.float().contiguous().to(device)
        else:
            w3 = torch.zeros(4, 3, 3, 3)
            w3[torch.arange(3), torch.arange(3), 1, 1] = 1.0
            packed[SUB] = pack_conv(w3, torch.cat([b_sub, torch.zeros(1)])).to(device)

    def _counted_convs(self, plan, o):
        """the reference's hooks see both MeanShifts as 1x1 convolutions (3 -> 3; add_mean on the 4H x 4W output) and an expansion as ONE"""
        r = super()._counted_convs(plan, o)
        if o.kind != "conv":
            return r
        if o.w == SUB:
            return [(3, 3, 1, plan.npix, L.ACT_NONE)]
        if o.w.startswith('fea_conv' + MS):
            return [(3, 3, 1, plan.npix, L.ACT_NONE)] + r
        if o.w == 'tail.1':
            return r + [(3, 3, 1, 16 * plan.npix, L.ACT_NONE)]
        if o.w.endswith(RES):                            # + the distilled part, which is `counted=False`
            j = int(o.w.split('expansion')[1][0])
            return [(o.cin, self.nf + (4 - j) * self.nd, 1, plan.npix, L.ACT_NONE)]
        return r

    def _complexity_terms(self, plan, o):
        if o.kind == "resdb":
            terms = [self._complexity_terms(plan, q) for q in o.replaces]
            return tuple(sum(t[i] for t in terms) for i in range(3))
        if o.kind == "prelu":                            # one flop per element of an nn.PReLU's output, like the ReLU family
            return o.prelu_elements(plan), 0, 0
        return super()._complexity_terms(plan, o)
